"""Times trimmed ICP + Huber (icp_set_robust_options("huber", overlap=0.7)) against plain point-to-plane on three inputs -- the bunny pair
(tests/golden/bunny_pair.npz, max distance 0.0003), a 640 x 480 depth frame's cloud downsampled by 8 (synth.rgbd_pair(0), max distance
0.1) and the 370 488-point ETH-like pair (synth.eth_like_pair(0), max distance 10).  Point-to-plane, k-NN (LBVH), 20 iterations from the
identity, stage timing off.  Per input: device time per ICP iteration (icp_get_timing total / iterations, median of --reps runs after one
warm-up) with robust mode off (the default merged loop), off with ICP_HIP_MERGE=0 (separate matcher / post / reduce launches, the form
robust mode runs in) and on.
usage: python tools/time_robust.py [--reps 5] [--inputs bunny,depth,eth] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.dirname(__file__))
sys.path.insert(0, ROOT)
from time_gicp import context, load, per_iteration_ms   # noqa: E402  (same inputs, contexts and timing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inputs", default="bunny,depth,eth")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.inputs.split(","):
        sp, sn, tp, tn, md, gt = load(name)
        row = dict(input=name, n_src=int(len(sp)), n_tgt=int(len(tp)))
        for label, merge, robust in (("off_merged", True, False), ("off_separate", False, False), ("trim_huber", True, True)):
            c = context(1, md, merge)
            if robust:
                c.set_robust_options("huber", overlap=0.7)
            c.set_target(tp, tn); c.set_source(sp, sn)
            row[label + "_ms_per_it"], _ = per_iteration_ms(c, a.reps)
            c.close()
        row["ratio_vs_merged"] = row["trim_huber_ms_per_it"] / row["off_merged_ms_per_it"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
