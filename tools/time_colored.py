"""Times colored ICP (params.metric = 4) against GICP and point-to-plane on two inputs -- a 640 x 480 depth frame's cloud downsampled by 8
(synth.rgbd_pair(0), max distance 0.1) and the 370 488-point ETH-like pair (synth.eth_like_pair(0), max distance 10), both with colours.
k-NN (LBVH), 20 iterations from the identity, stage timing off.  Per input:
  * device time per ICP iteration (icp_get_timing total / iterations, median of --reps runs after one warm-up): colored (k = 20,
    lambda = 0.968), GICP (k = 20), point-to-plane in the default merged loop, point-to-plane with ICP_HIP_MERGE=0;
  * preparation of the target's colour gradients at k = 10 and 20 (wall time of icp_get_color_gradients on a dropped cache, its copy of
    n x 12 bytes back included; median of --reps);
  * pose error against gt after the 20 iterations, point-to-plane and colored.
Then the textured plane of tests/colored_restatement.py (40 iterations, max distance 0.01): pose error of colored and point-to-plane.
usage: python tools/time_colored.py [--reps 5] [--inputs depth,eth] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding, synth

from time_gicp import context, per_iteration_ms, pose_err


def load(name):
    if name == "depth":
        r = synth.rgbd_pair(0)
        sp, sn, sc = synth.compact_valid(r["src_pts"][::8], r["src_nrm"][::8], r["src_rgba"][::8])
        tp, tn, tc = synth.compact_valid(r["tgt_pts"][::8], r["tgt_nrm"][::8], r["tgt_rgba"][::8])
        return sp, sn, sc, tp, tn, tc, 0.1, r["gt"]
    p = synth.eth_like_pair(0)
    return p["src_pts"], p["src_nrm"], p["src_rgba"], p["tgt_pts"], p["tgt_nrm"], p["tgt_rgba"], 10.0, p["gt"]


def plane_errors():
    import colored_restatement as CR
    d = CR.textured_plane()
    out = {}
    for label, metric in (("colored", 4), ("p2plane", 1)):
        c = context(metric, 0.01)
        c.params.n_iterations = 40
        c.push_params()
        c.set_target(d["tgt_pts"], d["tgt_nrm"], d["tgt_rgba"]); c.set_source(d["src_pts"], d["src_nrm"], d["src_rgba"])
        pose, _, rc = c.run(np.eye(4, dtype=np.float32), check=False)
        ang, tr = pose_err(pose, d["gt"])
        out["plane_%s_err_rad" % label], out["plane_%s_err_m" % label], out["plane_%s_status" % label] = ang, tr, rc
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inputs", default="depth,eth")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.inputs.split(","):
        sp, sn, sc, tp, tn, tc, md, gt = load(name)
        row = dict(input=name, n_src=int(len(sp)), n_tgt=int(len(tp)))
        poses = {}
        for label, metric, merge in (("colored", 4, True), ("gicp", 3, True), ("p2plane_merged", 1, True), ("p2plane_separate", 1, False)):
            c = context(metric, md, merge)
            c.set_target(tp, tn, tc); c.set_source(sp, sn, sc)
            row[label + "_ms_per_it"], poses[label] = per_iteration_ms(c, a.reps)
            if metric == 4:
                for k in (10, 20):
                    ts = []
                    for _ in range(a.reps + 1):
                        c.set_colored_options(0.968, k)   # drops the cache
                        t0 = time.perf_counter(); c.color_gradients(); ts.append(time.perf_counter() - t0)
                    row["gradients_k%d_ms" % k] = statistics.median(ts[1:]) * 1e3
            c.close()
        for label in ("p2plane_merged", "colored"):
            ang, tr = pose_err(poses[label], gt)
            row[label + "_err_rad"], row[label + "_err_m"] = ang, tr
        rows.append(row)
        print(json.dumps(row), flush=True)
    row = plane_errors()
    rows.append(row)
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
