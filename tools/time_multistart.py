"""Times multi-start ICP: K sequential icp_run calls (one per start) against ONE icp_run_multistart call with the same K starts, for
K in {1, 4, 16, 64} on three inputs -- the bunny pair (tests/golden/bunny_pair.npz, max distance 0.0003), a 640 x 480 depth frame's cloud
downsampled by 8 (synth.rgbd_pair(0), max distance 0.1) and the 370 488-point ETH-like pair (synth.eth_like_pair(0), max distance 10).
k-NN (LBVH), point-to-plane, 20 ICP iterations per start; the starts are the identity turned by small yaws about the source's centroid
(multistart.start_poses).  Wall time of the host call (its one synchronisation included), median of --reps after one warm-up.
usage: python tools/time_multistart.py [--reps 5] [--ks 1,4,16,64] [--inputs bunny,depth,eth] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding, synth
from icp_amd.multistart import start_poses


def load(name):
    if name == "bunny":
        d = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pair.npz"))
        return d["src_pts"], d["src_nrm"], d["tgt_pts"], d["tgt_nrm"], 0.0003
    if name == "depth":
        r = synth.rgbd_pair(0)
        sp, sn, _ = synth.compact_valid(r["src_pts"][::8], r["src_nrm"][::8], r["src_rgba"][::8])
        tp, tn, _ = synth.compact_valid(r["tgt_pts"][::8], r["tgt_nrm"][::8], r["tgt_rgba"][::8])
        return sp, sn, tp, tn, 0.1
    p = synth.eth_like_pair(0)
    return p["src_pts"], p["src_nrm"], p["tgt_pts"], p["tgt_nrm"], 10.0


def median_time(fn, reps):
    fn()                                                     # warm-up (index build, levels, allocations)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--inputs", default="bunny,depth,eth")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.inputs.split(","):
        sp, sn, tp, tn, md = load(name)
        c = binding.Context(0)
        p = c.params
        p.metric, p.matching, p.knn_backend, p.n_iterations, p.max_distance = 1, 0, 1, 20, md
        c.push_params()
        c.set_target(tp, tn); c.set_source(sp, sn)
        for K in (int(k) for k in a.ks.split(",")):
            starts = start_poses(np.eye(4), yaw_deg=np.linspace(-6.0, 6.0, K) if K > 1 else [0.0], axis=(0, 1, 0), points=sp)
            seq = median_time(lambda: [c.run(s, max_stats=64, check=False) for s in starts], a.reps)
            multi = median_time(lambda: c.run_multistart(starts, max_stats=64), a.reps)
            row = dict(input=name, n_src=int(len(sp)), K=K, sequential_ms=seq * 1e3, multistart_ms=multi * 1e3, speedup=seq / multi)
            rows.append(row)
            print("%-6s n=%6d K=%3d  sequential %9.3f ms  multistart %9.3f ms  x%.2f" % (name, len(sp), K, seq * 1e3, multi * 1e3, seq / multi), flush=True)
        c.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
