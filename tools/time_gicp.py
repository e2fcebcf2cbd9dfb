"""Times Generalized-ICP (params.metric = 3) against point-to-plane on three inputs -- the bunny pair (tests/golden/bunny_pair.npz, max
distance 0.0003), a 640 x 480 depth frame's cloud downsampled by 8 (synth.rgbd_pair(0), max distance 0.1) and the 370 488-point ETH-like
pair (synth.eth_like_pair(0), max distance 10).  k-NN (LBVH), 20 iterations from the identity, stage timing off.  Per input:
  * device time per ICP iteration (icp_get_timing total / iterations, median of --reps runs after one warm-up): GICP (k = 20),
    point-to-plane in the default merged loop, point-to-plane with ICP_HIP_MERGE=0 (separate matcher / reduce launches);
  * preparation of the GICP normals of the target at k = 10 and 20 (wall time of icp_get_gicp_normals on a dropped cache, its copy of
    n x 12 bytes back included; median of --reps);
  * pose error against gt after the 20 iterations, point-to-plane and GICP (the noisy synthetic pairs: depth and eth).
usage: python tools/time_gicp.py [--reps 5] [--inputs bunny,depth,eth] [--json out.json]"""
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


def load(name):
    if name == "bunny":
        d = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pair.npz"))
        return d["src_pts"], d["src_nrm"], d["tgt_pts"], d["tgt_nrm"], 0.0003, None
    if name == "depth":
        r = synth.rgbd_pair(0)
        sp, sn, _ = synth.compact_valid(r["src_pts"][::8], r["src_nrm"][::8], r["src_rgba"][::8])
        tp, tn, _ = synth.compact_valid(r["tgt_pts"][::8], r["tgt_nrm"][::8], r["tgt_rgba"][::8])
        return sp, sn, tp, tn, 0.1, r["gt"]
    p = synth.eth_like_pair(0)
    return p["src_pts"], p["src_nrm"], p["tgt_pts"], p["tgt_nrm"], 10.0, p["gt"]


def context(metric, md, merge=True):
    old = os.environ.get("ICP_HIP_MERGE")
    if not merge:
        os.environ["ICP_HIP_MERGE"] = "0"                 # read when the context is created
    try:
        c = binding.Context(0)
    finally:
        if not merge:
            if old is None:
                del os.environ["ICP_HIP_MERGE"]
            else:
                os.environ["ICP_HIP_MERGE"] = old
    p = c.params
    p.metric, p.matching, p.knn_backend, p.n_iterations, p.max_distance = metric, 0, 1, 20, md
    c.push_params()
    c.set_stage_timing(0)
    return c


def per_iteration_ms(c, reps):
    eye = np.eye(4, dtype=np.float32)
    pose, _, _ = c.run(eye, check=False)                  # warm-up (index build, levels, GICP normals, allocations)
    ts = []
    for _ in range(reps):
        c.run(eye, check=False)
        t = c.timing()
        ts.append(t["total_ms"] / max(t["iterations"], 1))
    return statistics.median(ts), pose


def pose_err(A, B):
    from conftest import pose_error
    return pose_error(A, B)


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
        poses = {}
        for label, metric, merge in (("gicp", 3, True), ("p2plane_merged", 1, True), ("p2plane_separate", 1, False)):
            c = context(metric, md, merge)
            c.set_target(tp, tn); c.set_source(sp, sn)
            row[label + "_ms_per_it"], poses[label] = per_iteration_ms(c, a.reps)
            if metric == 3:
                for k in (10, 20):
                    ts = []
                    for _ in range(a.reps + 1):
                        c.set_gicp_options(1e-3, k)       # drops the cache
                        t0 = time.perf_counter(); c.gicp_normals("target"); ts.append(time.perf_counter() - t0)
                    row["normals_k%d_ms" % k] = statistics.median(ts[1:]) * 1e3
            c.close()
        if gt is not None:
            for label in ("p2plane_merged", "gicp"):
                ang, tr = pose_err(poses[label], gt)
                row[label + "_err_rad"], row[label + "_err_m"] = ang, tr
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
