"""Times global registration (icp_register_global and the multi-start refinement behind it, globalreg.align) stage by stage on three
inputs -- the bunny pair (tests/golden/bunny_pair.npz, max distance 0.0003, inlier distance 5 mm), a 640 x 480 depth frame's cloud
downsampled by 8 (synth.rgbd_pair(0), max distance 0.1, inlier distance 5 cm) and the 370 488-point ETH-like pair (synth.eth_like_pair(0),
max distance 10, inlier distance 0.5 m) at feature_stride 1, 4 and 16.  k = 20, mutual matches, 4096 hypotheses, n_best = 16, point-to-plane,
LBVH, 20 iterations.  Wall times of the entry points (each ends in a stream synchronise), median of --reps after one warm-up:
  * features_ms : icp_compute_features(both) on a dropped cache (trees of the clouds included where they have to be built);
  * match_ms    : icp_match_features with the features cached (both directions, the compaction and the copy of the pairs);
  * ransac_ms   : icp_register_global with the features cached, minus match_ms (fit, score, the copy of the records, the host's ranking);
  * refine_ms   : icp_run_multistart from the 16 returned poses;
  * cpu_*_s     : the numpy restatement (tests/global_restatement.py) of the same stages, on inputs of at most --cpu-max points (its
                  neighbour search is quadratic); the only comparison there is.
Also per row: M (the number of pairs), valid hypotheses, the best hypothesis' inliers, and the pose error of the best RANSAC pose and of
the refined pose against gt where the input has one.
usage: python tools/time_global.py [--reps 5] [--inputs bunny,depth,eth] [--strides 1,4,16] [--cpu-max 2000] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from time_gicp import context, load, pose_err   # noqa: E402  (same inputs and contexts)
import numpy as np                               # noqa: E402

INLIER = {"bunny": 0.005, "depth": 0.05, "eth": 0.5}


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inputs", default="bunny,depth,eth")
    ap.add_argument("--strides", default="1,4,16")
    ap.add_argument("--cpu-max", type=int, default=2000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.inputs.split(","):
        sp, sn, tp, tn, md, gt = load(name)
        strides = [int(s) for s in a.strides.split(",")] if name == "eth" else [1]
        for stride in strides:
            c = context(1, md)
            c.set_target(tp, tn); c.set_source(sp, sn)
            opts = dict(k=20, feature_stride=stride, mutual=1, n_hypotheses=4096, inlier_distance=INLIER[name], n_best=16)
            feat, match, reg, refine = [], [], [], []
            for r in range(a.reps + 1):
                c.set_global_options(**opts)                     # drops the cache
                t_f, _ = wall_ms(lambda: c.compute_features("both"))
                t_m, (si, ti) = wall_ms(c.match_features)
                t_r, (poses, recs, _) = wall_ms(c.register_global)
                t_x, (results, _, best) = wall_ms(lambda: c.run_multistart(poses))
                if r > 0:                                        # (the first round is the warm-up)
                    feat.append(t_f); match.append(t_m); reg.append(t_r); refine.append(t_x)
            hyp = c.global_hypotheses()
            row = dict(input=name, n_source=int(len(sp)), n_target=int(len(tp)), feature_stride=stride, reps=a.reps,
                       features_ms=statistics.median(feat), match_ms=statistics.median(match),
                       ransac_ms=statistics.median([x - y for x, y in zip(reg, match)]), refine_ms=statistics.median(refine),
                       M=int(len(si)), valid=int((hyp["status"] == 0).sum()), best_inliers=int(recs[0]["n_inliers"]))
            if gt is not None:
                row["ransac_err"] = pose_err(poses[0], gt); row["refined_err"] = pose_err(results[best]["pose"], gt)
            if max(len(sp), len(tp)) <= a.cpu_max:
                import global_restatement as gr
                t0 = time.perf_counter()
                fs = gr.features(sp, sn, 20, stride); ft = gr.features(tp, tn, 20, stride)
                t1 = time.perf_counter()
                ei, et = gr.correspondences(fs["F"], ft["F"], stride, True)
                t2 = time.perf_counter()
                gr.ransac(sp[ei], tp[et], 0, 4096, 0.9, INLIER[name])
                t3 = time.perf_counter()
                row.update(cpu_features_s=t1 - t0, cpu_match_s=t2 - t1, cpu_ransac_s=t3 - t2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            c.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
