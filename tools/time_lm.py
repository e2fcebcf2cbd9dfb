"""Times the non-linear optimiser against the linear one on the 370 488-point ETH-like pair (synth.eth_like_pair(0)): k-NN (LBVH),
point-to-plane, 20 ICP iterations per run, max distance 10 (bench.py's setting), median of --reps runs after one warm-up run.
  linear     : icp_run with the linear optimiser (the bench workload)
  nonlinear  : the same run with icp_set_optimizer (one Levenberg-Marquardt solve of at most 10 iterations per ICP iteration)
Reports ICP iterations/s of each and the LM iterations the solves ran.  Kernel times of k_lm_eval / k_lm_step come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool with --only-nonlinear.
usage: python tools/time_lm.py [--reps 5] [--json out.json] [--only-nonlinear]"""
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


def make(pair, nonlinear):
    c = binding.Context(0)
    p = c.params
    p.metric, p.matching, p.knn_backend, p.n_iterations, p.max_distance, p.rejection = 1, 0, 1, 20, 10.0, 1
    c.push_params()
    c.set_target(pair["tgt_pts"], pair["tgt_nrm"])
    c.set_source(pair["src_pts"], pair["src_nrm"])
    if nonlinear:
        c.set_optimizer()
    return c


def time_runs(c, reps):
    c.run(np.eye(4, dtype=np.float32), check=False)          # warm-up (index build, allocations)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); c.run(np.eye(4, dtype=np.float32), check=False); out.append(time.perf_counter() - t0)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-nonlinear", action="store_true")
    a = ap.parse_args()
    pair = synth.eth_like_pair(0)
    res = dict(n_points=len(pair["src_pts"]), iterations_per_run=20, reps=a.reps)
    modes = (True,) if a.only_nonlinear else (False, True)
    for nl in modes:
        c = make(pair, nl)
        med, all_s = time_runs(c, a.reps)
        key = "nonlinear" if nl else "linear"
        res[key] = dict(median_s=med, runs_s=all_s, icp_iterations_per_s=20.0 / med)
        if nl:
            s = c.lm_summaries()
            res[key]["lm_iterations"] = [d["iterations"] for d in s]
            res[key]["terminations"] = [d["termination"] for d in s]
        c.close()
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
