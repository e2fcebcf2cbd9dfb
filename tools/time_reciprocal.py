"""What reciprocal (mutual nearest-neighbour) rejection (icp_set_reciprocal_options) costs, on the bench pair synth.eth_like_pair(0):
point-to-plane, 50 iterations, k-NN (LBVH), max distance 10, from the identity, stage timing 0.  Times are the run's device time
(icp_get_timing total_ms: events around the whole run).  Three contexts on the same pair, all in the separate loop form (ICP_HIP_MERGE=0 for
the process: the option itself never takes the merged form), warmed up once and then run `--reps` times, interleaved:
  separate_off   the option off
  separate_on    the option on: k_reciprocal, the bounded existence walk over the source tree
  naive          the option on through icp_debug_reciprocal_naive: the target points written out in the source's frame, a full k_knn_bvh
                 search of them against the source tree, a compare pass (same records and counts; checked here)
Reported: the median, minimum and maximum of each, the cost per iteration of the two routes over separate_off and the kept fraction per
iteration.  (The default, merged figure with the option off is bench.py's.)
usage: python tools/time_reciprocal.py [--reps 5] [--iterations 50] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.environ["ICP_HIP_MERGE"] = "0"                       # read when a context is created
    from icp_amd import binding, synth
    d = synth.eth_like_pair(0)
    eye = binding.pose_to_c(np.eye(4))
    lib = binding.load_library()

    def context(on, naive):
        c = binding.Context(0)
        c.params.metric = 1; c.params.knn_backend = 1; c.params.max_distance = 10.0; c.params.n_iterations = a.iterations
        c.push_params(); c.set_stage_timing(0)
        c.set_target(d["tgt_pts"], d["tgt_nrm"]); c.set_source(d["src_pts"], d["src_nrm"])
        c.set_reciprocal_options(on)
        if naive and lib.icp_debug_reciprocal_naive(c.h, C.c_int32(1)) != 0:
            raise RuntimeError("icp_debug_reciprocal_naive failed")
        return c
    ctxs = {"separate_off": context(False, False), "separate_on": context(True, False), "naive": context(True, True)}
    times = {k: [] for k in ctxs}
    poses = {}
    for rep in range(a.reps + 1):                            # rep 0: warm-up (index builds, allocations, code load)
        for k, c in ctxs.items():
            p = eye.copy()
            c.run_raw(p)
            poses[k] = p
            if rep:
                times[k].append(c.timing()["total_ms"])
    st_on, st_naive = ctxs["separate_on"].reciprocal_stats(), ctxs["naive"].reciprocal_stats()
    same = st_on == st_naive and np.array_equal(poses["separate_on"].view(np.uint32), poses["naive"].view(np.uint32))
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = dict(iterations=a.iterations, reps=a.reps,
               median_ms=med, min_ms={k: float(min(v)) for k, v in times.items()}, max_ms={k: float(max(v)) for k, v in times.items()},
               bounded_walk_us_per_iteration=1e3 * (med["separate_on"] - med["separate_off"]) / a.iterations,
               naive_us_per_iteration=1e3 * (med["naive"] - med["separate_off"]) / a.iterations,
               naive_equals_bounded_walk=bool(same),
               kept_fraction=[round(s["n_mutual"] / max(s["n_matched"], 1), 4) for s in st_on],
               n_matched=[s["n_matched"] for s in st_on])
    for c in ctxs.values():
        c.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
