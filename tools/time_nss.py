"""Times normal-space sampling (params.selection = 2) against RANDOM_SAMPLING (unchanged code: the yardstick) on the 370 488-point
ETH-like pair (synth.eth_like_pair(0), max distance 10): point-to-plane, k-NN (LBVH), 50 iterations from the identity, stage timing off,
selection_proba in {0.02, 0.1, 0.5}.  Per proba and variant -- random, nss (a draw per iteration), nss_held (one draw, held), all_cut
(SELECT_ALL on a source cut down to the held draw's points):
  * loop_ms / it_per_s : the device time of the 50 iterations (icp_get_timing: events around the loop) and iterations per second from it;
  * prologue_ms        : wall time of icp_run (it ends in a stream synchronise) minus loop_ms = everything in front of the loop: for random
                         and nss the up-front draws of all 50 iterations and the one copy of their sizes; for nss_held the draw, the copy, the
                         Morton sort and the gather of the held level.  Every repetition uses a new seed, so no draw is served from a cache.
Variants alternate inside each repetition; reported: the median and (min, max) of --reps repetitions after one warm-up each.
usage: python tools/time_nss.py [--reps 7] [--probas 0.02,0.1,0.5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from time_gicp import context, load   # noqa: E402  (same inputs and contexts)
import numpy as np                    # noqa: E402

ITERS = 50


def timed_run(c, seed):
    c.params.selection_seed = seed
    c.push_params()
    eye = np.eye(4, dtype=np.float32)
    t0 = time.perf_counter()
    _, recs, _ = c.run(eye, check=False)
    wall = (time.perf_counter() - t0) * 1e3
    t = c.timing()
    return t["total_ms"], wall - t["total_ms"], recs[-1]["n_src"]


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--probas", default="0.02,0.1,0.5")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sp, sn, tp, tn, md, _ = load("eth")
    rows = []
    for proba in [float(x) for x in a.probas.split(",")]:
        ctxs = {}
        for label, selection, resample in (("random", 1, True), ("nss", 2, True), ("nss_held", 2, False)):
            c = context(1, md)
            c.params.n_iterations, c.params.selection, c.params.selection_proba = ITERS, selection, proba
            c.set_nss_options(5, resample)
            c.set_target(tp, tn); c.set_source(sp, sn)
            timed_run(c, 1000)                                # warm-up: index build, levels, allocations, code objects
            ctxs[label] = c
        L = ctxs["nss_held"].selection(0)
        cut = context(1, md)
        cut.params.n_iterations = ITERS
        cut.set_target(tp, tn); cut.set_source(sp[L], sn[L])
        timed_run(cut, 0)
        ctxs["all_cut"] = cut
        loop = {k: [] for k in ctxs}; pro = {k: [] for k in ctxs}; n_src = {}
        for r in range(a.reps):
            for label, c in ctxs.items():
                lm, pm, n = timed_run(c, r)
                loop[label].append(lm); pro[label].append(pm); n_src[label] = n
        row = dict(proba=proba, iterations=ITERS, n_source=int(len(sp)), reps=a.reps)
        for label in ctxs:
            row[label] = dict(n_src_last=n_src[label], loop_ms=summary(loop[label]), prologue_ms=summary(pro[label]),
                              it_per_s=1e3 * ITERS / statistics.median(loop[label]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        for c in ctxs.values():
            c.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
