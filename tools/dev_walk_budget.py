"""Dev tool (a build with ICP_DEBUG_STEPS=1 ICP_DEBUG_TIMES=1: ICP_HIP_LIB=.../libicp_hip_times.so): the budget of the shared walk -- how many times a
WAVE executes each step of knn_walk_shared in one launch of the fused matcher (WALK_BUDGET in dev_bvh.hpp: a step counts once however many lanes
take part, which is what the wave pays for).  Next to the counts: the launch length and the time the waves spend in the walk, from the same
launch's time stamps.  usage: ICP_HIP_LIB=... python tools/dev_walk_budget.py [--csv FILE] [launch ...]   (default launches: 0 1 2 5 8 12 20)"""
import sys, os, ctypes as C
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))
import numpy as np
from icp_amd import binding, synth
args = sys.argv[1:]
csv = None
if args and args[0] == "--csv": csv = args[1]; args = args[2:]
launches = [int(a) for a in args] or [0, 1, 2, 5, 8, 12, 20]
p = synth.eth_like_pair(0)
n = len(p["src_pts"])
c = binding.Context(0)
c.params.max_distance = 10.0; c.params.metric = 1; c.params.knn_backend = 1
c.set_stage_timing(0)
c.push_params(); c.set_target(p["tgt_pts"], p["tgt_nrm"]); c.set_source(p["src_pts"], p["src_nrm"])
nw = ((n + 255) // 256) * 4
assert 16 * nw + 8 * 4096 <= n, "the debug buffer has no room for the budget rows at this size"
names = ["node steps", "leaf evaluations", "leaf winner updates", "leaf sequential scans", "hand-over rounds", "folds", "board posts + claims", "outer passes"]
rows = ["launch,waves,waves_with_walkers,walking_queries,launch_us,walk_us_mean_walking_wave,walk_us_max," + ",".join("%s_sum,%s_mean_walking_wave,%s_p99,%s_max" % ((s.replace(" ", "_").replace("+", "and"),) * 4) for s in names)]
for L in launches:
    c.params.n_iterations = L + 1; c.push_params()
    c.run(np.eye(4))
    buf = np.zeros(n, np.int32)
    assert c.lib.icp_debug_steps(c.h, buf.ctypes.data_as(C.c_void_p), C.c_int32(n)) == 0
    w = buf[: nw * 8].reshape(nw, 8)
    t = w[:, :6].astype(np.uint32).astype(np.int64)
    rel = (t - t[:, 0].min()) * 0.01                       # us since the first wave started
    walkers = w[:, 6] & 0xFF
    b = buf[nw * 8 + 8 * 4096: nw * 16 + 8 * 4096].reshape(nw, 8).astype(np.int64)
    ww = walkers > 0
    walk_us = rel[:, 2] - rel[:, 1]
    print("launch %d: %d waves, %d with walkers (%d walking queries); launch %.2f us, walk per walking wave mean %.2f max %.2f us"
          % (L, nw, ww.sum(), walkers.sum(), rel[:, 5].max(), walk_us[ww].mean() if ww.any() else 0.0, walk_us.max()))
    line = [L, nw, int(ww.sum()), int(walkers.sum()), "%.2f" % rel[:, 5].max(), "%.2f" % (walk_us[ww].mean() if ww.any() else 0.0), "%.2f" % walk_us.max()]
    for j, s in enumerate(names):
        col = b[:, j]; act = col[ww] if ww.any() else col
        print("   %-22s sum %9d   per walking wave: mean %7.2f  p99 %5d  max %5d   (waves without walkers that helped: %d executions)"
              % (s, col.sum(), act.mean(), np.percentile(act, 99), col.max(), col[~ww].sum()))
        line += [int(col.sum()), "%.2f" % act.mean(), int(np.percentile(act, 99)), int(col.max())]
    rows.append(",".join(str(x) for x in line))
if csv:
    os.makedirs(os.path.dirname(os.path.abspath(csv)), exist_ok=True)
    open(csv, "w").write("\n".join(rows) + "\n")
