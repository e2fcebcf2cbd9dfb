"""The library's own cost of the stage-timing modes (icp_set_stage_timing 0 / 1 / 17) on the bench pair: icp_run alone in the timed loop, without
bench.py's per-step bookkeeping (ctx.iteration_times + numpy in its timed region whenever --stage-timing > 0).  Six rounds, the modes alternating;
per mode the host time per run over 200 runs and the device-clock total of a run.  usage: python tools/time_stage_timing.py [OUT.json]
(profiles/run_overheads/mode_cost.json)."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))
from icp_amd import binding, synth
pair = synth.eth_like_pair(0)
opt = binding.LinearICPOptimizer(0)
opt.setMatchingMethod(0); opt.setMatchingMaxDistance(10.0); opt.setMetric(1); opt.setNbOfIterations(50)
opt.setWeightingMethod(0); opt.setRejectionMethod(1); opt.setKnnBackend(1)
ctx = opt.ctx; ctx.params.knn_incremental = 1; ctx.push_params()
ctx.set_target(pair["tgt_pts"], pair["tgt_nrm"], None); ctx.set_source(pair["src_pts"], pair["src_nrm"], None)
eye = binding.pose_to_c(np.eye(4, dtype=np.float32))
out = []
for rnd in range(6):
    for mode in (0, 1, 17):
        ctx.set_stage_timing(mode)
        for _ in range(20):
            p = eye.copy(); ctx.run_raw(p)
        dev = 0.0
        t = time.perf_counter()
        for _ in range(200):
            p = eye.copy(); ctx.run_raw(p)
        host_ms = (time.perf_counter() - t) * 1e3 / 200
        for _ in range(20):                                     # device-clock total of a run, read outside the timed loop
            p = eye.copy(); ctx.run_raw(p); dev += ctx.timing()["total_ms"]
        out.append(dict(round=rnd, mode=mode, host_ms_per_run=host_ms, device_total_ms=dev / 20))
        print(out[-1], flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
