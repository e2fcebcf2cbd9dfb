"""Free-space carving on the clock (icp_set_tsdf_carve_options), by the method of tools/time_tsdf_cloud.py: ONE
synthetic laser scan of 370 488 points (344 x 1077 beams, 1 cm range noise) at 5 cm voxels, truncation 4 voxels, max_depth 30 m (J = 600
all the way), fused from its true pose
  * into a HASHED volume that already holds the scan before it (so there are resident blocks in front of many bands), and
  * into a DENSE box around the room (128 x 168 x 60 voxels).
For each: the device time of ONE accumulate launch between events after the call that allocates and warms (icp_debug_tsdf_cloud_time with
carving off: the existing accumulate, the baseline of the session; icp_debug_tsdf_carve_time otherwise), for distance = inf with
min_range 0 and 0.5 m, and distance = 2.0 m, interleaved inside every repeat; every figure is the median [min, max] of --reps repeats
after one warm-up, each repeat on fresh volumes.  Also the host time of one carve-off icp_tsdf_integrate_cloud (a wall clock around the
call, which ends in its counter read), and a CRC of every carved volume.
The two levers of the carving launch (dev_tsdf_carve.hpp) are constants of the build, as section 6zf's pass count was: build the forms
with __graft_entry__.build_hip(variant=NAME, defines=["ICP_TSDF_CARVE_COMBINE=0|1", "ICP_TSDF_CARVE_SKIP=0|1"]) and run the tool once per
library with ICP_HIP_LIB=<library>, alternating them in one session; the CRCs of all builds must agree.  --baseline-only times the
carve-off part alone and also runs on a library without the feature (the parent commit's, for the comparison of the carve-off call).
usage: python tools/time_tsdf_carve.py [--reps 5] [--baseline-only] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding, synth

N_TILT, N_BEAM = 344, 1077
VOXEL = 0.05
OPTS = dict(voxel_size=VOXEL, truncation=4 * VOXEL, max_depth=30.0)
DENSE = dict(origin=(-3.2, -4.2, -0.2), dims=(128, 168, 60))
CONFIGS = {"inf_min0": (float("inf"), 0.0), "inf_min0.5": (float("inf"), 0.5), "2m": (2.0, 0.0)}


def scan(k):
    T = synth.scan_pose(k)
    pts, nrm, _ = synth.laser_scan(T, 0xE7A0 + k, N_TILT, N_BEAM)
    pts, nrm = synth.apply_pose(np.linalg.inv(T), pts, nrm)
    return (pts, nrm), T.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    prev, Tp = scan(0)
    cur, Tc = scan(1)
    pose = binding.pose_to_c(Tc)
    ctx = binding.Context(0)
    ctx.set_stage_timing(0)
    ctx.set_gicp_options(1e-3, 0)
    row = dict(library=binding.LIB_PATH, n_points=int(len(cur[0])), reps=a.reps)
    samples = {}

    def volume(storage):
        if not a.baseline_only:
            ctx.set_tsdf_carve(0.0)                    # (the scan before is fused without carving, whatever is timed behind it)
        if storage == "hashed":
            ctx.tsdf_create_hashed(block_capacity=1 << 14, origin=(0.0, 0.0, 0.0), **OPTS)
            ctx.set_source(*prev)
            ctx.tsdf_integrate_cloud("source", pose=Tp)
        else:
            ctx.tsdf_create(**DENSE, **OPTS)
        ctx.set_source(*cur)

    def state(storage):
        return ctx.tsdf_blocks()[1:] if storage == "hashed" else ctx.tsdf_volume()

    for rep in range(a.reps + 1):                      # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        now = {}
        for storage in ("hashed", "dense"):
            volume(storage)
            ms = (C.c_float * 3)()
            ctx._ck(lib.icp_debug_tsdf_cloud_time(ctx.h, 1, binding._ptr(pose), None, ms))
            now[storage + "/existing_accumulate_ms"] = ms[1]; now[storage + "/fold_ms"] = ms[2]; now[storage + "/touch_ms"] = ms[0]
            walls = []
            for _ in range(5):
                t0 = time.perf_counter()
                info = ctx.tsdf_integrate_cloud("source", pose=Tc)
                walls.append(1e3 * (time.perf_counter() - t0))
            now[storage + "/carve_off_call_wall_ms"] = statistics.median(walls)
            row[storage + "/info_off"] = info
            if a.baseline_only:
                continue
            for name, (dist, mr) in CONFIGS.items():
                volume(storage)
                ctx.set_tsdf_carve(dist, mr)
                ctx._ck(lib.icp_debug_tsdf_carve_time(ctx.h, 1, binding._ptr(pose), None, ms))
                now["%s/%s/carve_accumulate_ms" % (storage, name)] = ms[1]
                if rep == 0:
                    st = ctx.tsdf_carve_stats()
                    row["%s/%s/n_carved" % (storage, name)] = st["n_carved"]; row["%s/%s/n_steps" % (storage, name)] = st["n_steps"]
                    crc = 0
                    for x in state(storage):
                        crc = zlib.crc32(np.ascontiguousarray(x).tobytes(), crc)
                    row["%s/%s/volume_crc" % (storage, name)] = crc
        if rep:
            for k, v in now.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = [statistics.median(xs), min(xs), max(xs)]
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
