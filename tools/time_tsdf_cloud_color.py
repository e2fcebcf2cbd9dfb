"""The coloured cloud fuse on the clock (icp_tsdf_integrate_cloud_color), by the method of tools/time_tsdf_cloud.py
and tools/time_tsdf_carve.py: ONE synthetic laser scan of 370 488 coloured points (344 x 1077 beams, 1 cm range noise) at 5 cm voxels,
truncation 4 voxels, max_depth 30 m, fused from its true pose
  * into a coloured HASHED volume, and
  * into a coloured DENSE box around the room (128 x 168 x 60 voxels).
For each: the device time of ONE touch, ONE accumulate, ONE fold, ONE colour accumulate and ONE colour fold launch between events after
the call that allocates, fuses once and warms (icp_debug_tsdf_cloud_color_time), so the geometric fuse (touch + accumulate + fold) and
the coloured fuse (the same plus the two colour launches) are taken in the same session from the same launches; every figure is the
median [min, max] of --reps repeats after one warm-up, each repeat on fresh volumes.  Also the host time of one
icp_tsdf_integrate_cloud and one icp_tsdf_integrate_cloud_color (a wall clock around the call, which ends in its counter read), and a CRC
of every coloured volume.
The two levers of the colour accumulate (dev_tsdf_cloud_color.hpp) are constants of the build: build the forms with
__graft_entry__.build_hip(variant=NAME, defines=["ICP_TSDF_COLOR_PACK=0|1", "ICP_TSDF_COLOR_COMBINE=0|1"]) and run the tool once per
library with ICP_HIP_LIB=<library>, alternating them in one session; the CRCs of all builds must agree.
usage: python tools/time_tsdf_cloud_color.py [--reps 5] [--json out.json]"""
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
STAGES = ("touch", "accumulate", "fold", "color_accumulate", "color_fold")


def crc(arrays):
    v = 0
    for a in arrays:
        v = zlib.crc32(np.ascontiguousarray(a).tobytes(), v)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    T = synth.scan_pose(1)
    pts, _, rgba = synth.laser_scan(T, 0xE7A0 + 1, N_TILT, N_BEAM)
    pts, _ = synth.apply_pose(np.linalg.inv(T), pts, np.zeros_like(pts))
    T = T.astype(np.float32)
    pose = binding.pose_to_c(T)
    ctx = binding.Context(0)
    ctx.set_stage_timing(0)
    ctx.set_source(pts, None, rgba)
    row = dict(library=binding.LIB_PATH, n_points=int(len(pts)), reps=a.reps)
    samples = {}

    def create(kind):
        if kind == "hashed":
            ctx.tsdf_create_hashed(block_capacity=1 << 14, origin=(0.0, 0.0, 0.0), color=True, **OPTS)
        else:
            ctx.tsdf_create(color=True, **DENSE, **OPTS)

    for rep in range(a.reps + 1):                  # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        cur = {}
        for kind in ("hashed", "dense"):
            create(kind)
            ms = (C.c_float * 5)()
            ctx._ck(lib.icp_debug_tsdf_cloud_color_time(ctx.h, 1, binding._ptr(pose), None, ms))
            for k, name in enumerate(STAGES):
                cur["%s_%s_ms" % (kind, name)] = ms[k]
            cur[kind + "_geometric_fuse_ms"] = ms[0] + ms[1] + ms[2]
            cur[kind + "_colored_fuse_ms"] = sum(ms)
            state = ctx.tsdf_blocks(colors=True)[1:] if kind == "hashed" else ctx.tsdf_volume() + ctx.tsdf_color_volume()
            row[kind + "_crc"] = crc(state)
            create(kind)
            t0 = time.perf_counter(); plain = ctx.tsdf_integrate_cloud("source", pose=T); t1 = time.perf_counter()
            cur[kind + "_host_geometric_call_ms"] = 1e3 * (t1 - t0)
            create(kind)
            t0 = time.perf_counter(); info = ctx.tsdf_integrate_cloud("source", pose=T, color=True); t1 = time.perf_counter()
            cur[kind + "_host_colored_call_ms"] = 1e3 * (t1 - t0)
            row[kind + "_info"] = info
            assert {k: v for k, v in info.items() if k != "n_colored"} == plain
        if rep:
            for k, v in cur.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = statistics.median(xs); row[k + "_min"] = min(xs); row[k + "_max"] = max(xs)
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
