"""The cloud integrate on the clock (icp_tsdf_integrate_cloud): ONE synthetic laser scan of 370 488 points (344 x 1077
beams, 1 cm range noise) in its sensor frame, fused from its true pose into a hashed volume at 5 cm and at 10 cm voxels (truncation 4
voxels, no return cut off):
  * touch, accumulate, fold: the device time of ONE launch of each between events (icp_debug_tsdf_cloud_time: after the call that
    allocates the blocks and fuses the scan once, so the timed touch claims nothing new and the fold meets weights of 1);
  * insert: beside them, the device time of ONE icp_voxel_map_insert of the same cloud into a hashed voxel map of 0.25 m
    (icp_debug_vmap_time: both kernels and the counters' clear) -- what the laser half pays per scan today;
  * depth frame: and the touch and the integrate of ONE 640 x 480 depth frame of the same room over the pool the scan has left
    (icp_debug_htsdf_time) -- what the RGB-D half pays per frame on a pool of that size.
Every figure is the median of --reps repeats after one warm-up, each repeat on a fresh volume.  Reads nothing but icp_amd.synth.
usage: python tools/time_tsdf_cloud.py [--reps 7] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding, synth, tum

N_TILT, N_BEAM = 344, 1077
MAP_VOXEL = 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    T = synth.scan_pose(0)
    pts, nrm, _ = synth.laser_scan(T, 0xE7A0, N_TILT, N_BEAM)
    pts, nrm = synth.apply_pose(np.linalg.inv(T), pts, nrm)
    pose = binding.pose_to_c(T.astype(np.float32))
    W, H, K = tum.TUM_WIDTH, tum.TUM_HEIGHT, tum.TUM_K
    Tc = synth.camera_pose(0)
    depth = np.ascontiguousarray(synth.depth_frame(Tc, K.astype(np.float64), W, H, 0x7A11, 0.05)[0][:, 2].reshape(H, W), np.float32)
    cam = binding.depth_camera(K, W, H)
    cpose = binding.pose_to_c(Tc.astype(np.float32))
    ctx = binding.Context(0)
    ctx.set_stage_timing(0)
    ctx.set_gicp_options(1e-3, 0)
    ctx.set_source(pts, nrm)
    row = dict(library=binding.LIB_PATH, n_points=int(len(pts)), reps=a.reps, map_voxel=MAP_VOXEL)
    samples = {}
    for rep in range(a.reps + 1):                  # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        cur = {}
        for voxel in (0.05, 0.10):
            tag = "%dcm_" % round(100 * voxel)
            ctx.tsdf_create_hashed(block_capacity=1 << 14, origin=(0.0, 0.0, 0.0), voxel_size=voxel, truncation=4 * voxel, max_depth=30.0)
            ms = (C.c_float * 3)()
            ctx._ck(lib.icp_debug_tsdf_cloud_time(ctx.h, 1, binding._ptr(pose), None, ms))
            cur[tag + "touch_ms"], cur[tag + "accumulate_ms"], cur[tag + "fold_ms"] = ms[0], ms[1], ms[2]
            cur[tag + "total_ms"] = ms[0] + ms[1] + ms[2]
            row[tag + "blocks_after_scan"] = ctx.tsdf_blocks()[0]["n_blocks"]
            t_ms, i_ms = C.c_float(0), C.c_float(0)
            ctx._ck(lib.icp_debug_htsdf_time(ctx.h, binding._ptr(depth), C.byref(cam), binding._ptr(cpose), C.byref(t_ms), C.byref(i_ms)))
            cur[tag + "depth_touch_ms"], cur[tag + "depth_integrate_ms"] = t_ms.value, i_ms.value
            info = ctx.tsdf_blocks()[0]
            row[tag + "blocks_after_frame"] = info["n_blocks"]; row[tag + "capacity"] = info["capacity"]
        ctx.voxel_map_create_hashed(MAP_VOXEL, 1 << 16)
        ins, rec = C.c_float(0), C.c_float(0)
        ctx._ck(lib.icp_debug_vmap_time(ctx.h, 1, binding._ptr(pose), C.byref(ins), C.byref(rec)))
        cur["voxel_map_insert_ms"] = ins.value
        if rep:
            for k, v in cur.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = statistics.median(xs); row[k + "_min"] = min(xs); row[k + "_max"] = max(xs)
    ctx.tsdf_create_hashed(block_capacity=1 << 14, origin=(0.0, 0.0, 0.0), voxel_size=0.05, truncation=0.2, max_depth=30.0)
    row["info_5cm"] = ctx.tsdf_integrate_cloud("source", pose=T.astype(np.float32))
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
