"""A laser scan aligned to the TSDF volume on the clock (icp_tsdf_align_cloud, icp_track_scans_sdf): synthetic scans of
370 488 points (344 x 1077 beams, 1 cm range noise) in their sensor frames, 5 cm voxels, truncation 0.4 m (8 voxels: synth.scan_pose moves
0.40 m per scan, and the band is the basin of convergence).
  * pair: the device time of ONE accumulate + k_sdf_solve pair between events (icp_debug_sdf_cloud_time) of scan 1 at its true pose against
    the model scan 0 has left, on a dense box around the room (k_sdf_accumulate_cloud) and on a hashed volume (k_hsdf_accumulate_cloud);
    beside it, in the same repeat, the k_vgicp_accumulate + k_sdf_solve pair of tools/time_vgicp.py (icp_debug_vgicp_time: the ETH-like pair
    of the same size against a 0.25 m grid, the cloud's own normals);
  * tracked scan: the host's wall time of icp_track_scans_sdf over --scans scans minus that over scan 0 alone, per tracked scan (upload,
    alignment, record read and fuse of one scan against one model); beside it the same difference of icp_track_scans_vmap on a hashed
    voxel map of 0.25 m plus the upload and icp_tsdf_integrate_cloud of one scan, which eth.reconstruct's default tracker pays later.
Every figure is the median of --reps repeats after one warm-up, the candidates interleaved inside each repeat, with the least and the
largest sample beside it.  Reads nothing but icp_amd.synth.
usage: python tools/time_sdf_cloud.py [--reps 7] [--scans 3] [--json out.json]"""
import argparse
import ctypes as C
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

N_TILT, N_BEAM = 344, 1077
VOXEL, MAP_VOXEL = 0.05, 0.25
TSDF = dict(voxel_size=VOXEL, truncation=0.4, max_depth=30.0)
DENSE = dict(dims=(140, 180, 72), origin=(-3.5, -4.5, -0.5))       # synth's room, half a metre of margin


def create(ctx, hashed):
    if hashed:
        ctx.tsdf_create_hashed(block_capacity=1 << 14, origin=(0.0, 0.0, 0.0), **TSDF)
    else:
        ctx.tsdf_create(**DENSE, **TSDF)


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scans", type=int, default=3)
    ap.add_argument("--n-tilt", type=int, default=N_TILT)
    ap.add_argument("--n-beam", type=int, default=N_BEAM)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    scans, poses = [], []
    for k in range(a.scans):
        T = synth.scan_pose(k)
        pts, nrm, _ = synth.laser_scan(T, 0xE7A0 + k, a.n_tilt, a.n_beam)
        pts, nrm = synth.apply_pose(np.linalg.inv(T), pts, nrm)
        scans.append((np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(nrm, np.float32))); poses.append(T.astype(np.float32))
    d = synth.eth_like_pair(0, a.n_tilt, a.n_beam)
    ctx = binding.Context(0)
    ctx.set_stage_timing(0)
    ctx.set_gicp_options(1e-3, 0)
    vg = binding.Context(0)
    vg.set_stage_timing(0)
    vg.set_gicp_options(1e-3, 0)
    vg.set_target(d["tgt_pts"], d["tgt_nrm"]); vg.set_source(d["src_pts"], d["src_nrm"])
    vo = binding.vgicp_options(voxel_size=MAP_VOXEL, stop_rotation=0.0, stop_translation=0.0)
    so = binding.sdf_options(n_iterations=30)
    mo = dict(voxel_size=MAP_VOXEL, n_iterations=30)
    eye = binding.pose_to_c(np.eye(4, dtype=np.float32))
    row = dict(library=binding.LIB_PATH, n_points=int(len(scans[0][0])), n_scans=a.scans, reps=a.reps, voxel=VOXEL, map_voxel=MAP_VOXEL)
    samples = {}
    for rep in range(a.reps + 1):                  # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        cur = {}
        for hashed in (False, True):
            tag = "hashed_" if hashed else "dense_"
            create(ctx, hashed)
            ctx.set_source(scans[0][0])
            ctx.tsdf_integrate_cloud("source", pose=poses[0])
            ctx.set_source(scans[1][0])
            ms = C.c_float(0)
            ctx._ck(lib.icp_debug_sdf_cloud_time(ctx.h, 1, binding._ptr(binding.pose_to_c(poses[1])), C.byref(so), C.byref(ms)))
            cur[tag + "pair_ms"] = ms.value
            it, build, index = C.c_float(0), C.c_float(0), C.c_float(0)
            vg._ck(lib.icp_debug_vgicp_time(vg.h, binding._ptr(eye), C.byref(vo), C.byref(it), C.byref(build), C.byref(index)))
            cur[tag + "beside_vgicp_pair_ms"] = it.value
            if not rep:
                sums, counts = ctx.tsdf_cloud_system("source", poses[1])
                row[tag + "pair_counts"] = [int(counts[0]), int(counts[1])]
            # the loops: all scans, and scan 0 alone
            create(ctx, hashed)
            t_all, out = wall(lambda: ctx.track_scans_sdf([s[0] for s in scans], poses[0], n_iterations=30))
            create(ctx, hashed)
            t_one, _ = wall(lambda: ctx.track_scans_sdf([scans[0][0]], poses[0], n_iterations=30))
            cur[tag + "tracked_scan_ms"] = (t_all - t_one) / (a.scans - 1)
            if not rep:
                row[tag + "track"] = dict(status=out[3], iterations=[r["iterations"] for r in out[1]], n_valid_first=[r["n_valid_first"] for r in out[1]])
        ctx.voxel_map_create_hashed(MAP_VOXEL, 1 << 16)
        t_all, out = wall(lambda: ctx.track_scans_vmap(scans, poses[0], **mo))
        ctx.voxel_map_create_hashed(MAP_VOXEL, 1 << 16)
        t_one, _ = wall(lambda: ctx.track_scans_vmap(scans[:1], poses[0], **mo))
        cur["vmap_tracked_scan_ms"] = (t_all - t_one) / (a.scans - 1)
        create(ctx, True)
        ctx.set_source(scans[0][0]); ctx.tsdf_integrate_cloud("source", pose=poses[0])

        def later_fuse():
            ctx.set_source(scans[1][0])
            return ctx.tsdf_integrate_cloud("source", pose=poses[1])
        cur["later_fuse_ms"], _ = wall(later_fuse)
        cur["vmap_tracked_scan_plus_fuse_ms"] = cur["vmap_tracked_scan_ms"] + cur["later_fuse_ms"]
        if not rep:
            row["vmap_track"] = dict(status=out[2], iterations=[r["iterations"] for r in out[1]])
        else:
            for k, v in cur.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = statistics.median(xs); row[k + "_min"] = min(xs); row[k + "_max"] = max(xs)
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    ctx.close(); vg.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
