"""The hashed TSDF volume on the clock, against the dense volume of tools/time_tsdf.py on the same 640 x 480 synthetic
sequence and the same grid (the 8.96 m cube at 256^3: voxel 35 mm, truncation 5 voxels), from a volume holding 4 frames:
  kernels : device time of ONE k_sdf_accumulate + k_sdf_solve pair (icp_debug_sdf_time; the solve is the same kernel on both storages, so
            the difference is the accumulate launch's) on the dense and on the hashed volume; of one dense integrate (icp_debug_tsdf_time)
            against one touch plus one integrate over the pool (icp_debug_htsdf_time)
  tracking: frames/s of icp_track_depth_sdf at stride 1 with 20 iterations on either storage -- `*_all` with the stops off -- the hashed
            loop with its second host wait per frame; the hashed volume starts at the default capacity and grows on the way
  memory  : bytes held (blocks x 4 KiB + 12 bytes per table slot + 8 per pool block) after the sequence at 35 mm, 5 cm and 1 cm voxels
            (truncation 5 voxels), against the dense box over the same cube (8 bytes per voxel; computed, not allocated)
  lookups : the share of the frame's sampled cells that lie inside one block (one table lookup), across a face, an edge, a corner
Repeats are interleaved (every configuration once per round) and the median is reported.  Stage timing is off.
usage: python tools/time_htsdf.py [--reps 9] [--frames 12] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))
import numpy as np
from icp_amd import binding, synth, tum

EXTENT, ORIGIN = 8.96, (-4.2, -4.5, -1.5)          # tools/time_tsdf.py's cube, camera-0 coordinates


def volume_options(n):
    s = EXTENT / n
    return dict(dims=(n, n, n), origin=tuple(o + s / 2 for o in ORIGIN), voxel_size=s, truncation=5 * s)


def hashed_options(voxel):
    return dict(origin=tuple(o + voxel / 2 for o in ORIGIN), voxel_size=voxel, truncation=5 * voxel)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def held_bytes(info):
    return info["n_blocks"] * 4096, info["capacity"] * (4096 + 8 + 2 * 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = tum.TUM_K
    T = [synth.camera_pose(k) for k in range(a.frames)]
    made = [synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05) for k, Tk in enumerate(T)]
    depth = np.stack([m[0][:, 2].reshape(H, W).copy() for m in made])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames)
    dense_opt = volume_options(256)
    hash_opt = {k: v for k, v in dense_opt.items() if k != "dims"}

    # kernels: both volumes hold frames 0 .. 3 at their true poses; frame 2 is timed
    d, h = binding.Context(0), binding.Context(0)
    d.tsdf_create(**dense_opt); h.tsdf_create_hashed(block_capacity=1 << 15, **hash_opt)
    for k in range(4):
        nd = d.tsdf_integrate(depth[k], cam, gt[k]); nh = h.tsdf_integrate(depth[k], cam, gt[k])
    info = h.tsdf_blocks()[0]
    d2 = np.ascontiguousarray(depth[2], np.float32); p2 = binding.pose_to_c(gt[2])
    one = binding.sdf_options(stride=1, n_iterations=20, stop_rotation=0.0, stop_translation=0.0)
    kern = dict(dense_pair_ms=[], hashed_pair_ms=[], dense_integrate_ms=[], hashed_touch_ms=[], hashed_integrate_ms=[])
    for rep in range(a.reps + 1):                       # the first round warms up
        ms = C.c_float(0)
        d._ck(lib.icp_debug_sdf_time(d.h, binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(one), C.byref(ms))); dp = ms.value
        h._ck(lib.icp_debug_sdf_time(h.h, binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(one), C.byref(ms))); hp = ms.value
        d._ck(lib.icp_debug_tsdf_time(d.h, C.c_int32(0), binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(ms))); di = ms.value
        t_ms, i_ms = C.c_float(0), C.c_float(0)
        h._ck(lib.icp_debug_htsdf_time(h.h, binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(t_ms), C.byref(i_ms)))
        if rep:
            for key, v in (("dense_pair_ms", dp), ("hashed_pair_ms", hp), ("dense_integrate_ms", di), ("hashed_touch_ms", t_ms.value), ("hashed_integrate_ms", i_ms.value)):
                kern[key].append(v)
    out["kernels"] = {k + "_median": median(v) for k, v in kern.items()}
    out["kernels"].update(updated_voxels_dense=nd, updated_voxels_hashed=nh, n_blocks=info["n_blocks"])
    out["kernels"]["pair_hashed_over_dense"] = out["kernels"]["hashed_pair_ms_median"] / out["kernels"]["dense_pair_ms_median"]
    out["kernels"]["touch_plus_integrate_over_dense"] = (out["kernels"]["hashed_touch_ms_median"] + out["kernels"]["hashed_integrate_ms_median"]) / out["kernels"]["dense_integrate_ms_median"]
    d.close(); h.close()

    # lookups: the cells of frame 2's pixels at its pose
    P = gt[2]
    z = depth[2].reshape(-1); ok = np.isfinite(z) & (z > 0)
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))
    x = (uu.reshape(-1)[ok] - K[0, 2]) / K[0, 0] * z[ok]; y = (vv.reshape(-1)[ok] - K[1, 2]) / K[1, 1] * z[ok]
    q = np.stack([x, y, z[ok]], 1) @ P[:3, :3].T.astype(np.float64) + P[:3, 3]
    cell = np.floor((q - np.array(hash_opt["origin"])) / hash_opt["voxel_size"]).astype(np.int64)
    crossing = ((cell & 7) == 7).sum(1)
    out["lookups"] = {"%d_blocks" % (1 << k): float((crossing == k).mean()) for k in range(4)}

    # tracking
    ctx = binding.Context(0)
    ctx.set_stage_timing(0)
    sdf_opt = dict(sdf=binding.sdf_options(stride=1, n_iterations=20), sdf_all=binding.sdf_options(stride=1, n_iterations=20, stop_rotation=0.0, stop_translation=0.0))
    times = dict(dense_sdf=[], hashed_sdf=[], dense_sdf_all=[], hashed_sdf_all=[])
    err = {}
    for rep in range(a.reps + 1):
        for route in times:
            storage, opt = route.split("_", 1)
            t0 = time.perf_counter()
            if storage == "dense":
                ctx.tsdf_create(**dense_opt)
            else:
                ctx.tsdf_create_hashed(**hash_opt)
            pose, recs, rc = ctx.track_depth_sdf(depth, cam, options=sdf_opt[opt])
            dt = time.perf_counter() - t0
            if rep:
                times[route].append(dt)
            err[route] = dict(status=rc, iterations=[r["iterations"] for r in recs],
                              final_translation_error_m=float(np.linalg.norm(pose[:3, 3].astype(np.float64) - gt[-1][:3, 3])))
            if storage == "hashed":
                err[route].update(ctx.tsdf_blocks()[0])
    n = a.frames - 1
    out["tracking"] = {k: dict(median_s=median(v), frames_per_s_median=n / median(v), ms_per_frame_median=1e3 * median(v) / n, **err[k]) for k, v in times.items()}
    out["tracking"]["hashed_over_dense_time_all"] = out["tracking"]["hashed_sdf_all"]["median_s"] / out["tracking"]["dense_sdf_all"]["median_s"]

    # memory: the sequence fused at its true poses
    out["memory"] = {}
    for voxel in (EXTENT / 256, 0.05, 0.01):
        ctx.tsdf_create_hashed(**hashed_options(voxel))
        for k in range(a.frames):
            ctx.tsdf_integrate(depth[k], cam, gt[k])
        info = ctx.tsdf_blocks()[0]
        used, held = held_bytes(info)
        n_side = int(round(EXTENT / voxel))
        out["memory"]["%.4g" % voxel] = dict(n_blocks=info["n_blocks"], capacity=info["capacity"], n_grown=info["n_grown"], block_bytes=used, held_bytes=held,
                                            dense_side=n_side, dense_bytes=8 * n_side ** 3, dense_over_blocks=8 * n_side ** 3 / max(used, 1))
    ctx.tsdf_release()
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
