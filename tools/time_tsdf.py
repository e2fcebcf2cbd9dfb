"""Frame-to-model tracking on the clock, on the synthetic room at 640 x 480:
  kernels : device time of one icp_tsdf_integrate and of one icp_tsdf_raycast launch (events around the launch, icp_debug_tsdf_time) for a
            256^3 and a 512^3 volume over the same 8.96 m cube (voxel 35 mm / 17.5 mm, truncation 5 voxels), from a volume holding 4 frames
  tracking: frames/s of icp_track_depth_model (256^3) against icp_track_depth_frames on the 12-frame sequence of
            tools/time_depth_tracking.py, same params (point-to-plane k-NN on the LBVH, 35 iterations, max distance 0.1, source (false, 8)),
            and of icp_track_depth_sdf on the same sequence and volume at stride 1 with 20 iterations: `sdf` with the
            default stops, `sdf_all` with the stops off (every frame runs its 20 iterations); sdf_pair_ms is the device time of ONE
            k_sdf_accumulate + k_sdf_solve pair (icp_debug_sdf_time)
  colour  : on the same sequence with its colour frames and the 256^3 volume with its colour array:
            icp_track_depth_model_color (the colored metric, otherwise `model`'s params) against icp_track_depth_sdf_color at stride 1, weight
            0.1 -- `sdf_color` with the default stops, `sdf_color_all` with the stops off -- and, for the cost of the photometric row alone,
            icp_track_depth_sdf painting the same volume (`sdf_paint_all`, stops off); sdf_color_pair_ms is ONE k_sdf_accumulate_color +
            k_sdf_solve_color pair (icp_debug_sdf_color_time)
Repeats are interleaved (every configuration once per round) and the median is reported.  Stage timing is off.
usage: python tools/time_tsdf.py [--reps 9] [--frames 12] [--skip-512] [--json out.json]"""
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

EXTENT, ORIGIN = 8.96, (-4.2, -4.5, -1.5)          # camera-0 coordinates: the room spans x -2.7 .. 3.3, y -1.3 .. 1.3, z -1.2 .. 6.8


def volume_options(n):
    s = EXTENT / n
    return dict(dims=(n, n, n), origin=tuple(o + s / 2 for o in ORIGIN), voxel_size=s, truncation=5 * s)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--skip-512", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = tum.TUM_K
    T = [synth.camera_pose(k) for k in range(a.frames)]
    made = [synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05) for k, Tk in enumerate(T)]
    depth = np.stack([m[0][:, 2].reshape(H, W).copy() for m in made])
    rgbx = np.stack([np.ascontiguousarray(m[2], np.uint8) for m in made])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames, kernels={})

    # kernels
    sizes = [256] if a.skip_512 else [256, 512]
    ctxs = {}
    for n in sizes:
        c = binding.Context(0)
        c.tsdf_create(**volume_options(n))
        updated = [c.tsdf_integrate(depth[k], cam, gt[k]) for k in range(4)]
        _, _, _, hits = c.tsdf_raycast(cam, gt[1])
        ctxs[n] = c
        out["kernels"][str(n)] = dict(voxel_size=EXTENT / n, updated_voxels=updated[-1], hits=hits, integrate_ms=[], raycast_ms=[])
    d2 = np.ascontiguousarray(depth[2], np.float32); p2 = binding.pose_to_c(gt[2])
    for rep in range(a.reps + 1):                       # the first round warms up
        for n in sizes:
            for which, key in ((0, "integrate_ms"), (1, "raycast_ms")):
                ms = C.c_float(0)
                ctxs[n]._ck(lib.icp_debug_tsdf_time(ctxs[n].h, C.c_int32(which), binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(ms)))
                if rep:
                    out["kernels"][str(n)][key].append(ms.value)
    for n in sizes:
        r = out["kernels"][str(n)]
        r["integrate_ms_median"] = median(r["integrate_ms"]); r["raycast_ms_median"] = median(r["raycast_ms"])
        r["integrate_gb_per_s"] = r["updated_voxels"] * 16 / (r["integrate_ms_median"] * 1e-3) / 1e9      # 16 bytes per updated voxel
        ctxs[n].close()

    # tracking
    ctx = binding.Context(0)
    ctx.params.metric = 1; ctx.params.knn_backend = 1
    tum.reconstruct_room_params(ctx.params)
    ctx.push_params(); ctx.set_stage_timing(0)
    to, so = tum.reconstruct_room_options(ctx.params)
    times = dict(model=[], frame0=[], sdf=[], sdf_all=[], model_color=[], sdf_color=[], sdf_color_all=[], sdf_paint_all=[])
    so_color = binding.depth_options(bool(so.keep_original_size), int(so.downsample_factor), float(so.max_distance), fix_color_index=True)
    c2 = np.ascontiguousarray(rgbx[2], np.uint8); co = binding.sdf_color_options(weight=0.1)
    err = {}
    sdf_opt = dict(sdf=binding.sdf_options(stride=1, n_iterations=20), sdf_all=binding.sdf_options(stride=1, n_iterations=20, stop_rotation=0.0, stop_translation=0.0))
    pair_ms, color_pair_ms = [], []
    for rep in range(a.reps + 1):
        for route in ("model", "frame0", "sdf", "sdf_all", "model_color", "sdf_color", "sdf_paint_all", "sdf_color_all"):
            ctx.params.metric = 4 if route == "model_color" else 1
            ctx.push_params()
            t0 = time.perf_counter()
            if route == "model":
                ctx.tsdf_create(**volume_options(256))
                pose, recs, rc = ctx.track_depth_model(depth, cam, so)
            elif route == "model_color":
                ctx.tsdf_create(color=True, **volume_options(256))
                pose, recs, rc = ctx.track_depth_model(depth, cam, so_color, rgbx_frames=rgbx)
            elif route in ("sdf_color", "sdf_color_all"):
                ctx.tsdf_create(color=True, **volume_options(256))
                pose, recs, rc = ctx.track_depth_sdf(depth, cam, rgbx_frames=rgbx, options=sdf_opt[route.replace("_color", "")], color_weight=0.1)
            elif route == "sdf_paint_all":
                ctx.tsdf_create(color=True, **volume_options(256))
                pose, recs, rc = ctx.track_depth_sdf(depth, cam, rgbx_frames=rgbx, options=sdf_opt["sdf_all"])
            elif route in sdf_opt:
                ctx.tsdf_create(**volume_options(256))
                pose, recs, rc = ctx.track_depth_sdf(depth, cam, options=sdf_opt[route])
            else:
                pose, recs, rc = ctx.track_depth_frames(depth, None, cam, to, so)
            dt = time.perf_counter() - t0
            if rep:
                times[route].append(dt)
            err[route] = dict(status=rc, iterations=[r["iterations"] for r in recs],
                              final_translation_error_m=float(np.linalg.norm(pose[:3, 3].astype(np.float64) - gt[-1][:3, 3])))
        ms = C.c_float(0)                               # (the volume holds the sequence sdf_color_all has just fused,
        ctx._ck(lib.icp_debug_sdf_time(ctx.h, binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(sdf_opt["sdf_all"]), C.byref(ms)))
        msc = C.c_float(0)                              #  geometry and colours)
        ctx._ck(lib.icp_debug_sdf_color_time(ctx.h, binding._ptr(d2), binding._ptr(c2), C.byref(cam), binding._ptr(p2), C.byref(sdf_opt["sdf_all"]), C.byref(co), C.byref(msc)))
        if rep:
            pair_ms.append(ms.value); color_pair_ms.append(msc.value)
    n = a.frames - 1
    out["tracking"] = {k: dict(median_s=median(v), frames_per_s_median=n / median(v), frames_per_s_best=n / min(v), **err[k]) for k, v in times.items()}
    out["tracking"]["sdf_pair_ms_median"] = median(pair_ms)
    tr = out["tracking"]
    tr["sdf_color_pair_ms_median"] = median(color_pair_ms)
    tr["sdf_color_over_model_color"] = tr["sdf_color_all"]["frames_per_s_median"] / tr["model_color"]["frames_per_s_median"]
    tr["sdf_color_time_over_sdf_paint"] = tr["sdf_color_all"]["median_s"] / tr["sdf_paint_all"]["median_s"]
    tr["sdf_color_time_over_sdf"] = tr["sdf_color_all"]["median_s"] / tr["sdf_all"]["median_s"]
    out["tracking"]["sdf_over_model"] = out["tracking"]["sdf_all"]["frames_per_s_median"] / out["tracking"]["model"]["frames_per_s_median"]
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
