"""The coloured model on the clock, on the synthetic room at 640 x 480 with the 256^3 volume of tools/time_tsdf.py:
  kernels : device time of one icp_tsdf_integrate_color against one icp_tsdf_integrate, and of one icp_tsdf_raycast_color against one
            icp_tsdf_raycast (events around the launch: icp_debug_tsdf_color_time / icp_debug_tsdf_time), each from a volume holding 4 frames
  tracking: frames/s of icp_track_depth_model_color under colour weighting and under the colored metric against icp_track_depth_model
            with point-to-plane, on the 12-frame sequence (k-NN on the LBVH, 35 iterations, max distance 0.1, source (false, 8))
The yardsticks are the geometry-only calls.  Repeats are interleaved (every configuration once per round) and the median is reported.
Stage timing is off.
usage: python tools/time_tsdf_color.py [--reps 9] [--frames 12] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from icp_amd import binding, synth, tum
from time_tsdf import median, volume_options


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = tum.TUM_K
    T = [synth.camera_pose(k) for k in range(a.frames)]
    frames = [synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05) for k, Tk in enumerate(T)]
    depth = np.stack([f[0][:, 2].reshape(H, W).copy() for f in frames])
    rgbx = np.stack([np.ascontiguousarray(f[2], np.uint8) for f in frames])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames, volume=256)

    # kernels: two contexts holding the same four frames, one with colours
    plain, col = binding.Context(0), binding.Context(0)
    plain.tsdf_create(**volume_options(256)); col.tsdf_create(color=True, **volume_options(256))
    for k in range(4):
        updated = plain.tsdf_integrate(depth[k], cam, gt[k])
        updated_c, coloured = col.tsdf_integrate(depth[k], cam, gt[k], rgbx=rgbx[k])
    _, _, _, _, hits, hits_c = col.tsdf_raycast_color(cam, gt[1])
    d2 = np.ascontiguousarray(depth[2], np.float32); c2 = np.ascontiguousarray(rgbx[2], np.uint8); p2 = binding.pose_to_c(gt[2])
    ms = dict(integrate=[], integrate_color=[], raycast=[], raycast_color=[])
    for rep in range(a.reps + 1):                       # the first round warms up
        for which, key in ((0, "integrate"), (1, "raycast")):
            t = C.c_float(0)
            plain._ck(lib.icp_debug_tsdf_time(plain.h, C.c_int32(which), binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(t)))
            tc = C.c_float(0)
            col._ck(lib.icp_debug_tsdf_color_time(col.h, C.c_int32(which), binding._ptr(d2), binding._ptr(c2), C.byref(cam), binding._ptr(p2), C.byref(tc)))
            if rep:
                ms[key].append(t.value); ms[key + "_color"].append(tc.value)
    out["kernels"] = dict(updated_voxels=updated, coloured_voxels=coloured, hits=hits, coloured_hits=hits_c,
                          **{k + "_ms_median": median(v) for k, v in ms.items()},
                          integrate_color_over_integrate=median(ms["integrate_color"]) / median(ms["integrate"]),
                          raycast_color_over_raycast=median(ms["raycast_color"]) / median(ms["raycast"]))
    assert updated == updated_c
    plain.close(); col.close()

    # tracking
    ctx = binding.Context(0)
    so = binding.depth_options(False, 8, fix_color_index=True)
    routes = dict(model_point_to_plane=dict(metric=1, weighting=0, color=False), model_color_weighting=dict(metric=1, weighting=3, color=True),
                  model_colored_metric=dict(metric=4, weighting=0, color=True))
    times = {k: [] for k in routes}
    err = {}
    for rep in range(a.reps + 1):
        for route, r in routes.items():
            ctx.params.metric = r["metric"]; ctx.params.weighting = r["weighting"]; ctx.params.knn_backend = 1
            tum.reconstruct_room_params(ctx.params)
            ctx.push_params(); ctx.set_stage_timing(0)
            t0 = time.perf_counter()
            ctx.tsdf_create(color=r["color"], **volume_options(256))
            pose, recs, rc = ctx.track_depth_model(depth, cam, so, rgbx_frames=rgbx if r["color"] else None)
            dt = time.perf_counter() - t0
            if rep:
                times[route].append(dt)
            err[route] = dict(status=rc, iterations=[x["iterations"] for x in recs],
                              final_translation_error_m=float(np.linalg.norm(pose[:3, 3].astype(np.float64) - gt[-1][:3, 3])))
    n = a.frames - 1
    out["tracking"] = {k: dict(median_s=median(v), frames_per_s_median=n / median(v), frames_per_s_best=n / min(v), **err[k]) for k, v in times.items()}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
