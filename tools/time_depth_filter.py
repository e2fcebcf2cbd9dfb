"""The bilateral depth filter on the clock, on the synthetic room at 640 x 480 with 2 mm of depth noise:
  kernel  : device time of ONE k_depth_filter launch for radius 1 .. 4 at the default sigmas, between two events around the launch with the
            frame already on the device and the code object loaded (icp_debug_depth_filter_time), and of ONE device-to-device copy of the
            same 1.2 MB between the same events -- the floor: a filter reads the frame once and writes it once.  Every configuration once per
            round, the rounds interleaved; median, minimum and maximum over the rounds.  A window of one launch is a few microseconds, as
            much the events' own cost as the kernel's, so each configuration is also timed as BATCH launches back to back between one
            pair of events, divided by BATCH (`batch_us`): that is the figure to compare.
  tracking: wall time per tracked frame of icp_track_depth_sdf (256^3 volume of tools/time_tsdf.py, stride 1, 20 iterations, stops off) and of
            icp_track_depth_model (point-to-plane k-NN on the LBVH, 35 iterations, max distance 0.1, source (false, 8)) on the 12-frame
            sequence, with the filter off and on (radius 3), the four interleaved per round; median over the rounds.
Stage timing is off.
usage: python tools/time_depth_filter.py [--reps 9] [--frames 12] [--json out.json]"""
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

EXTENT, ORIGIN = 8.96, (-4.2, -4.5, -1.5)          # tools/time_tsdf.py's volume
SIGMA = 0.002
BATCH = 200


def volume_options(n):
    s = EXTENT / n
    return dict(dims=(n, n, n), origin=tuple(o + s / 2 for o in ORIGIN), voxel_size=s, truncation=5 * s)


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = tum.TUM_K
    T = [synth.camera_pose(k) for k in range(a.frames)]
    depth = np.stack([synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05, sigma=SIGMA)[0][:, 2].reshape(H, W).copy() for k, Tk in enumerate(T)])
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    fn = lib.icp_debug_depth_filter_time
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames, sigma_m=SIGMA, frame_bytes=W * H * 4)

    # kernel
    ctx = binding.Context(0)
    d0 = np.ascontiguousarray(depth[0], np.float32)
    ms = dict(copy=[], r1=[], r2=[], r3=[], r4=[])
    batch = {k: [] for k in ms}
    for rep in range(a.reps + 1):                       # the first round warms up
        for key in ms:
            if key != "copy":
                ctx.set_depth_filter(radius=int(key[1]))
            t = C.c_float(0)
            ctx._ck(fn(ctx.h, 1 if key == "copy" else 0, binding._ptr(d0), W, H, 1, C.byref(t)))
            tb = C.c_float(0)
            ctx._ck(fn(ctx.h, 1 if key == "copy" else 0, binding._ptr(d0), W, H, BATCH, C.byref(tb)))
            if rep:
                ms[key].append(t.value); batch[key].append(tb.value / BATCH * 1e3)
    out["kernel_ms"] = {k: stats(v) for k, v in ms.items()}
    out["batch_us"] = {k: stats(v) for k, v in batch.items()}
    for k, v in out["batch_us"].items():
        v["gb_per_s"] = 2 * W * H * 4 / (v["median"] * 1e-6) / 1e9      # one read and one write of the frame
    ctx.set_depth_filter(radius=0)

    # tracking
    ctx.params.metric = 1; ctx.params.knn_backend = 1
    tum.reconstruct_room_params(ctx.params)
    ctx.push_params(); ctx.set_stage_timing(0)
    _, so = tum.reconstruct_room_options(ctx.params)
    sdf_all = binding.sdf_options(stride=1, n_iterations=20, stop_rotation=0.0, stop_translation=0.0)
    times = dict(sdf_off=[], sdf_on=[], model_off=[], model_on=[])
    last = {}
    for rep in range(a.reps + 1):
        for route in times:
            ctx.set_depth_filter(radius=3 if route.endswith("_on") else 0)
            ctx.tsdf_create(**volume_options(256))
            t0 = time.perf_counter()
            if route.startswith("sdf"):
                pose, recs, rc = ctx.track_depth_sdf(depth, cam, options=sdf_all)
            else:
                pose, recs, rc = ctx.track_depth_model(depth, cam, so)
            dt = time.perf_counter() - t0
            if rep:
                times[route].append(dt / (a.frames - 1) * 1e3)
            last[route] = dict(status=rc, iterations=[r["iterations"] for r in recs])
    out["tracked_frame_ms"] = {k: dict(stats(v), **last[k]) for k, v in times.items()}
    tf = out["tracked_frame_ms"]
    tf["sdf_on_minus_off_ms"] = tf["sdf_on"]["median"] - tf["sdf_off"]["median"]
    tf["model_on_minus_off_ms"] = tf["model_on"]["median"] - tf["model_off"]["median"]
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
