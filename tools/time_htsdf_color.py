"""The coloured hashed TSDF volume on the clock, in tools/time_htsdf.py's setting: the 640 x 480 synthetic room
sequence with its colour frames, the 8.96 m cube at 35 mm voxels (truncation 5 voxels) and at 1 cm, from volumes holding 4 frames.
In ONE process:
  integrate: device time of ONE k_htsdf_integrate_color launch (icp_debug_htsdf_color_time) against ONE k_htsdf_integrate over the same
             blocks (icp_debug_htsdf_time) and against ONE k_tsdf_integrate_color over the blocks' bounding box (icp_debug_tsdf_color_time
             on a dense coloured volume of that box; 35 mm only -- at 1 cm the box does not fit a dense coloured volume's 24 bytes per voxel
             everywhere, so it is skipped when the box has more than 2^29 voxels)
  pair     : ONE k_hsdf_accumulate_color + k_sdf_solve_color pair (icp_debug_sdf_color_time on the coloured hashed volume) against the
             geometric hashed pair (icp_debug_sdf_time) and against the dense coloured and dense geometric pairs on the cube at 256^3
  tracking : ms per tracked frame of track_depth_sdf on the coloured hashed volume with color_weight 0.1 and with color_weight 0 (the
             colours still fused), 20 iterations, stops off
  evict    : ONE icp_tsdf_evict_blocks (icp_debug_htsdf_evict_time, hold=1) that removes the blocks beyond 2.5 m, with and without colours
  memory   : bytes of both models after the sequence: blocks x (4 KiB | 12 KiB) against the dense cube at 8 | 24 bytes per voxel
Repeats are interleaved (every configuration once per round), the first round warms up, medians with their range.  Stage timing is off.
usage: python tools/time_htsdf_color.py [--reps 9] [--frames 12] [--json out.json]"""
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


def hashed_options(voxel):
    return dict(origin=tuple(o + voxel / 2 for o in ORIGIN), voxel_size=voxel, truncation=5 * voxel)


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], lo=xs[0], hi=xs[-1])


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
    depth = np.stack([m[0][:, 2].reshape(H, W).copy() for m in made]).astype(np.float32)
    rgbx = np.stack([np.ascontiguousarray(m[2]) for m in made]).astype(np.uint8)
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    P, B = binding._ptr, C.byref
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames)
    d2 = np.ascontiguousarray(depth[2]); c2 = np.ascontiguousarray(rgbx[2]); p2 = binding.pose_to_c(gt[2])
    one = binding.sdf_options(stride=1, n_iterations=20, stop_rotation=0.0, stop_translation=0.0)
    co = binding.sdf_color_options(weight=0.1)

    for voxel in (EXTENT / 256, 0.01):
        tag = "%.4g" % voxel
        hc, hg = binding.Context(0), binding.Context(0)
        hc.tsdf_create_hashed(block_capacity=1 << 15, color=True, **hashed_options(voxel)); hg.tsdf_create_hashed(block_capacity=1 << 15, **hashed_options(voxel))
        for k in range(4):
            hc.tsdf_integrate(depth[k], cam, gt[k], rgbx=rgbx[k]); hg.tsdf_integrate(depth[k], cam, gt[k])
        info, coords, *_ = hc.tsdf_blocks()
        lo = coords.min(0).astype(np.int64) * 8; dims = (coords.max(0).astype(np.int64) + 1) * 8 - lo
        box = None
        if int(dims[0]) * int(dims[1]) * int(dims[2]) <= 1 << 29:
            box = binding.Context(0)
            o = hashed_options(voxel)
            box.tsdf_create(color=True, dims=tuple(int(x) for x in dims), origin=tuple(o["origin"][i] + float(lo[i]) * voxel for i in range(3)), voxel_size=voxel,
                            truncation=o["truncation"])
            for k in range(4):
                box.tsdf_integrate(depth[k], cam, gt[k], rgbx=rgbx[k])
        dc = dg = None
        if voxel > 0.02:                                 # the cube at 256^3, as tools/time_tsdf.py has it
            dense = dict(dims=(256, 256, 256), **hashed_options(voxel))
            dc, dg = binding.Context(0), binding.Context(0)
            dc.tsdf_create(color=True, **dense); dg.tsdf_create(**dense)
            for k in range(4):
                dc.tsdf_integrate(depth[k], cam, gt[k], rgbx=rgbx[k]); dg.tsdf_integrate(depth[k], cam, gt[k])
        t = {}
        ms, ms2 = C.c_float(0), C.c_float(0)
        for rep in range(a.reps + 1):
            r = {}
            hc._ck(lib.icp_debug_htsdf_color_time(hc.h, P(d2), P(c2), B(cam), P(p2), B(ms))); r["hashed_integrate_color_ms"] = ms.value
            hg._ck(lib.icp_debug_htsdf_time(hg.h, P(d2), B(cam), P(p2), B(ms2), B(ms))); r["hashed_integrate_ms"] = ms.value
            hc._ck(lib.icp_debug_htsdf_time(hc.h, P(d2), B(cam), P(p2), B(ms2), B(ms))); r["hashed_integrate_on_colored_ms"] = ms.value
            if box is not None:
                box._ck(lib.icp_debug_tsdf_color_time(box.h, C.c_int32(0), P(d2), P(c2), B(cam), P(p2), B(ms))); r["box_integrate_color_ms"] = ms.value
            hc._ck(lib.icp_debug_sdf_color_time(hc.h, P(d2), P(c2), B(cam), P(p2), B(one), B(co), B(ms))); r["hashed_pair_color_ms"] = ms.value
            hg._ck(lib.icp_debug_sdf_time(hg.h, P(d2), B(cam), P(p2), B(one), B(ms))); r["hashed_pair_ms"] = ms.value
            if dc is not None:
                dc._ck(lib.icp_debug_sdf_color_time(dc.h, P(d2), P(c2), B(cam), P(p2), B(one), B(co), B(ms))); r["dense_pair_color_ms"] = ms.value
                dg._ck(lib.icp_debug_sdf_time(dg.h, P(d2), B(cam), P(p2), B(one), B(ms))); r["dense_pair_ms"] = ms.value
            if rep:
                for k, v in r.items():
                    t.setdefault(k, []).append(v)
        res = {k: stats(v) for k, v in t.items()}
        med = {k: v["median"] for k, v in res.items()}
        res.update(n_blocks=info["n_blocks"], box_dims=[int(x) for x in dims],
                   integrate_color_over_geometric=med["hashed_integrate_color_ms"] / med["hashed_integrate_ms"],
                   pair_color_over_geometric_hashed=med["hashed_pair_color_ms"] / med["hashed_pair_ms"])
        if box is not None:
            res["integrate_color_hashed_over_box"] = med["hashed_integrate_color_ms"] / med["box_integrate_color_ms"]
        if dc is not None:
            res["pair_color_over_geometric_dense"] = med["dense_pair_color_ms"] / med["dense_pair_ms"]
            res["pair_color_hashed_over_dense"] = med["hashed_pair_color_ms"] / med["dense_pair_color_ms"]
        out["kernels_" + tag] = res
        for c in (hc, hg, box, dc, dg):
            if c is not None:
                c.close()

    # tracking and evict at 35 mm
    ctx = binding.Context(0)
    ctx.set_stage_timing(0)
    opts = hashed_options(EXTENT / 256)
    times = dict(colored=[], geometric_with_fusion=[], geometric=[])
    errs = {}
    for rep in range(a.reps + 1):
        for route in times:
            t0 = time.perf_counter()
            ctx.tsdf_create_hashed(color=route != "geometric", **opts)
            if route == "colored":
                pose, recs, rc = ctx.track_depth_sdf(depth, cam, rgbx_frames=rgbx, options=one, color_weight=0.1)
            elif route == "geometric_with_fusion":
                pose, recs, rc = ctx.track_depth_sdf(depth, cam, rgbx_frames=rgbx, options=one)
            else:
                pose, recs, rc = ctx.track_depth_sdf(depth, cam, options=one)
            dt = time.perf_counter() - t0
            if rep:
                times[route].append(1e3 * dt / (a.frames - 1))
            errs[route] = dict(status=rc, final_translation_error_m=float(np.linalg.norm(pose[:3, 3].astype(np.float64) - gt[-1][:3, 3])))
    out["tracking_ms_per_frame"] = {k: dict(stats(v), **errs[k]) for k, v in times.items()}
    out["tracking_ms_per_frame"]["colored_over_geometric"] = stats(times["colored"])["median"] / stats(times["geometric"])["median"]

    ev = dict(colored=[], geometric=[])
    n_ev = {}
    centre = np.zeros(3, np.float32)
    for rep in range(a.reps + 1):
        for route in ev:
            ctx.tsdf_create_hashed(color=route == "colored", **opts)
            for k in range(a.frames):
                ctx.tsdf_integrate(depth[k], cam, gt[k], rgbx=rgbx[k] if route == "colored" else None)
            st = binding.IcpTsdfStreamInfo(); ms = C.c_float(0)
            ctx._ck(lib.icp_debug_htsdf_evict_time(ctx.h, P(centre), C.c_float(2.5), C.c_int32(1), B(st), B(ms)))
            n_ev[route] = dict(n_evicted=st.n_evicted, n_kept=st.n_blocks, n_moved=st.n_moved)
            if rep:
                ev[route].append(ms.value)
    out["evict_ms"] = {k: dict(stats(v), **n_ev[k]) for k, v in ev.items()}
    out["evict_ms"]["colored_over_geometric"] = stats(ev["colored"])["median"] / stats(ev["geometric"])["median"]

    out["memory"] = {}
    for voxel in (EXTENT / 256, 0.01):
        ctx.tsdf_create_hashed(color=True, **hashed_options(voxel))
        for k in range(a.frames):
            ctx.tsdf_integrate(depth[k], cam, gt[k], rgbx=rgbx[k])
        info = ctx.tsdf_blocks()[0]
        side = int(round(EXTENT / voxel))
        out["memory"]["%.4g" % voxel] = dict(n_blocks=info["n_blocks"], capacity=info["capacity"], geometry_block_bytes=info["n_blocks"] * 4096,
                                            colored_block_bytes=info["n_blocks"] * 12288, colored_held_bytes=info["capacity"] * (12288 + 8 + 2 * 12),
                                            dense_side=side, dense_bytes=8 * side ** 3, dense_colored_bytes=24 * side ** 3,
                                            dense_colored_over_colored_blocks=24 * side ** 3 / max(info["n_blocks"] * 12288, 1))
    ctx.tsdf_release()
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
