"""The coloured views of the hashed TSDF volume on the clock, in tools/time_htsdf_raycast.py's and
tools/time_htsdf_color.py's setting: the 640 x 480 synthetic room sequence with its colour frames fused at its true poses into a coloured
hashed volume, at 35 mm voxels (the 8.96 m cube at 256^3) and at 1 cm.  In ONE process:
  raycast : device time of ONE coloured hashed ray-cast (icp_debug_htsdf_raycast_color_time) against ONE geometric hashed ray-cast of the
            same volume (icp_debug_htsdf_raycast_time) and against ONE icp_tsdf_raycast_color (icp_debug_tsdf_color_time) on the dense
            coloured volume over the blocks' bounding box, from three of the fused poses; the box is skipped (and said so) when it has more
            than --max-box-voxels voxels (24 bytes each, built through host arrays)
  mesh    : device time of all passes of ONE icp_tsdf_mesh_color_hashed (icp_debug_htsdf_mesh_color_time) against icp_tsdf_mesh_hashed's
            (icp_debug_htsdf_mesh_time)
  frame   : wall time of a tracked frame (the call's wall time over its tracked frames) of icp_track_depth_model_color_hashed against
            icp_track_depth_model_hashed, the same params
  route   : wall time of tum.densify_hashed_model and one tsdf_raycast_color, the only route to a coloured view before these calls existed
            (under the same box limit, three timed rounds)
Repeats are interleaved (every configuration once per round, the first round warms up); medians with their range.
usage: python tools/time_htsdf_color_view.py [--reps 9] [--frames 12] [--max-box-voxels 268435456] [--json out.json]"""
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
    return dict(median=xs[len(xs) // 2], lo=xs[0], hi=xs[-1], rounds=len(xs))


def copy_of(blocks, o, ctx):
    """`ctx` holding a coloured hashed volume with these blocks and options; returns ctx."""
    coords, t, w, rgb, cw = blocks
    ctx.tsdf_create_hashed(origin=tuple(o.origin), voxel_size=o.voxel_size, truncation=o.truncation, max_weight=o.max_weight, min_depth=o.min_depth,
                           max_depth=o.max_depth, ray_step=o.ray_step, block_capacity=max(len(coords), 1), color=True)
    ctx.tsdf_upload_blocks(coords, t, w, rgb, cw)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--max-box-voxels", type=int, default=1 << 28)
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
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames, max_box_voxels=a.max_box_voxels)
    views = sorted({0, a.frames // 2, a.frames - 1})
    o0 = tum.reconstruct_room_options(binding.default_params())[1]
    so = binding.depth_options(bool(o0.keep_original_size), int(o0.downsample_factor), float(o0.max_distance), fix_color_index=True)

    for name, voxel in (("35mm", EXTENT / 256), ("1cm", 0.01)):
        hc = binding.Context(0)
        hc.tsdf_create_hashed(block_capacity=1 << 15, color=True, **hashed_options(voxel))
        for k in range(a.frames):
            hc.tsdf_integrate(depth[k], cam, gt[k], rgbx=rgbx[k])
        info, *blocks = hc.tsdf_blocks(colors=True)
        coords = blocks[0]
        dims = (coords.max(0).astype(np.int64) + 1) * 8 - coords.min(0).astype(np.int64) * 8
        box_voxels = int(dims[0]) * int(dims[1]) * int(dims[2])
        res = dict(n_blocks=info["n_blocks"], colored_block_bytes=info["n_blocks"] * 12288, dense_box_dims=[int(d) for d in dims], dense_box_colored_bytes=24 * box_voxels)
        dense = None
        if box_voxels <= a.max_box_voxels:
            dense = binding.Context(0)
            tum.densify_hashed_model(copy_of(blocks, hc.tsdf_hashed_options, dense))
        else:
            res["not_taken"] = "the dense coloured box of %d voxels exceeds --max-box-voxels: no icp_tsdf_raycast_color figure and no densify route at this size" % box_voxels
        loops = {}
        for kind in ("color", "geometric"):
            c = binding.Context(0)
            tum.reconstruct_room_params(c.params, K, W, H); c.push_params()
            loops[kind] = c
        route = binding.Context(0)
        t = {}
        ms, host_ms = C.c_float(0), C.c_float(0)
        counts = (C.c_int32 * 3)()
        for rep in range(a.reps + 1):                   # the first round warms up
            r = {}
            for v in views:
                p = binding.pose_to_c(gt[v])
                hc._ck(lib.icp_debug_htsdf_raycast_color_time(hc.h, B(cam), P(p), B(ms))); r["raycast_color_hashed_view%d_ms" % v] = ms.value
                hc._ck(lib.icp_debug_htsdf_raycast_time(hc.h, B(cam), P(p), B(ms))); r["raycast_hashed_view%d_ms" % v] = ms.value
                if dense is not None:
                    dense._ck(lib.icp_debug_tsdf_color_time(dense.h, C.c_int32(1), None, None, B(cam), P(p), B(ms))); r["raycast_color_dense_view%d_ms" % v] = ms.value
            hc._ck(lib.icp_debug_htsdf_mesh_color_time(hc.h, C.c_float(0), B(ms))); r["mesh_color_hashed_ms"] = ms.value
            hc._ck(lib.icp_debug_htsdf_mesh_time(hc.h, C.c_float(0), B(ms), B(host_ms), None, counts)); r["mesh_hashed_ms"] = ms.value
            tracked = a.frames - 1
            c = loops["color"]
            c.tsdf_create_hashed(block_capacity=1 << 15, color=True, **hashed_options(voxel))
            t0 = time.perf_counter(); _, recs, _ = c.track_depth_model_hashed(depth, cam, so, rgbx_frames=rgbx)
            r["frame_model_color_hashed_wall_ms"] = 1e3 * (time.perf_counter() - t0) / tracked
            res["statuses_color"] = sorted(set(x["status"] for x in recs))
            c = loops["geometric"]
            c.tsdf_create_hashed(block_capacity=1 << 15, **hashed_options(voxel))
            t0 = time.perf_counter(); _, recs, _ = c.track_depth_model_hashed(depth, cam, so)
            r["frame_model_hashed_wall_ms"] = 1e3 * (time.perf_counter() - t0) / tracked
            res["statuses_geometric"] = sorted(set(x["status"] for x in recs))
            if dense is not None and rep <= 3:          # the route goes through host arrays: three timed rounds
                copy_of(blocks, hc.tsdf_hashed_options, route)
                t0 = time.perf_counter()
                tum.densify_hashed_model(route)
                route.tsdf_raycast_color(cam, gt[views[-1]])
                r["view_densify_then_raycast_color_wall_ms"] = 1e3 * (time.perf_counter() - t0)
                route.tsdf_release()
            if rep:
                for k, x in r.items():
                    t.setdefault(k, []).append(x)
        res.update({k: stats(x) for k, x in t.items()})
        med = {k: stats(x)["median"] for k, x in t.items()}
        res.update(mesh_vertices=counts[0], mesh_triangles=counts[1], hits=[list(hc.tsdf_raycast_color_hashed(cam, gt[v])[4:6]) for v in views], views=views,
                   raycast_color_over_geometric_hashed=[med["raycast_color_hashed_view%d_ms" % v] / med["raycast_hashed_view%d_ms" % v] for v in views],
                   mesh_color_over_geometric_hashed=med["mesh_color_hashed_ms"] / med["mesh_hashed_ms"],
                   frame_color_over_geometric=med["frame_model_color_hashed_wall_ms"] / med["frame_model_hashed_wall_ms"])
        if dense is not None:
            res["raycast_color_hashed_over_dense"] = [med["raycast_color_hashed_view%d_ms" % v] / med["raycast_color_dense_view%d_ms" % v] for v in views]
            res["densify_route_over_color_hashed_frame"] = med["view_densify_then_raycast_color_wall_ms"] / med["frame_model_color_hashed_wall_ms"]
        out[name] = res
        for c in [hc, dense, route] + list(loops.values()):
            if c is not None:
                c.close()
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
