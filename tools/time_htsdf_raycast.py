"""The ray-cast of the hashed TSDF volume on the clock, on tools/time_htsdf.py's 640 x 480 synthetic room fused at its
true poses, at 35 mm voxels (the 8.96 m cube at 256^3) and at 1 cm:
  raycast : device time of ONE icp_tsdf_raycast_hashed launch between two events (icp_debug_htsdf_raycast_time), against ONE
            icp_tsdf_raycast launch (icp_debug_tsdf_time) on the dense volume over the bounding box of the blocks, the volume resident --
            the only route to a view before this call existed --, from three of the fused poses
  frame   : wall time of a tracked frame (the call's wall time over its tracked frames) of icp_track_depth_model_hashed, against
            icp_track_depth_model on that box, against icp_track_depth_sdf on the hashed volume (stride 4, 20 iterations), and against
            densify-then-ray-cast: tum.densify_hashed_model and one tsdf_raycast per view, what a frame of a model loop would have had to do
  causes  : with --breakdown, on the CPU from the restatement's trace (tests/htsdf_raycast_restatement.py): the share of samples whose
            lowest corner's block is missing, the share answered by the per-lane cache, the share of cells in 2, 4 or 8 blocks, probes per ray
Repeats are interleaved (every configuration once per round, the first round warms up) and the median is reported.
usage: python tools/time_htsdf_raycast.py [--reps 9] [--frames 12] [--breakdown] [--json out.json]"""
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
SDF = dict(stride=4, n_iterations=20)


def hashed_options(voxel):
    return dict(origin=tuple(o + voxel / 2 for o in ORIGIN), voxel_size=voxel, truncation=5 * voxel)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def copy_of(coords, t, w, o, ctx):
    """`ctx` holding a hashed volume with these blocks and options; returns ctx."""
    ctx.tsdf_create_hashed(origin=tuple(o.origin), voxel_size=o.voxel_size, truncation=o.truncation, max_weight=o.max_weight, min_depth=o.min_depth,
                           max_depth=o.max_depth, ray_step=o.ray_step, block_capacity=max(len(coords), 1))
    ctx.tsdf_upload_blocks(coords, t, w)
    return ctx


def dense_box_options(coords, o):
    lo = coords.min(0).astype(np.int64) * 8
    dims = (coords.max(0).astype(np.int64) + 1) * 8 - lo
    origin = [float(np.float32(np.float32(o.origin[a]) + np.float32(lo[a]) * np.float32(o.voxel_size))) for a in range(3)]
    return dict(dims=tuple(int(d) for d in dims), origin=origin, voxel_size=o.voxel_size, truncation=o.truncation, max_weight=o.max_weight,
                min_depth=o.min_depth, max_depth=o.max_depth, ray_step=o.ray_step)


def breakdown(coords, t, w, o, K, W, H, pose):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import htsdf_raycast_restatement as RR
    import tsdf_restatement as TS
    vol = RR.Blocks(coords, t, w, origin=tuple(o.origin), voxel_size=o.voxel_size, truncation=o.truncation, min_depth=o.min_depth, max_depth=o.max_depth, ray_step=o.ray_step)
    tr = {}
    RR.raycast(vol, TS.Camera(K, W, H), pose, trace=tr)
    n = float(tr["samples"])
    cls = {k: sum(tr["classes"][(k, v)] for v in (True, False)) for k in (1, 2, 4, 8)}
    return dict(samples=tr["samples"], samples_per_ray=n / (W * H), hits=tr["hits"], share_lowest_block_missing=tr["base_missing"] / n, share_cached=tr["cached"] / n,
                share_out_of_range=tr["out_of_range"] / n, share_in_2_blocks=cls[2] / n, share_in_4_blocks=cls[4] / n, share_in_8_blocks=cls[8] / n,
                share_valid=sum(tr["classes"][(k, True)] for k in (1, 2, 4, 8)) / n, probes_per_ray_at_most=tr["probes"] / (W * H))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = tum.TUM_K
    T = [synth.camera_pose(k) for k in range(a.frames)]
    depth = np.stack([synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05)[0][:, 2].reshape(H, W).copy() for k, Tk in enumerate(T)])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames, sdf=SDF)
    vox = {"35mm": EXTENT / 256, "1cm": 0.01}
    views = sorted({0, a.frames // 2, a.frames - 1})
    so = tum.reconstruct_room_options(binding.default_params())[1]

    hashed, dense, blocks, box = {}, {}, {}, {}
    for name, voxel in vox.items():
        c = binding.Context(0)
        c.tsdf_create_hashed(block_capacity=1 << 15, **hashed_options(voxel))
        for k in range(a.frames):
            c.tsdf_integrate(depth[k], cam, gt[k])
        hashed[name] = c
        blocks[name] = c.tsdf_blocks()[1:] + (c.tsdf_hashed_options,)
        box[name] = dense_box_options(blocks[name][0], blocks[name][3])
        dense[name] = binding.Context(0)
        tum.densify_hashed_model(copy_of(*blocks[name], dense[name]))
    loops = {}
    for name in vox:                                    # the tracking contexts: the library's default params with reconstructRoom's settings
        for kind in ("model_hashed", "model_dense", "sdf_hashed"):
            c = binding.Context(0)
            tum.reconstruct_room_params(c.params, K, W, H); c.push_params()
            loops[(name, kind)] = c
    route = binding.Context(0)

    times = {}

    def put(key, ms):
        times.setdefault(key, []).append(ms)
    hits = {}
    for rep in range(a.reps + 1):                       # the first round warms up
        row = {}
        for name, voxel in vox.items():
            for v in views:
                p = binding.pose_to_c(gt[v]); ms = C.c_float(0)
                hashed[name]._ck(lib.icp_debug_htsdf_raycast_time(hashed[name].h, C.byref(cam), binding._ptr(p), C.byref(ms)))
                row["raycast_hashed_%s_view%d_ms" % (name, v)] = ms.value
                dense[name]._ck(lib.icp_debug_tsdf_time(dense[name].h, C.c_int32(1), None, C.byref(cam), binding._ptr(p), C.byref(ms)))
                row["raycast_dense_%s_view%d_ms" % (name, v)] = ms.value
            if rep == 0:
                hits[name] = dict(hashed=[hashed[name].tsdf_raycast_hashed(cam, gt[v])[3] for v in views], dense=[dense[name].tsdf_raycast(cam, gt[v])[3] for v in views])
            tracked = a.frames - 1
            c = loops[(name, "model_hashed")]
            c.tsdf_create_hashed(block_capacity=1 << 15, **hashed_options(voxel))
            t0 = time.perf_counter(); _, recs, _ = c.track_depth_model_hashed(depth, cam, so)
            row["frame_model_hashed_%s_wall_ms" % name] = 1e3 * (time.perf_counter() - t0) / tracked
            out.setdefault("statuses", {})["model_hashed_" + name] = sorted(set(r["status"] for r in recs))
            c = loops[(name, "model_dense")]
            c.tsdf_create(**box[name])
            t0 = time.perf_counter(); _, recs, _ = c.track_depth_model(depth, cam, so)
            row["frame_model_dense_%s_wall_ms" % name] = 1e3 * (time.perf_counter() - t0) / tracked
            out["statuses"]["model_dense_" + name] = sorted(set(r["status"] for r in recs))
            c.tsdf_release()
            c = loops[(name, "sdf_hashed")]
            c.tsdf_create_hashed(block_capacity=1 << 15, **hashed_options(voxel))
            t0 = time.perf_counter(); _, recs, _ = c.track_depth_sdf(depth, cam, **SDF)
            row["frame_sdf_hashed_%s_wall_ms" % name] = 1e3 * (time.perf_counter() - t0) / tracked
            if name == "35mm" or rep <= 3:              # the large box's route takes seconds: three timed rounds
                copy_of(*blocks[name], route)
                t0 = time.perf_counter()
                tum.densify_hashed_model(route)
                route.tsdf_raycast(cam, gt[views[-1]])
                row["view_densify_then_raycast_%s_wall_ms" % name] = 1e3 * (time.perf_counter() - t0)
                route.tsdf_release()
        if rep:
            for k, v_ in row.items():
                put(k, v_)
    out["median"] = {k: median(v) for k, v in times.items()}
    out["min"] = {k: min(v) for k, v in times.items()}
    out["max"] = {k: max(v) for k, v in times.items()}
    out["rounds"] = {k: len(v) for k, v in times.items()}
    m = out["median"]
    for name in vox:
        coords = blocks[name][0]
        dims = box[name]["dims"]
        hd = [m["raycast_hashed_%s_view%d_ms" % (name, v)] / m["raycast_dense_%s_view%d_ms" % (name, v)] for v in views]
        out[name] = dict(n_blocks=len(coords), pool_bytes=len(coords) * 4096, dense_box_dims=list(dims), dense_box_bytes=8 * int(np.prod(dims)), views=views, hits=hits[name],
                         raycast_hashed_over_dense=hd,
                         frame_model_hashed_over_model_dense=m["frame_model_hashed_%s_wall_ms" % name] / m["frame_model_dense_%s_wall_ms" % name],
                         frame_model_hashed_over_sdf_hashed=m["frame_model_hashed_%s_wall_ms" % name] / m["frame_sdf_hashed_%s_wall_ms" % name],
                         densify_then_raycast_over_model_hashed_frame=m["view_densify_then_raycast_%s_wall_ms" % name] / m["frame_model_hashed_%s_wall_ms" % name])
        if a.breakdown:
            out[name]["causes"] = {"view%d" % v: breakdown(*blocks[name], K, W, H, gt[v]) for v in views}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    for c in list(hashed.values()) + list(dense.values()) + list(loops.values()) + [route]:
        c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
