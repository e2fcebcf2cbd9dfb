"""The mesh of the hashed TSDF volume on the clock: icp_tsdf_mesh_hashed against the two routes the same commit offers,
on tools/time_htsdf.py's 640 x 480 synthetic room fused at its true poses, at 35 mm voxels (the 8.96 m cube at 256^3) and at 1 cm:
  hashed  : device time of ALL passes of one call between two events (icp_debug_htsdf_mesh_time), the host time of the order in front of
            them (key download, sort, upload), the passes one by one, V and T, pool bytes read per second (blocks x 4 KiB over the device
            time, and over the classify pass, the one pass over the pool), and the wall time of Context.tsdf_mesh_hashed()
  dense   : device time of icp_tsdf_mesh (icp_debug_tsdf_mesh_time) on the dense volume over the bounding box of the blocks
  densify : wall time of the whole route -- tsdf_blocks, tsdf_blocks_to_dense, create, upload, mesh (tum.densify_hashed_model, then
            Context.tsdf_mesh) -- on a context that holds a copy of the hashed volume (at 1 cm three timed rounds: it takes seconds)
  refusal : the bounding box against icp_tsdf_mesh's voxel rule (INT32_MAX / 12); a box beyond it is not allocated, `dense` and `densify` are
            then left out for that voxel size and densify_route_refused says so
Repeats are interleaved (every configuration once per round, the first round warms up) and the median is reported.
usage: python tools/time_htsdf_mesh.py [--reps 9] [--frames 12] [--json out.json]"""
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
PASSES = ("neighbours", "classify", "cells", "count", "scans", "vertices", "triangles")


def hashed_options(voxel):
    return dict(origin=tuple(o + voxel / 2 for o in ORIGIN), voxel_size=voxel, truncation=5 * voxel)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def hashed_time(ctx, lib):
    dev, host = C.c_float(0), C.c_float(0)
    passes = (C.c_float * 7)(); counts = (C.c_int32 * 3)()
    ctx._ck(lib.icp_debug_htsdf_mesh_time(ctx.h, C.c_float(0), C.byref(dev), C.byref(host), passes, counts))
    return dev.value, host.value, list(passes), list(counts)


def box_of(coords):
    lo = coords.min(0).astype(np.int64) * 8
    return lo, (coords.max(0).astype(np.int64) + 1) * 8 - lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = tum.TUM_K
    T = [synth.camera_pose(k) for k in range(a.frames)]
    depth = np.stack([synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05)[0][:, 2].reshape(H, W).copy() for k, Tk in enumerate(T)])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    out = dict(width=W, height=H, reps=a.reps, frames=a.frames)

    vox = {"35mm": EXTENT / 256, "1cm": 0.01}
    LIMIT = 0x7FFFFFFF // 12                            # icp_tsdf_mesh's voxel rule
    hashed, blocks, box, dense = {}, {}, {}, {}
    for name, voxel in vox.items():
        c = binding.Context(0)
        c.tsdf_create_hashed(block_capacity=1 << 15, **hashed_options(voxel))
        for k in range(a.frames):
            c.tsdf_integrate(depth[k], cam, gt[k])
        hashed[name] = c
        blocks[name] = c.tsdf_blocks()[1:] + (c.tsdf_hashed_options,)
        box[name] = box_of(blocks[name][0])[1]
        if int(np.prod(box[name])) <= LIMIT:             # icp_tsdf_mesh on the bounding box, the volume resident
            dense[name] = binding.Context(0)
            tum.densify_hashed_model(_copy_of(*blocks[name], dense[name]))
    route = binding.Context(0)                          # the densify route, from a hashed volume every time

    keys = ["hashed_%s_ms", "hashed_%s_order_ms", "hashed_%s_wall_ms", "dense_%s_ms", "densify_route_%s_wall_ms"]
    times = {k % name: [] for k in keys for name in vox}
    passes = {name: [] for name in vox}
    counts, mesh_sizes = {}, {}
    for rep in range(a.reps + 1):                       # the first round warms up
        row = {}
        for name in vox:
            dev, host, ps, cn = hashed_time(hashed[name], lib)
            row["hashed_%s_ms" % name] = dev; row["hashed_%s_order_ms" % name] = host
            counts[name] = cn
            t0 = time.perf_counter()
            v, n, t = hashed[name].tsdf_mesh_hashed()
            row["hashed_%s_wall_ms" % name] = 1e3 * (time.perf_counter() - t0)
            mesh_sizes[name] = (len(v), len(t))
            if rep:
                passes[name].append(ps)
            if name not in dense:
                continue
            ms = C.c_float(0)
            dense[name]._ck(lib.icp_debug_tsdf_mesh_time(dense[name].h, C.c_float(0), C.byref(ms)))
            row["dense_%s_ms" % name] = ms.value
            if name != "35mm" and rep > 3:              # the large box's route takes seconds: three timed rounds
                continue
            _copy_of(*blocks[name], route)
            t0 = time.perf_counter()
            tum.densify_hashed_model(route)
            dv, dn, dt = route.tsdf_mesh()
            row["densify_route_%s_wall_ms" % name] = 1e3 * (time.perf_counter() - t0)
            assert (len(dv), len(dt)) == mesh_sizes[name], ((len(dv), len(dt)), mesh_sizes[name])      # the same surface either way
            route.tsdf_release()
        if rep:
            for k, v_ in row.items():
                times[k].append(v_)
    times = {k: v for k, v in times.items() if v}
    out["median"] = {k: median(v) for k, v in times.items()}
    out["min"] = {k: min(v) for k, v in times.items()}
    out["max"] = {k: max(v) for k, v in times.items()}
    out["rounds"] = {k: len(v) for k, v in times.items()}
    for name in vox:
        nv, nt, nb = counts[name]
        med = [median([p[i] for p in passes[name]]) for i in range(7)]
        m = out["median"]
        dev = m["hashed_%s_ms" % name]
        voxels = int(np.prod(box[name]))
        out[name] = dict(n_blocks=nb, pool_bytes=nb * 4096, V=nv, T=nt, passes_ms_median=dict(zip(PASSES, med)),
                         pool_bytes_per_s_over_device_time=nb * 4096 / (dev * 1e-3), pool_bytes_per_s_over_classify=nb * 4096 / max(med[1] * 1e-3, 1e-9),
                         host_order_over_device_time=m["hashed_%s_order_ms" % name] / dev,
                         host_order_share_of_call=m["hashed_%s_order_ms" % name] / max(m["hashed_%s_wall_ms" % name], 1e-9),
                         dense_box_dims=[int(d) for d in box[name]], dense_box_voxels=voxels, dense_box_bytes=8 * voxels, mesh_voxel_limit=LIMIT,
                         densify_route_refused=bool(voxels > LIMIT))
        if name in dense:
            out[name].update(hashed_over_dense_device_time=dev / m["dense_%s_ms" % name],
                             densify_route_over_hashed_wall=m["densify_route_%s_wall_ms" % name] / m["hashed_%s_wall_ms" % name])
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    for c in list(hashed.values()) + list(dense.values()) + [route]:
        c.close()
    return 0


def _copy_of(coords, t, w, o, ctx):
    """`ctx` holding a hashed volume with these blocks and options; returns ctx."""
    ctx.tsdf_create_hashed(origin=tuple(o.origin), voxel_size=o.voxel_size, truncation=o.truncation, max_weight=o.max_weight, min_depth=o.min_depth,
                           max_depth=o.max_depth, ray_step=o.ray_step, block_capacity=max(len(coords), 1))
    ctx.tsdf_upload_blocks(coords, t, w)
    return ctx


if __name__ == "__main__":
    sys.exit(main())
