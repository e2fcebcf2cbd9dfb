"""icp_tsdf_mesh on the clock, on the synthetic room at 640 x 480 fused (4 frames) into a 256^3 and a 512^3 volume over
the same 8.96 m cube (tools/time_tsdf.py's volumes):
  mesh     : device time of ALL passes of one icp_tsdf_mesh -- counting, the two scans, scatter, normals included -- between two events
             (icp_debug_tsdf_mesh_time), V and T, and the bytes of volume read per second (8 bytes per voxel: the volume is streamed once);
             against the streaming floor, 8 bytes per voxel per pass over the volume at the achievable HBM rate (6.3 TB/s)
  call     : host time of Context.tsdf_mesh (the counting call and the filling call, the mesh copied to the host)
  download : host time of icp_tsdf_download of the same volume -- the only complete route before
  one view : device time of icp_tsdf_raycast of one 640 x 480 view (icp_debug_tsdf_time) + host time of icp_depth_mesh of its depth image --
             the partial route
Repeats are interleaved (every configuration once per round) and the median is reported.
usage: python tools/time_tsdf_mesh.py [--reps 9] [--skip-512] [--json out.json]"""
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
HBM_ACHIEVABLE = 6.3e12                            # bytes per second


def volume_options(n):
    s = EXTENT / n
    return dict(dims=(n, n, n), origin=tuple(o + s / 2 for o in ORIGIN), voxel_size=s, truncation=5 * s)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-512", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = tum.TUM_K
    T = [synth.camera_pose(k) for k in range(4)]
    depth = np.stack([synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05)[0][:, 2].reshape(H, W).copy() for k, Tk in enumerate(T)])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    out = dict(width=W, height=H, reps=a.reps, volumes={})
    sizes = [256] if a.skip_512 else [256, 512]
    ctxs = {}
    for n in sizes:
        c = binding.Context(0)
        c.tsdf_create(**volume_options(n))
        for k in range(4):
            c.tsdf_integrate(depth[k], cam, gt[k])
        v, nr, t = c.tsdf_mesh()
        ctxs[n] = c
        out["volumes"][str(n)] = dict(voxel_size=EXTENT / n, vertices=len(v), triangles=len(t), mesh_bytes=v.nbytes + nr.nbytes + t.nbytes,
                                      mesh_ms=[], call_ms=[], download_ms=[], raycast_ms=[], depth_mesh_ms=[])
    p1 = binding.pose_to_c(gt[1])
    world_to_cam = np.linalg.inv(gt[1].astype(np.float64)).astype(np.float32)
    for rep in range(a.reps + 1):                       # the first round warms up
        for n in sizes:
            c, r = ctxs[n], out["volumes"][str(n)]
            ms = C.c_float(0)
            c._ck(lib.icp_debug_tsdf_mesh_time(c.h, C.c_float(0.0), C.byref(ms)))
            mesh_ms = ms.value
            t0 = time.perf_counter(); c.tsdf_mesh(); call_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter(); c.tsdf_volume(); download_ms = (time.perf_counter() - t0) * 1e3
            c._ck(lib.icp_debug_tsdf_time(c.h, C.c_int32(1), None, C.byref(cam), binding._ptr(p1), C.byref(ms)))
            d, _, _, _ = c.tsdf_raycast(cam, gt[1])
            t0 = time.perf_counter(); c.depth_mesh(d, None, cam, world_to_cam, 0.1); depth_mesh_ms = (time.perf_counter() - t0) * 1e3
            if rep:
                r["mesh_ms"].append(mesh_ms); r["call_ms"].append(call_ms); r["download_ms"].append(download_ms)
                r["raycast_ms"].append(ms.value); r["depth_mesh_ms"].append(depth_mesh_ms)
    for n in sizes:
        r = out["volumes"][str(n)]
        for key in ("mesh_ms", "call_ms", "download_ms", "raycast_ms", "depth_mesh_ms"):
            r[key + "_median"] = median(r[key])
        vol_bytes = 8.0 * n ** 3
        r["volume_gb_per_s"] = vol_bytes / (r["mesh_ms_median"] * 1e-3) / 1e9
        r["streaming_floor_ms"] = vol_bytes / HBM_ACHIEVABLE * 1e3        # one pass over the volume
        r["times_the_floor"] = r["mesh_ms_median"] / r["streaming_floor_ms"]
        ctxs[n].close()
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
