"""Vertex clustering of the hashed TSDF volume's mesh on the clock: tools/time_htsdf.py's 640 x 480 synthetic room
fused at its true poses, at 35 mm voxels (the 8.96 m cube at 256^3) and at 1 cm, clustered with cells of 2 and of 4 voxels:
  passes  : device time of every clustering step of one icp_tsdf_mesh_clustered with normals, an event after each
            (icp_debug_mesh_cluster_time), and their sum -- with the accumulate in both forms, neighbouring lanes combined (`combine`) and one
            set of atomic adds per vertex (`atomic`) -- beside the device time of the extraction in the same session (icp_debug_htsdf_mesh_time)
  sizes   : vertices, triangles and bytes (vertices, normals, triangles) that cross to the host before and after
  wall    : Context.tsdf_mesh_hashed() with and without cluster=
Repeats are interleaved (every configuration once per round, the first round warms up) and the median is reported.  Every voxel size runs
in a child process of its own under `timeout`; a child that fails ends the run.
usage: python tools/time_mesh_cluster.py [--reps 9] [--frames 12] [--json out.json] [--limit 600]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))

EXTENT, ORIGIN = 8.96, (-4.2, -4.5, -1.5)          # tools/time_tsdf.py's cube, camera-0 coordinates
VOXELS = {"35mm": EXTENT / 256, "1cm": 0.01}
CELLS = (2, 4)
PASSES = ("clear", "vertices", "classify", "insert", "survive_scan", "leaders_scan_rank", "accumulate", "finalize_triangles")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def worker(name, reps, frames):
    import numpy as np
    from icp_amd import binding, synth, tum
    voxel = VOXELS[name]
    W, H, K = tum.TUM_WIDTH, tum.TUM_HEIGHT, tum.TUM_K
    T = [synth.camera_pose(k) for k in range(frames)]
    depth = np.stack([synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05)[0][:, 2].reshape(H, W).copy() for k, Tk in enumerate(T)])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(np.float32) for Tk in T]
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    lib.icp_debug_mesh_cluster_time.argtypes = [C.c_void_p, C.c_float, C.POINTER(binding.IcpMeshClusterOptions), C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                                C.POINTER(binding.IcpMeshClusterInfo)]
    ctx = binding.Context(0)
    origin = tuple(o + voxel / 2 for o in ORIGIN)
    ctx.tsdf_create_hashed(block_capacity=1 << 15, origin=origin, voxel_size=voxel, truncation=5 * voxel)
    for k in range(frames):
        ctx.tsdf_integrate(depth[k], cam, gt[k])
    times, infos = {}, {}
    for rep in range(reps + 1):                         # the first round warms up
        row = {}
        dev, host = C.c_float(0), C.c_float(0)
        counts = (C.c_int32 * 3)()
        ctx._ck(lib.icp_debug_htsdf_mesh_time(ctx.h, C.c_float(0), C.byref(dev), C.byref(host), None, counts))
        row["extract_ms"] = dev.value
        t0 = time.perf_counter()
        v, n, t = ctx.tsdf_mesh_hashed()
        row["wall_plain_ms"] = 1e3 * (time.perf_counter() - t0)
        for cells in CELLS:
            opt = binding.mesh_cluster_options(cells * voxel, origin)
            for form, combine in (("combine", 1), ("atomic", 0)):
                ps = (C.c_float * len(PASSES))(); info = binding.IcpMeshClusterInfo()
                ctx._ck(lib.icp_debug_mesh_cluster_time(ctx.h, 0.0, C.byref(opt), 0, combine, ps, C.byref(info)))
                for p, ms in zip(PASSES, ps):
                    row["cells%d_%s_%s_ms" % (cells, form, p)] = ms
                row["cells%d_%s_sum_ms" % (cells, form)] = sum(ps)
                infos[cells] = binding._record(info)
            t0 = time.perf_counter()
            cv, cn, ct = ctx.tsdf_mesh_hashed(cluster=cells * voxel)
            row["cells%d_wall_clustered_ms" % cells] = 1e3 * (time.perf_counter() - t0)
            assert (len(cv), len(ct)) == (infos[cells]["n_vertices"], infos[cells]["n_triangles"])
        if rep:
            for k, x in row.items():
                times.setdefault(k, []).append(x)
    out = dict(voxel=voxel, n_blocks=int(counts[2]), V=len(v), T=len(t), bytes_plain=len(v) * 24 + len(t) * 12,
               median={k: median(x) for k, x in times.items()}, min={k: min(x) for k, x in times.items()}, max={k: max(x) for k, x in times.items()})
    for cells in CELLS:
        i = infos[cells]
        out["cells%d" % cells] = dict(i, cell_size=cells * voxel, bytes_clustered=i["n_vertices"] * 24 + i["n_triangles"] * 12,
                                      triangles_ratio=len(t) / max(i["n_triangles"], 1))
    ctx.close()
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--limit", type=int, default=600, help="seconds every voxel size's child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps, a.frames)
    out = dict(reps=a.reps, frames=a.frames, passes=list(PASSES))
    for name in VOXELS:                                 # a fresh child per voxel size, under its own time limit; a failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--reps", str(a.reps), "--frames", str(a.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print("the %s run ended with status %d: stopping" % (name, r.returncode), file=sys.stderr)
            return r.returncode
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
