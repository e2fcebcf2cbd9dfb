"""Times the depth mesh of reconstructRoom (icp_depth_mesh, SimpleMesh.h:36-119) on a seeded synthetic 640 x 480 frame, median of --reps:
  device      : the wall time of one icp_depth_mesh call (upload + three kernels and the scan + read-back), threshold 0.1, with colours
  restatement : the numpy restatement of tests/test_depth_mesh_host.py on the same frame (the host route it replaces)
  write_off   : meshio.write_off of the joined mesh (depth mesh + camera glyph)
  room        : frames/s of tum.reconstruct_room on a synthetic TUM directory (21 frames: 3 scheduled), with and without out_dir
The kernel time per pass comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--only-device, so the trace holds
nothing else).  The tool checks that the device and the restatement agree bit for bit.
usage: python tools/time_depth_mesh.py [--reps 5] [--json out.json] [--only-device]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding, meshio, synth, tum


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-device", action="store_true")
    a = ap.parse_args()
    W, H = 640, 480
    K = tum.TUM_K
    pose = synth.make_pose((0.02, -0.03, 0.01), (0.05, 0.02, -0.04)).astype(np.float32)
    pts, _, rgba = synth.depth_frame(synth.camera_pose(0), K.astype(np.float64), W, H, 0x7A11, 0.05)
    depth = pts[:, 2].reshape(H, W).copy()
    ctx = binding.Context(0)
    cam = binding.depth_camera(K, W, H)
    mesh = ctx.depth_mesh(depth, rgba, cam, pose, 0.1)                # warm-up: code objects, buffers
    res = dict(width=W, height=H, reps=a.reps, n_triangles=int(len(mesh[2])))
    res["device_ms"], res["device_all_ms"] = median_ms(lambda: ctx.depth_mesh(depth, rgba, cam, pose, 0.1), a.reps)
    if not a.only_device:
        from test_depth_mesh_host import mesh_spec
        spec = mesh_spec(depth, rgba, K, pose, 0.1)
        res["bit_exact"] = bool(np.array_equal(spec[0].view(np.uint32), mesh[0].view(np.uint32)) and np.array_equal(spec[1], mesh[1])
                                and np.array_equal(spec[2], mesh[2]))
        res["restatement_ms"], _ = median_ms(lambda: mesh_spec(depth, rgba, K, pose, 0.1), a.reps)
        joined = meshio.join_meshes(mesh, meshio.camera_glyph(pose))
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "mesh.off")
            res["write_off_ms"], _ = median_ms(lambda: meshio.write_off(path, *joined), a.reps)
            res["off_bytes"] = os.path.getsize(path)
            seq_dir = os.path.join(d, "seq")
            tum.write_synthetic_sequence(seq_dir, 21)
            seq = tum.load_sequence(seq_dir)
            n = len(seq["frames"])

            def room(out_dir):
                p = binding.default_params(); p.metric = 1; p.knn_backend = 1
                tum.reconstruct_room(ctx, seq, p, out_dir=out_dir)
            room(None)
            ms, _ = median_ms(lambda: room(None), a.reps)
            res["room_fps_no_out"] = n / (ms / 1e3)
            ms, _ = median_ms(lambda: room(os.path.join(d, "out")), a.reps)
            res["room_fps_out"] = n / (ms / 1e3)
            res["room_frames"] = n
    ctx.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
