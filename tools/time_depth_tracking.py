"""Frames per second of reconstructRoom's tracking loop (main.cpp:183-341) on a synthetic 640 x 480 sequence of 12 frames, two ways:
  device : icp_track_depth_frames -- depth + colour frames go up once, the clouds are built in place (dev_depth.hpp)
  host   : the route it replaces -- per frame icp_backproject_depth (organised cloud back to the host), the constructor's stride and
           filter in numpy, icp_set_source, icp_run (frame 0: the same, keepOriginalSize per the options, icp_set_target)
Both run point-to-plane k-NN (LBVH), 35 iterations, max distance 0.1, source (false, 8) -- the reference's default variant -- from the
same frames, and the tool checks that both end on the same poses.  Stage timing is off in both.  Frames/s counts the 11 tracked frames
and the wall clock includes frame 0's target.  --convergence ROT,TRANS stops every frame's run on a converged pose
(icp_set_convergence_options) in both routes; the iterations every frame ran are reported.
usage: python tools/time_depth_tracking.py [--reps 5] [--convergence 1e-6,1e-6] [--json out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))
import numpy as np
from icp_amd import binding, synth, tum


def make_frames(n, W, H):
    K = tum.TUM_K
    depth, rgbx = [], []
    for k in range(n):
        pts, _, rgba = synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), W, H, 0x7A11 + k, 0.05)
        depth.append(pts[:, 2].reshape(H, W).copy()); rgbx.append(rgba)
    return K, np.stack(depth), np.stack(rgbx)


def host_route(ctx, K, depth, rgbx, to, so):
    def cloud(k, opt):
        xyz, nrm, rgba, valid = ctx.backproject_depth(depth[k], rgbx[k], K, max_distance=opt.max_distance)
        idx = np.arange(0, depth[k].size, opt.downsample_factor)
        sel = idx[valid[idx] | bool(opt.keep_original_size)]
        return xyz[sel], nrm[sel], rgba[sel]
    ctx.set_target(*cloud(0, to))
    pose = np.eye(4, dtype=np.float32); poses = []
    for k in range(1, len(depth)):
        ctx.set_source(*cloud(k, so))
        pose, _, _ = ctx.run(pose, max_stats=64, check=False)
        poses.append(pose)
    return poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--convergence", default=None, help="rotation_eps,translation_eps")
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K, depth, rgbx = make_frames(a.frames, W, H)
    ctx = binding.Context(0)
    ctx.params.metric = 1; ctx.params.knn_backend = 1
    tum.reconstruct_room_params(ctx.params)
    ctx.push_params(); ctx.set_stage_timing(0)
    if a.convergence:
        rot, trans = (float(x) for x in a.convergence.split(","))
        ctx.set_convergence_options(rot, trans)
    to, so = tum.reconstruct_room_options(ctx.params)
    cam = binding.depth_camera(K, W, H)
    res = {}
    for route in ("device", "host", "device", "host"):          # first pass of each warms up (allocations, code objects)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            if route == "device":
                _, recs, rc = ctx.track_depth_frames(depth, rgbx, cam, to, so)
                poses = [r["pose"] for r in recs]; iterations = [r["iterations"] for r in recs]
            else:
                poses = host_route(ctx, K, depth, rgbx, to, so)
            times.append(time.perf_counter() - t0)
        res[route] = dict(seconds=sorted(times), poses=poses)
    same = all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(res["device"]["poses"], res["host"]["poses"]))
    n = a.frames - 1
    out = dict(frames=a.frames, width=W, height=H, reps=a.reps, poses_bit_identical=bool(same), convergence=a.convergence, iterations=iterations)
    for route in ("device", "host"):
        s = res[route]["seconds"]
        out[route] = dict(median_s=s[len(s) // 2], min_s=s[0], frames_per_s_median=n / s[len(s) // 2], frames_per_s_best=n / s[0])
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
