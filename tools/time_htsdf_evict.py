"""Streaming the hashed TSDF volume on the clock.  Two settings:
  room : tools/time_htsdf.py's -- the 640 x 480 synthetic room sequence, 35 mm voxels, truncation 5 voxels, a volume holding 4 frames:
         ONE icp_tsdf_evict_blocks that removes nothing (icp_debug_htsdf_evict_time: the device's time from the call's first command to its
         last) beside the pieces of one tracked frame of icp_track_depth_sdf on the same volume (20 accumulate + solve pairs, a touch, an
         integrate: icp_debug_sdf_time, icp_debug_htsdf_time) and beside the wall time of a tracked frame; ONE evict that removes a few
         hundred blocks with hold=1, and ONE icp_tsdf_insert_blocks that puts them back (icp_debug_htsdf_insert_time)
  wall : a camera that slides along a wavy wall and back (tests/htsdf_evict_fixture.py's scene at 640 x 480, 25 mm voxels): the integrate
         launch over the pool (icp_debug_htsdf_time) after the whole track on the unbounded volume and on the local one, the blocks each
         holds, and the wall time per frame of tsdf_local.track_depth_sdf_local against icp_track_depth_sdf, in this one process
Repeats are interleaved (every configuration once per round); medians with their range.  Stage timing is off.
usage: python tools/time_htsdf_evict.py [--reps 9] [--out-steps 24] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))
import numpy as np
from icp_amd import binding, synth, tsdf_local, tum

EXTENT, ORIGIN = 8.96, (-4.2, -4.5, -1.5)          # tools/time_htsdf.py's cube, camera-0 coordinates
f32 = np.float32


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], lo=xs[0], hi=xs[-1])


def wall(x, y):
    return 1.0 + 0.07 * np.sin(2.6 * x) + 0.05 * np.cos(3.1 * y + 0.4 * x) + 0.04 * np.sin(7.0 * x + 1.0)


def wall_frames(n_out, step, K, W, H):
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    a = (u - K[0, 2]) / K[0, 0]; b = (v - K[1, 2]) / K[1, 1]
    xs = [k * step for k in range(n_out + 1)]; xs = xs + xs[-2::-1]
    out = []
    for x0 in xs:
        z = np.ones_like(a)
        for _ in range(30):
            z = wall(x0 + a * z, b * z)
        out.append(z.astype(f32))
    return np.stack(out), xs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out-steps", type=int, default=24)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = tum.TUM_WIDTH, tum.TUM_HEIGHT
    K = np.asarray(tum.TUM_K, np.float64)
    cam = binding.depth_camera(K, W, H)
    lib = binding.load_library()
    out = dict(width=W, height=H, reps=a.reps)

    # ---- room ----
    T = [synth.camera_pose(k) for k in range(6)]
    depth = np.stack([synth.depth_frame(Tk, K, W, H, 0x7A11 + k, 0.05)[0][:, 2].reshape(H, W).copy() for k, Tk in enumerate(T)])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(f32) for Tk in T]
    s = EXTENT / 256
    opt = dict(origin=tuple(o + s / 2 for o in ORIGIN), voxel_size=s, truncation=5 * s)
    h = binding.Context(0)
    h.tsdf_create_hashed(block_capacity=1 << 15, **opt)
    for k in range(4):
        h.tsdf_integrate(depth[k], cam, gt[k])
    n_room = h.tsdf_blocks()[0]["n_blocks"]
    centre = np.ascontiguousarray(gt[2][:3, 3], f32)
    d2 = np.ascontiguousarray(depth[2], f32); p2 = binding.pose_to_c(gt[2])
    one = binding.sdf_options(stride=1, n_iterations=20, stop_rotation=0.0, stop_translation=0.0)
    # the radius at which a few hundred blocks leave: the 300 farthest block centres
    coords = h.tsdf_blocks()[1]
    dist = np.sort(np.linalg.norm(np.asarray(opt["origin"]) + (8.0 * coords + 3.5) * s - centre, axis=1))
    r_some = float(0.5 * (dist[-301] + dist[-300])) if len(dist) > 600 else float(dist[len(dist) // 2])
    room = dict(evict_none_ms=[], pair_ms=[], touch_ms=[], integrate_ms=[], evict_some_ms=[], insert_some_ms=[], tracked_frame_wall_ms=[])
    info = binding.IcpTsdfStreamInfo()
    n_some = 0
    for rep in range(a.reps + 1):                       # the first round warms up
        ms, t_ms, i_ms = C.c_float(0), C.c_float(0), C.c_float(0)
        h._ck(lib.icp_debug_htsdf_evict_time(h.h, binding._ptr(centre), C.c_float(1e6), 1, C.byref(info), C.byref(ms))); none = ms.value
        assert info.n_evicted == 0
        h._ck(lib.icp_debug_sdf_time(h.h, binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(one), C.byref(ms))); pair = ms.value
        h._ck(lib.icp_debug_htsdf_time(h.h, binding._ptr(d2), C.byref(cam), binding._ptr(p2), C.byref(t_ms), C.byref(i_ms)))
        h._ck(lib.icp_debug_htsdf_evict_time(h.h, binding._ptr(centre), C.c_float(r_some), 1, C.byref(info), C.byref(ms))); some = ms.value
        n_some = info.n_evicted
        ec = np.empty((n_some, 3), np.int32); et = np.empty((n_some, 8, 8, 8), f32); ew = np.empty((n_some, 8, 8, 8), f32)
        h._ck(lib.icp_tsdf_evicted_blocks(h.h, n_some, binding._ptr(ec), binding._ptr(et), binding._ptr(ew)))
        h._ck(lib.icp_debug_htsdf_insert_time(h.h, n_some, binding._ptr(ec), binding._ptr(et), binding._ptr(ew), C.byref(info), C.byref(ms))); ins = ms.value
        assert info.n_blocks == n_room
        t = binding.Context(0)
        t.tsdf_create_hashed(block_capacity=1 << 15, **opt)
        t0 = time.perf_counter()
        t.track_depth_sdf(depth, cam, stride=1, n_iterations=20)
        wall_ms = (time.perf_counter() - t0) * 1e3 / len(depth)
        t.close()
        if rep:
            for k, v in zip(room, (none, pair, t_ms.value, i_ms.value, some, ins, wall_ms)):
                room[k].append(v)
    out["room"] = dict(n_blocks=n_room, n_evicted_some=n_some, radius_some=r_some, **{k: stats(v) for k, v in room.items()})
    frame_ms = 20 * out["room"]["pair_ms"]["median"] + out["room"]["touch_ms"]["median"] + out["room"]["integrate_ms"]["median"]
    out["room"]["tracked_frame_device_ms"] = frame_ms
    out["room"]["evict_none_share_of_frame"] = out["room"]["evict_none_ms"]["median"] / frame_ms
    h.close()

    # ---- wall ----
    step = 0.25
    frames, xs = wall_frames(a.out_steps, step, K, W, H)
    vol = dict(origin=(0.0125, -0.0375, 0.6125), voxel_size=0.025, truncation=0.1, max_depth=1.3, min_depth=0.2)
    keep = binding.tsdf_view_reach(cam, vol) + 2 * step
    sdf = dict(stride=2, n_iterations=15)
    wl = dict(unbounded_frame_ms=[], local_frame_ms=[], unbounded_integrate_ms=[], local_integrate_ms=[])
    last = np.ascontiguousarray(frames[-1], f32)
    for rep in range(min(a.reps, 3) + 1):
        u, l = binding.Context(0), binding.Context(0)
        for c in (u, l):
            c.tsdf_create_hashed(block_capacity=1 << 12, **vol)
        t0 = time.perf_counter(); upose, urecs, _ = u.track_depth_sdf(frames, cam, **sdf); tu = (time.perf_counter() - t0) * 1e3 / len(frames)
        t0 = time.perf_counter(); lpose, lrecs, _, evs, store = tsdf_local.track_depth_sdf_local(l, frames, cam, keep, **sdf); tl = (time.perf_counter() - t0) * 1e3 / len(frames)
        same = bool(np.array_equal(upose.view(np.uint32), lpose.view(np.uint32)))
        nu, nl = u.tsdf_blocks()[0]["n_blocks"], l.tsdf_blocks()[0]["n_blocks"]
        t_ms, iu, il = C.c_float(0), C.c_float(0), C.c_float(0)
        pl = binding.pose_to_c(upose)
        u._ck(lib.icp_debug_htsdf_time(u.h, binding._ptr(last), C.byref(cam), binding._ptr(pl), C.byref(t_ms), C.byref(iu)))
        l._ck(lib.icp_debug_htsdf_time(l.h, binding._ptr(last), C.byref(cam), binding._ptr(pl), C.byref(t_ms), C.byref(il)))
        if rep:
            for k, v in zip(wl, (tu, tl, iu.value, il.value)):
                wl[k].append(v)
        out["wall"] = dict(frames=len(frames), out_steps=a.out_steps, step=step, keep_radius=keep, voxel_size=vol["voxel_size"], blocks_unbounded=nu, blocks_local=nl,
                           blocks_stored=len(store), peak_local=max(e["n_resident"] + e["n_evicted"] for e in evs), poses_bit_identical=same,
                           frames_with_eviction=sum(1 for e in evs if e["n_evicted"]), frames_with_insertion=sum(1 for e in evs if e["n_inserted"]))
        u.close(); l.close()
    out["wall"].update({k: stats(v) for k, v in wl.items()})
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
