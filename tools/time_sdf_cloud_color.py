"""A coloured laser scan aligned to the coloured TSDF volume on the clock (icp_tsdf_align_cloud_color, icp_track_scans_sdf_photometric;
DESIGN.md section 6zj): tools/time_sdf_cloud.py's synthetic scans of 370 488 points (344 x 1077 beams, 1 cm range noise) in their sensor
frames, coloured by three smooth sinusoids of the world point, 5 cm voxels, truncation 0.4 m, dense and hashed.
  * pair: the device time of ONE coloured accumulate + k_sdf_solve_color pair between events (icp_debug_sdf_cloud_color_time) of scan 1 at
    its true pose against the coloured model scan 0 has left; beside it, in the same repeat and on the same model, the geometric pair
    (icp_debug_sdf_cloud_time).  The depth form's ratio of the two is 1.12 to 1.17 (README); the cloud's is printed as *_pair_ratio;
  * tracked scan: the host's wall time of the photometric loop over --scans scans minus that over scan 0 alone, per tracked scan; beside
    it the same difference of icp_track_scans_sdf_color (the same uploads and coloured fuses, the geometric alignment).
Every figure is the median of --reps repeats after one warm-up, the candidates interleaved inside each repeat, with the least and the
largest sample beside it.  ICP_HIP_LIB selects the library, so the same script times a build of the parent commit (whose library lacks the
coloured calls: the coloured figures are then left out).  Reads nothing but icp_amd.synth.
usage: python tools/time_sdf_cloud_color.py [--reps 7] [--scans 3] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding, synth

N_TILT, N_BEAM = 344, 1077
VOXEL, WEIGHT = 0.05, 0.1
TSDF = dict(voxel_size=VOXEL, truncation=0.4, max_depth=30.0)
DENSE = dict(dims=(140, 180, 72), origin=(-3.5, -4.5, -0.5))       # synth's room, half a metre of margin


def create(ctx, hashed):
    if hashed:
        ctx.tsdf_create_hashed(block_capacity=1 << 14, origin=(0.0, 0.0, 0.0), color=True, **TSDF)
    else:
        ctx.tsdf_create(color=True, **DENSE, **TSDF)


def texture(w):
    """rgba (n, 4) uint8 of world points: three sinusoids of wavelengths 0.7 .. 1.1 m."""
    x, y, z = w[:, 0].astype(np.float64), w[:, 1].astype(np.float64), w[:, 2].astype(np.float64)
    r = 128 + 70 * np.sin(2 * np.pi * (x + 0.4 * y + 0.2 * z) / 0.7)
    g = 125 + 60 * np.cos(2 * np.pi * (0.8 * x - 0.5 * y + 0.3 * z) / 0.9 + 0.5)
    b = 120 + 50 * np.sin(2 * np.pi * (0.6 * x + 0.9 * y - 0.4 * z) / 1.1 + 1.3)
    rgb = np.clip(np.rint(np.stack([r, g, b], 1)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, np.full((len(w), 1), 255, np.uint8)], 1))


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scans", type=int, default=3)
    ap.add_argument("--n-tilt", type=int, default=N_TILT)
    ap.add_argument("--n-beam", type=int, default=N_BEAM)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    colored = hasattr(lib, "icp_debug_sdf_cloud_color_time")
    scans, cols, poses = [], [], []
    for k in range(a.scans):
        T = synth.scan_pose(k)
        world, nrm, _ = synth.laser_scan(T, 0xE7A0 + k, a.n_tilt, a.n_beam)
        pts, nrm = synth.apply_pose(np.linalg.inv(T), world, nrm)
        scans.append(np.ascontiguousarray(pts, np.float32)); cols.append(texture(np.asarray(world))); poses.append(T.astype(np.float32))
    ctx = binding.Context(0)
    ctx.set_stage_timing(0)
    so = binding.sdf_options(n_iterations=30)
    co = binding.sdf_color_options(weight=WEIGHT)
    row = dict(library=binding.LIB_PATH, colored=colored, n_points=int(len(scans[0])), n_scans=a.scans, reps=a.reps, voxel=VOXEL, weight=WEIGHT)
    samples = {}
    for rep in range(a.reps + 1):                  # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        cur = {}
        for hashed in (False, True):
            tag = "hashed_" if hashed else "dense_"
            create(ctx, hashed)
            ctx.set_source(scans[0], None, cols[0])
            ctx.tsdf_integrate_cloud("source", pose=poses[0], color=True)
            ctx.set_source(scans[1], None, cols[1])
            p1 = binding.pose_to_c(poses[1])
            ms = C.c_float(0)
            ctx._ck(lib.icp_debug_sdf_cloud_time(ctx.h, 1, binding._ptr(p1), C.byref(so), C.byref(ms)))
            cur[tag + "geometric_pair_ms"] = ms.value
            if colored:
                ctx._ck(lib.icp_debug_sdf_cloud_color_time(ctx.h, 1, binding._ptr(p1), C.byref(so), C.byref(co), C.byref(ms)))
                cur[tag + "colored_pair_ms"] = ms.value
                cur[tag + "pair_ratio"] = cur[tag + "colored_pair_ms"] / cur[tag + "geometric_pair_ms"]
                if not rep:
                    sums, counts = ctx.tsdf_cloud_system("source", poses[1], color_weight=WEIGHT)
                    row[tag + "pair_counts"] = [int(c) for c in counts]
            # the loops: all scans, and scan 0 alone
            kinds = (("geometric", {}),) + ((("colored", dict(color_weight=WEIGHT)),) if colored else ())
            for kind, kw in kinds:
                create(ctx, hashed)
                t_all, out = wall(lambda: ctx.track_scans_sdf(scans, poses[0], colors=cols, n_iterations=30, **kw))
                create(ctx, hashed)
                t_one, _ = wall(lambda: ctx.track_scans_sdf(scans[:1], poses[0], colors=cols[:1], n_iterations=30, **kw))
                cur[tag + kind + "_tracked_scan_ms"] = (t_all - t_one) / (a.scans - 1)
                if not rep:
                    row[tag + kind + "_track"] = dict(status=out[3], iterations=[r["iterations"] for r in out[1]], n_valid_first=[r["n_valid_first"] for r in out[1]],
                                                      translation_error_m=[float(np.linalg.norm(P[:3, 3] - T[:3, 3])) for P, T in zip(out[0], poses)])
        if rep:
            for k, v in cur.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = statistics.median(xs); row[k + "_min"] = min(xs); row[k + "_max"] = max(xs)
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
