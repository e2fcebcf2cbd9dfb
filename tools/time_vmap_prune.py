"""Times the local voxel map with tools/time_hmap.py's method and data: 370 488-point scans, voxel 0.25 m, the room
of section 6t; every figure the median of --reps repeats after one warm-up, the two storages interleaved inside each repeat, in one process.
  * prune: the device time of ONE icp_voxel_map_prune of the tracked map between two events (icp_debug_vmap_prune_time), with a radius
    that removes nothing (the sweep alone) -- the room's dense extent, the hashed table the room rule has grown, and two reference
    sizes: an empty dense box of 2^24 cells (the largest a dense map can be) and an empty hashed table of 2^20 slots;
  * compact: the device time of one compaction of the tracked hashed map into a table of the same size (allocation and clearing included),
    beside one rehash of it (icp_debug_hmap_rehash_time);
  * track: wall time per scan of icp_track_scans_vmap_local against icp_track_scans_vmap over --scans scans, uploads and the map's creation
    included, with --keep-radius (50 m: the sweep runs and nothing leaves, so both loops do the same alignments) and with --local-radius
    (cells leave).
usage: python tools/time_vmap_prune.py [--reps 5] [--scans 6] [--capacity 65536] [--keep-radius 50] [--local-radius 4] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding
import vmap_outcome_fixture as MF

ALL = 2e19                                          # r2 is infinite in fp32: nothing is removed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--capacity", type=int, default=1 << 16)
    ap.add_argument("--keep-radius", type=float, default=50.0)
    ap.add_argument("--local-radius", type=float, default=4.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    scans = MF.scans(a.scans, (344, 1077))
    lo, dims = [tuple(int(v) for v in x) for x in MF.extent()]
    opt = binding.vgicp_options(voxel_size=MF.VOXEL)
    centre = np.asarray(MF.truth(a.scans - 1), np.float32)[:3, 3].copy()
    ctx = {k: binding.Context(0) for k in ("dense", "hashed", "big_dense", "big_hashed")}
    for c in ctx.values():
        c.set_gicp_options(MF.EPSILON, 0)
    ctx["big_dense"].voxel_map_create(MF.VOXEL, (-128, -128, -128), (256, 256, 256))
    ctx["big_hashed"].voxel_map_create_hashed(MF.VOXEL, 1 << 20)
    row = dict(library=binding.LIB_PATH, n_points=int(len(scans[0][0])), n_scans=a.scans, reps=a.reps, dims=dims, capacity_asked=a.capacity,
               keep_radius=a.keep_radius, local_radius=a.local_radius)
    samples = {}

    def create(c, kind):
        if kind == "dense":
            c.voxel_map_create(MF.VOXEL, lo, dims)
        else:
            c.voxel_map_create_hashed(MF.VOXEL, a.capacity)

    def track(kind, radius):
        c = ctx[kind]
        create(c, kind)
        t0 = time.perf_counter()
        out = c.track_scans_vmap(scans, MF.truth(0), keep_radius=radius, options=opt)
        return (time.perf_counter() - t0) * 1e3 / (len(scans) - 1), out

    def prune_ms(kind):
        c = ctx[kind]
        ms = C.c_float(0)
        c._ck(lib.icp_debug_vmap_prune_time(c.h, binding._ptr(centre), C.c_float(ALL), C.byref(ms)))
        return ms.value

    def table_ms(name):
        c = ctx["hashed"]
        ms = C.c_float(0)
        c._ck(getattr(lib, name)(c.h, C.byref(ms)))
        return ms.value

    for rep in range(a.reps + 1):                  # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        cur = {}
        for kind in (("dense", "hashed") if rep % 2 else ("hashed", "dense")):
            for name, radius in ((("plain", None), ("keep", a.keep_radius), ("local", a.local_radius)) if rep % 2 else (("local", a.local_radius), ("keep", a.keep_radius), ("plain", None))):
                cur["%s_track_%s_ms_per_scan" % (kind, name)], out = track(kind, radius)
                row["%s_track_%s_status" % (kind, name)] = out[2]; row["%s_track_%s_iterations" % (kind, name)] = [r["iterations"] for r in out[1]]
                if radius is not None:
                    row["%s_track_%s_prunes" % (kind, name)] = [(p["n_removed"], p["n_occupied"], p["n_vacated"], p["capacity"], p["n_compacted"]) for p in out[3]]
            cur[kind + "_prune_ms"] = prune_ms(kind)
            cur["big_" + kind + "_prune_ms"] = prune_ms("big_" + kind)
        cur["rehash_ms"] = table_ms("icp_debug_hmap_rehash_time")
        cur["compact_ms"] = table_ms("icp_debug_hmap_compact_time")
        if rep:
            for k, v in cur.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = statistics.median(xs); row[k + "_min"] = min(xs); row[k + "_max"] = max(xs)
    for kind in ("dense", "hashed"):
        row["ratio_%s_keep_over_plain" % kind] = row[kind + "_track_keep_ms_per_scan"] / row[kind + "_track_plain_ms_per_scan"]
        row["ratio_%s_prune_over_plain_scan" % kind] = row[kind + "_prune_ms"] / row[kind + "_track_plain_ms_per_scan"]
    row["hashed_info"] = ctx["hashed"].voxel_map_hashed()[0]
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    for c in ctx.values():
        c.close()


if __name__ == "__main__":
    main()
