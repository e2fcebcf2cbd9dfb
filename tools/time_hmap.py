"""Times the hashed voxel map against the dense one on 370 488-point scans and the room of section 6t, with
tools/time_vmap.py's method: every figure the median of --reps repeats after one warm-up, the two storages interleaved inside each repeat,
in one process.  (The dense map's kernels are instruction for instruction the parent commit's: tools/dev_isa_compare.py.)
  * insert: the device time of ONE icp_voxel_map_insert of synth.eth_like_pair(0)'s target at the identity (both kernels and the clear of
    the counters between two events: icp_debug_vmap_time), and of the records kernel alone;
  * accumulate: the device time of one accumulate launch of that cloud against the map it was fused into, at a pose 2 cm off
    (k_vgicp_accumulate against k_hmap_accumulate: icp_debug_vmap_accumulate_time, the mean of 20 launches);
  * track: wall time per scan of icp_track_scans_vmap over --scans scans of the outcome fixture's path at full size, uploads included;
  * rehash: the device time of one rehash of the tracked map into a table of the same size (allocation and clearing included);
  * bytes: what the hashed map allocates against a dense map over the bounding box of the trajectory's cells.
All with the clouds' own normals (covariance_k = 0), epsilon 1e-3, voxel 0.25 m, 30 iterations and the default stops.
usage: python tools/time_hmap.py [--reps 5] [--scans 6] [--capacity 65536] [--json out.json]"""
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
from icp_amd import binding, synth
import vmap_outcome_fixture as MF

SLOT_BYTES = 8 + 4 + 72 + 40 + 4
CELL_BYTES = 4 + 72 + 40 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--capacity", type=int, default=1 << 16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    eye = np.eye(4, dtype=np.float32)
    near = synth.make_pose((0.004, -0.003, 0.005), (0.02, -0.015, 0.01)).astype(np.float32)
    d = synth.eth_like_pair(0)
    tp, tn = d["tgt_pts"], d["tgt_nrm"]
    scans = MF.scans(a.scans, (344, 1077))
    lo, dims = [tuple(int(v) for v in x) for x in MF.extent()]
    opt = binding.vgicp_options(voxel_size=MF.VOXEL)
    ctx = {}
    for kind in ("dense", "hashed"):
        ctx[kind] = (binding.Context(0), binding.Context(0))      # the single cloud; the sequence
        for c in ctx[kind]:
            c.set_gicp_options(MF.EPSILON, 0)
        ctx[kind][0].set_target(tp, tn); ctx[kind][0].set_source(tp, tn)
    row = dict(library=binding.LIB_PATH, n_points=int(len(tp)), n_scans=a.scans, reps=a.reps, dims=dims, capacity_asked=a.capacity)
    samples = {}

    def create(c, kind):
        if kind == "dense":
            c.voxel_map_create(MF.VOXEL, lo, dims)
        else:
            c.voxel_map_create_hashed(MF.VOXEL, a.capacity)

    def insert_ms(kind):
        one = ctx[kind][0]
        create(one, kind)
        ins, rec = C.c_float(0), C.c_float(0)
        one._ck(lib.icp_debug_vmap_time(one.h, 0, binding._ptr(binding.pose_to_c(eye)), C.byref(ins), C.byref(rec)))
        return ins.value, rec.value

    def accumulate_ms(kind):
        one = ctx[kind][0]
        ms = C.c_float(0)
        one._ck(lib.icp_debug_vmap_accumulate_time(one.h, binding._ptr(binding.pose_to_c(near)), C.byref(opt), 20, C.byref(ms)))
        return ms.value

    def track(kind):
        seq = ctx[kind][1]
        create(seq, kind)
        t0 = time.perf_counter()
        pose, recs, rc = seq.track_scans_vmap(scans, MF.truth(0), options=opt)
        return (time.perf_counter() - t0) * 1e3 / (len(scans) - 1), recs, rc

    def rehash_ms():
        seq = ctx["hashed"][1]
        ms = C.c_float(0)
        seq._ck(lib.icp_debug_hmap_rehash_time(seq.h, C.byref(ms)))
        return ms.value

    for rep in range(a.reps + 1):                  # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        cur = {}
        for kind in (("dense", "hashed") if rep % 2 else ("hashed", "dense")):
            cur[kind + "_insert_ms"], cur[kind + "_records_ms"] = insert_ms(kind)
            cur[kind + "_accumulate_ms"] = accumulate_ms(kind)
            cur[kind + "_track_ms_per_scan"], recs, rc = track(kind)
            row[kind + "_track_status"] = rc; row[kind + "_track_iterations"] = [r["iterations"] for r in recs]
        cur["rehash_ms"] = rehash_ms()
        if rep:
            for k, v in cur.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = statistics.median(xs); row[k + "_min"] = min(xs); row[k + "_max"] = max(xs)
    for k in ("insert_ms", "records_ms", "accumulate_ms", "track_ms_per_scan"):
        row["ratio_" + k] = row["hashed_" + k] / row["dense_" + k]
    info, coords, counts, sums, cells = ctx["hashed"][1].voxel_map_hashed()
    dinfo = ctx["dense"][1].voxel_map()[0]
    box = coords.max(0).astype(np.int64) - coords.min(0) + 1
    row.update(hashed_info=info, dense_n_occupied=dinfo["n_occupied"], trajectory_box=[int(v) for v in box], hashed_bytes=info["capacity"] * SLOT_BYTES,
               dense_box_bytes=int(box[0] * box[1] * box[2]) * CELL_BYTES, single_cloud_info=ctx["hashed"][0].voxel_map_hashed()[0])
    row["ratio_bytes"] = row["hashed_bytes"] / row["dense_box_bytes"]
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    for pair in ctx.values():
        for c in pair:
            c.close()


if __name__ == "__main__":
    main()
