"""Times the voxel map of scan-to-map laser tracking on 370 488-point scans, with tools/time_vgicp.py's method: every
figure the median of --reps repeats after one warm-up, the candidates interleaved inside each repeat.
  * insert: the device time of ONE icp_voxel_map_insert of synth.eth_like_pair(0)'s target at the identity into a map over the room (both
    kernels and the clear of the counters between two events: icp_debug_vmap_time), and of k_vmap_records alone;
  * build: the device time of an icp_voxelize_target build of the same cloud from a dropped grid (icp_debug_vgicp_time);
  * track: wall time per scan of icp_track_scans_vmap over --scans scans of the outcome fixture's path at full size, uploads included;
  * pairs: wall time per pair of icp_set_target + icp_set_source + icp_vgicp_align over the same scans, from the identity.
All with the clouds' own normals (covariance_k = 0), epsilon 1e-3, voxel 0.25 m, 30 iterations and the default stops.
A library without the voxel map (ICP_HIP_LIB=<the parent commit's build>) reports build and pairs alone: run the tool once per library,
alternating, to compare commits.
usage: python tools/time_vmap.py [--reps 5] [--scans 6] [--json out.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = binding.load_library()
    has_map = hasattr(lib, "icp_voxel_map_insert")
    eye = np.eye(4, dtype=np.float32)
    d = synth.eth_like_pair(0)
    tp, tn = d["tgt_pts"], d["tgt_nrm"]
    scans = MF.scans(a.scans, (344, 1077))
    lo, dims = [tuple(int(v) for v in x) for x in MF.extent()]
    opt = binding.vgicp_options(voxel_size=MF.VOXEL)
    one = binding.Context(0)                       # the single cloud: insert against build
    one.set_gicp_options(MF.EPSILON, 0)
    one.set_target(tp, tn); one.set_source(tp, tn)
    seq = binding.Context(0)                       # the sequence: track against pairs
    seq.set_gicp_options(MF.EPSILON, 0)
    row = dict(library=binding.LIB_PATH, has_map=has_map, n_points=int(len(tp)), n_scans=a.scans, reps=a.reps, dims=dims)
    samples = {}

    def build_ms():
        it, build, index = C.c_float(0), C.c_float(0), C.c_float(0)
        one._ck(lib.icp_debug_vgicp_time(one.h, binding._ptr(binding.pose_to_c(eye)), C.byref(opt), C.byref(it), C.byref(build), C.byref(index)))
        return build.value

    def insert_ms():
        one.voxel_map_create(MF.VOXEL, lo, dims)
        ins, rec = C.c_float(0), C.c_float(0)
        one._ck(lib.icp_debug_vmap_time(one.h, 0, binding._ptr(binding.pose_to_c(eye)), C.byref(ins), C.byref(rec)))
        return ins.value, rec.value

    def track():
        seq.voxel_map_create(MF.VOXEL, lo, dims)
        t0 = time.perf_counter()
        pose, recs, rc = seq.track_scans_vmap(scans, MF.truth(0), options=opt)
        return (time.perf_counter() - t0) * 1e3 / (len(scans) - 1), recs, rc

    def pairs():
        t0 = time.perf_counter()
        its = []
        for k in range(1, len(scans)):
            seq.set_target(*scans[k - 1]); seq.set_source(*scans[k])
            pose, rec, rc = seq.vgicp_align(eye, options=opt)
            its.append(rec["iterations"])
        return (time.perf_counter() - t0) * 1e3 / (len(scans) - 1), its

    for rep in range(a.reps + 1):                  # (repeat 0 warms up: code objects, allocations, page-locked blocks)
        cur = {"build_ms": build_ms()}
        if has_map:
            cur["insert_ms"], cur["records_ms"] = insert_ms()
            cur["track_ms_per_scan"], recs, rc = track()
            row["track_status"] = rc; row["track_iterations"] = [r["iterations"] for r in recs]
        cur["pair_ms_per_pair"], row["pair_iterations"] = pairs()
        if rep:
            for k, v in cur.items():
                samples.setdefault(k, []).append(v)
    for k, xs in samples.items():
        row[k] = statistics.median(xs); row[k + "_min"] = min(xs); row[k + "_max"] = max(xs)
    if has_map:
        row["records_share"] = row["records_ms"] / row["insert_ms"]
        row["track_scans_per_s"] = 1e3 / row["track_ms_per_scan"]
        info = one.voxel_map()[0]
        row["n_occupied"] = info["n_occupied"]
    row["pairs_per_s"] = 1e3 / row["pair_ms_per_pair"]
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    one.close(); seq.close()


if __name__ == "__main__":
    main()
