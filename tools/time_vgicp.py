"""Times voxelized GICP (icp_vgicp_align) against Generalized-ICP (params.metric = 3) and point-to-plane on the 370 488-point ETH-like pair
(synth.eth_like_pair(0), max distance 10), with tools/time_gicp.py's method: every figure the median of --reps repeats after one warm-up,
the candidates interleaved inside each repeat so that a drift of the clocks touches all of them alike.
  * device time per iteration: VGICP at each voxel size (one k_vgicp_accumulate + k_sdf_solve pair between two events), GICP (k = 20) and
    point-to-plane in the default merged loop (icp_get_timing total / iterations over 20 iterations from the identity, stage timing off);
  * grid build (event time of a build from a dropped grid, its two host reads included; the GICP normals cached) against the target's index
    build (the event bracket of the LBVH build behind icp_set_target);
  * pose error against gt: VGICP after 30 iterations with the stops off, GICP and point-to-plane after their 20.
Both VGICP and GICP use 20-neighbour GICP normals and epsilon 1e-3.
usage: python tools/time_vgicp.py [--reps 5] [--voxels 0.25,0.125] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "icp-variants_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
from icp_amd import binding, synth


def context(metric, md):
    c = binding.Context(0)
    p = c.params
    p.metric, p.matching, p.knn_backend, p.n_iterations, p.max_distance = metric, 0, 1, 20, md
    c.push_params()
    c.set_stage_timing(0)
    return c


def vgicp_times(c, pose, o):
    it, build, index = C.c_float(0), C.c_float(0), C.c_float(0)
    c._ck(c.lib.icp_debug_vgicp_time(c.h, binding._ptr(binding.pose_to_c(pose)), C.byref(o), C.byref(it), C.byref(build), C.byref(index)))
    return it.value, build.value, index.value


def main():
    from conftest import pose_error
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--voxels", default="0.25,0.125")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    voxels = [float(v) for v in a.voxels.split(",")]
    d = synth.eth_like_pair(0)
    sp, sn, tp, tn, gt = d["src_pts"], d["src_nrm"], d["tgt_pts"], d["tgt_nrm"], d["gt"]
    eye = np.eye(4, dtype=np.float32)
    ctx = {label: context(metric, 10.0) for label, metric in (("gicp", 3), ("p2plane", 1))}
    for c in ctx.values():
        c.set_target(tp, tn); c.set_source(sp, sn)
    ix = context(1, 10.0)
    ix.set_gicp_options(1e-3, 0)                                                        # (its grid reads the cloud's own normals: nothing else to compute)
    ix.set_target(tp, tn); ix.set_source(sp, sn)
    row = dict(n_src=int(len(sp)), n_tgt=int(len(tp)), reps=a.reps)
    poses = {label: c.run(eye, check=False)[0] for label, c in ctx.items()}            # warm-up: index, levels, GICP normals, allocations
    v = ctx["gicp"]                                                                     # VGICP on the GICP context: the same cached normals
    opts = {vs: binding.vgicp_options(voxel_size=vs, stop_rotation=0.0, stop_translation=0.0) for vs in voxels}
    for vs, o in opts.items():
        pose, rec, rc = v.vgicp_align(eye, options=o)                                   # warm-up, and the outcome
        ang, tr = pose_error(pose, gt)
        info = v.voxelize_target(o)
        row["vgicp_%g" % vs] = dict(status=rc, iterations=rec["iterations"], n_valid_first=rec["n_valid_first"], n_valid_last=rec["n_valid_last"],
                                    err_rad=ang, err_m=tr, dims=info["dims"], n_occupied=info["n_occupied"])
    samples = {}
    for _ in range(a.reps):
        for label, c in ctx.items():
            c.run(eye, check=False)
            t = c.timing()
            samples.setdefault(label + "_ms_per_it", []).append(t["total_ms"] / max(t["iterations"], 1))
        for vs, o in opts.items():
            it, build, index = vgicp_times(v, eye, o)
            samples.setdefault("vgicp_%g_ms_per_it" % vs, []).append(it)
            samples.setdefault("vgicp_%g_build_ms" % vs, []).append(build)
        ix.set_target(tp, tn)                                                           # a fresh index build, on a context of its own
        samples.setdefault("index_build_ms", []).append(vgicp_times(ix, eye, opts[voxels[0]])[2])
    for k, xs in samples.items():
        row[k] = statistics.median(xs)
    for label in ctx:
        ang, tr = pose_error(poses[label], gt)
        row[label + "_err_rad"], row[label + "_err_m"] = ang, tr
    ang, tr = pose_error(eye, gt)
    row["identity_err_rad"], row["identity_err_m"] = ang, tr
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    for c in list(ctx.values()) + [ix]:
        c.close()


if __name__ == "__main__":
    main()
