"""The voxel map contract of include/icp_hip.h (icp_voxel_map_create / insert / upload, icp_get_voxel_map, icp_voxel_map_system / align,
icp_track_scans_vmap) restated in numpy.  Written from the contract alone; whatever the map shares with voxelized GICP's grid -- the cell
rule, the quantisation, the record, the transforms, the sums of a step, the step and the stop -- is vgicp_restatement's, reused here.  The
integer state is numpy int64, the records are compared with the device bit for bit.  Contains no device code."""
import numpy as np

import vgicp_restatement as VR

f32, f64 = np.float32, np.float64
OK = VR.OK
MAX_CELLS = VR.MAX_CELLS
INFO = ("n_considered", "n_entered", "n_outside", "n_cells_touched", "n_cells_new", "n_occupied")


class BadOptions(ValueError):
    pass


def extent(lower, upper, voxel_size):
    """(lo, dims) of the box lower .. upper by the cell rule."""
    lo = VR.cell_coords(np.asarray(lower, f32)[None], voxel_size)[0]
    hi = VR.cell_coords(np.asarray(upper, f32)[None], voxel_size)[0]
    return lo, hi - lo + 1


def create(voxel_size, lo, dims):
    """icp_voxel_map_create: the map as vgicp_restatement.grid's dict (lo, dims, counts int32, sums int64, cells fp32, n_occupied,
    voxel_size), all zero."""
    vs = f32(voxel_size)
    lo = np.asarray(lo, np.int64); dims = np.asarray(dims, np.int64)
    if not (np.isfinite(vs) and vs > 0):
        raise BadOptions("voxel_size must be finite and > 0")
    if (dims < 1).any() or int(dims[0]) * int(dims[1]) * int(dims[2]) > MAX_CELLS:
        raise BadOptions("dims must be >= 1 with a product of at most 2^24")
    n = int(dims[0] * dims[1] * dims[2])
    return dict(lo=lo, dims=dims, counts=np.zeros(n, np.int32), sums=np.zeros((n, 9), np.int64), cells=np.zeros((n, 9), f32), n_occupied=0, voxel_size=vs)


def records(m, which=None):
    """The records of the cells `which` (every cell by default) from their sums and counts: vgicp_restatement.grid's arithmetic."""
    idx = np.arange(len(m["counts"])) if which is None else np.asarray(which, np.int64)
    dims, lo = m["dims"], m["lo"]
    cnt = m["counts"][idx].astype(np.int64)
    rec = np.zeros((len(idx), 9), f32)
    o = np.nonzero(cnt > 0)[0]
    occ = idx[o]
    cc = np.stack([occ % dims[0] + lo[0], (occ // dims[0]) % dims[1] + lo[1], occ // (dims[0] * dims[1]) + lo[2]], 1)
    v = f64(m["voxel_size"])
    s = m["sums"][occ]
    mu = (cc.astype(f64) + 0.5) * v + (s[:, :3].astype(f64) / cnt[o].astype(f64)[:, None]) * (v / 65536.0)
    rec[o, :3] = mu.astype(f32)
    tr = (s[:, 3] + s[:, 6]) + s[:, 8]
    has = tr > 0
    S = np.zeros((len(occ), 6), f64)
    S[has] = s[has, 3:].astype(f64) / tr[has].astype(f64)[:, None]
    rec[o, 3:] = S.astype(f32)
    m["cells"][idx] = rec


def insert(m, points, normals, pose):
    """icp_voxel_map_insert of a cloud with its GICP normals at `pose`, in place.  Returns icp_voxel_map_insert_info as a dict."""
    p = np.asarray(points, f32); n = np.asarray(normals, f32)
    considered = np.isfinite(p).all(1)
    pt = VR.transform_points(pose, p); nt = VR.transform_normals(pose, n)
    enters = considered & np.isfinite(pt).all(1) & np.isfinite(nt).all(1)
    c, q, mm = VR.quantise(pt[enters], nt[enters], m["voxel_size"])
    rel = c - m["lo"]
    inside = ((rel >= 0) & (rel < m["dims"])).all(1)
    idx = ((rel[:, 2] * m["dims"][1] + rel[:, 1]) * m["dims"][0] + rel[:, 0])[inside]
    before = m["counts"].copy()
    counts = m["counts"].astype(np.int64)
    np.add.at(counts, idx, 1)
    np.add.at(m["sums"], idx, np.concatenate([q, mm], 1)[inside])
    m["counts"] = counts.astype(np.int32)
    touched = np.unique(idx)
    records(m, touched)
    new = int((before[touched] == 0).sum())
    m["n_occupied"] += new
    return dict(n_considered=int(considered.sum()), n_entered=int(enters.sum()), n_outside=int((~inside).sum()), n_cells_touched=int(len(touched)),
                n_cells_new=new, n_occupied=int(m["n_occupied"]))


def upload(m, counts, sums):
    """icp_voxel_map_upload: the integer state replaced, every record recomputed."""
    m["counts"] = np.asarray(counts, np.int32).reshape(-1).copy(); m["sums"] = np.asarray(sums, np.int64).reshape(-1, 9).copy()
    m["cells"] = np.zeros((len(m["counts"]), 9), f32)
    records(m)
    m["n_occupied"] = int((m["counts"] > 0).sum())


def system(m, src, src_normals, pose, eps, min_points=1, **_):
    """icp_voxel_map_system: vgicp_restatement.system with the map as the grid."""
    return VR.system(m, src, src_normals, pose, eps, min_points)


def align(m, src, src_normals, pose, eps, **kw):
    """icp_voxel_map_align: vgicp_restatement.align with the map as the grid."""
    return VR.align(m, src, src_normals, pose, eps, **kw)


def track(m, scans, pose, eps, **kw):
    """icp_track_scans_vmap over [(xyz, normals)]: (poses: one per scan, records of scans 1 .., first error)."""
    cur = np.asarray(pose, f32).copy()
    insert(m, scans[0][0], scans[0][1], cur)
    poses, recs, first = [cur.copy()], [], OK
    for xyz, nrm in scans[1:]:
        cur, rec, _ = align(m, xyz, nrm, cur, eps, **kw)
        recs.append(rec); poses.append(cur.copy())
        if rec["status"] == OK:
            insert(m, xyz, nrm, cur)
        elif first == OK:
            first = rec["status"]
    return poses, recs, first
