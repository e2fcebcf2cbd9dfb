"""The voxelized GICP contract of include/icp_hip.h (icp_voxelize_target, icp_get_voxel_grid, icp_vgicp_system, icp_vgicp_align) restated in
numpy.  Written from the contract alone: every fp32 operation is one numpy float32 operation in the order the contract writes it, the
integer sums are numpy int64, everything after a conversion to fp64 is numpy float64.  The grid is compared with the device exactly (the
records bit for bit); `system` returns, next to every sum, the sum of the absolute values of its terms, which bounds what another summation
order may change.  Step, composition and stop are direct SDF tracking's (sdf_restatement), as the contract says.  Contains no device code."""
import numpy as np

import sdf_restatement as SR

f32, f64 = np.float32, np.float64
OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = SR.OK, SR.ERR_NO_SOURCE, SR.ERR_NO_CORRESPONDENCES
DEFAULTS = dict(voxel_size=0.25, min_points=1, n_iterations=30, min_valid=64, stop_rotation=1e-5, stop_translation=1e-5)
CLAMP = f32(2.0 ** 30)
MAX_CELLS = 1 << 24
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError("icp_vgicp_options has no field %r" % k)
        o[k] = v
    return o


def cell_coords(p, voxel_size):
    """(n, 3) int64 cell coordinates of finite fp32 points: (int)clamp(floorf(p / voxel_size), -2^30, 2^30)."""
    vs = f32(voxel_size)
    with np.errstate(all="ignore"):
        c = np.floor(np.asarray(p, f32) / vs).astype(f32)
    return np.minimum(np.maximum(c, -CLAMP), CLAMP).astype(np.int64)


def entering(points, normals):
    return np.isfinite(np.asarray(points, f32)).all(1) & np.isfinite(np.asarray(normals, f32)).all(1)


def quantise(points, normals, voxel_size):
    """Per entering point (the caller has filtered): cell coordinates (n, 3), q (n, 3) and the six products m_a m_b (n, 6), all int64."""
    vs = f32(voxel_size)
    p = np.asarray(points, f32); nr = np.asarray(normals, f32)
    c = cell_coords(p, vs)
    with np.errstate(all="ignore"):
        off = ((p - (c.astype(f32) + f32(0.5)) * vs) / vs) * f32(65536.0)
        q = np.rint(np.minimum(np.maximum(off, f32(-32768.0)), f32(32768.0))).astype(np.int64)
        m = np.rint(np.minimum(np.maximum(nr, f32(-2.0)), f32(2.0)) * f32(16384.0)).astype(np.int64)
    mm = np.stack([m[:, a] * m[:, b] for a, b in PAIRS], 1)
    return c, q, mm


class GridTooLarge(ValueError):
    pass


class NoTarget(ValueError):
    pass


def grid(points, normals, voxel_size):
    """icp_voxelize_target + icp_get_voxel_grid: dict(lo (3,), dims (3,), counts (n_cells,) int32, sums (n_cells, 9) int64, cells
    (n_cells, 9) float32, n_occupied, n_points, voxel_size)."""
    vs = f32(voxel_size)
    ok = entering(points, normals)
    if not ok.any():
        raise NoTarget("no entering point")
    c, q, mm = quantise(np.asarray(points, f32)[ok], np.asarray(normals, f32)[ok], vs)
    lo = c.min(0); dims = c.max(0) - lo + 1
    if int(dims[0]) * int(dims[1]) * int(dims[2]) > MAX_CELLS:
        raise GridTooLarge("voxel_size %g: more than 2^24 cells" % float(vs))
    n_cells = int(dims[0] * dims[1] * dims[2])
    idx = ((c[:, 2] - lo[2]) * dims[1] + (c[:, 1] - lo[1])) * dims[0] + (c[:, 0] - lo[0])
    counts = np.zeros(n_cells, np.int64); sums = np.zeros((n_cells, 9), np.int64)
    np.add.at(counts, idx, 1)
    np.add.at(sums, idx, np.concatenate([q, mm], 1))
    cells = np.zeros((n_cells, 9), f32)
    occ = np.nonzero(counts > 0)[0]
    cz = occ // (dims[0] * dims[1]); cy = (occ // dims[0]) % dims[1]; cx = occ % dims[0]
    cc = np.stack([cx + lo[0], cy + lo[1], cz + lo[2]], 1)
    v = f64(vs)
    mu = (cc.astype(f64) + 0.5) * v + (sums[occ, :3].astype(f64) / counts[occ].astype(f64)[:, None]) * (v / 65536.0)
    cells[occ, :3] = mu.astype(f32)
    tr = (sums[occ, 3] + sums[occ, 6]) + sums[occ, 8]
    has = tr > 0
    S = np.zeros((len(occ), 6), f64)
    S[has] = sums[occ[has], 3:].astype(f64) / tr[has].astype(f64)[:, None]
    cells[occ, 3:] = S.astype(f32)
    return dict(lo=lo, dims=dims, counts=counts.astype(np.int32), sums=sums, cells=cells, n_occupied=int(len(occ)), n_points=int(ok.sum()),
                voxel_size=vs)


def transform_points(pose, pts):
    """icp_transform_points in fp32: ((P_r0 x + P_r1 y) + P_r2 z) + P_r3."""
    P = np.asarray(pose, f32); x = np.asarray(pts, f32)
    with np.errstate(all="ignore"):
        return np.stack([((P[r, 0] * x[:, 0] + P[r, 1] * x[:, 1]) + P[r, 2] * x[:, 2]) + P[r, 3] for r in range(3)], 1).astype(f32)


def normal_matrix(pose):
    """(R^-1)^T of the pose's rotation block: fp64 cofactors over the fp64 determinant, each entry rounded once to fp32."""
    R = np.asarray(pose, f32)[:3, :3].astype(f64)
    a, b, c = R[0]; d, e, f = R[1]; g, h, i = R[2]
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = (a * c00 + b * c01) + c * c02
    cof = np.array([[c00, c01, c02], [c * h - b * i, a * i - c * g, b * g - a * h], [b * f - c * e, c * d - a * f, a * e - b * d]], f64)
    with np.errstate(all="ignore"):
        return (cof / det).astype(f32)


def transform_normals(pose, nrm):
    """icp_transform_normals in fp32: (N_r0 x + N_r1 y) + N_r2 z with N the normal matrix."""
    N = normal_matrix(pose); x = np.asarray(nrm, f32)
    with np.errstate(all="ignore"):
        return np.stack([(N[r, 0] * x[:, 0] + N[r, 1] * x[:, 1]) + N[r, 2] * x[:, 2] for r in range(3)], 1).astype(f32)


def point_terms(g, src, src_normals, pose, eps, min_points=1):
    """Every source point at `pose`: dict of considered (n,), valid (n,), and for the valid points p (fp32), r, M, N (fp64) and the cell index."""
    s = np.asarray(src, f32)
    considered = np.isfinite(s).all(1)
    p = transform_points(pose, s)
    b32 = transform_normals(pose, src_normals)
    pfin = considered & np.isfinite(p).all(1)
    c = np.zeros((len(s), 3), np.int64)
    c[pfin] = cell_coords(p[pfin], g["voxel_size"])
    rel = c - g["lo"]
    inside = pfin & ((rel >= 0) & (rel < g["dims"])).all(1)
    idx = np.where(inside, (rel[:, 2] * g["dims"][1] + rel[:, 1]) * g["dims"][0] + rel[:, 0], 0)
    cnt = np.where(inside, g["counts"][idx], 0)
    with np.errstate(all="ignore"):
        b = b32.astype(f64)
        ln = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
        bok = np.isfinite(b32).all(1) & (ln > 0)
    valid = inside & (cnt >= int(min_points)) & bok
    v = np.nonzero(valid)[0]
    b = b[v] / ln[v, None]
    rec = g["cells"][idx[v]].astype(f64)
    P = p[v].astype(f64)
    r = rec[:, :3] - P
    ome = 1.0 - f64(f32(eps))
    Sg = np.empty((len(v), 3, 3), f64)
    for k, (i, j) in enumerate(PAIRS):
        t = ome * (rec[:, 3 + k] + b[:, i] * b[:, j])
        Sg[:, i, j] = Sg[:, j, i] = (2.0 - t) if i == j else -t
    S00, S01, S02, S11, S12, S22 = Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]
    c00 = S11 * S22 - S12 * S12; c01 = S02 * S12 - S01 * S22; c02 = S01 * S12 - S02 * S11
    c11 = S00 * S22 - S02 * S02; c12 = S01 * S02 - S00 * S12; c22 = S00 * S11 - S01 * S01
    det = (S00 * c00 + S01 * c01) + S02 * c02
    M = np.empty_like(Sg)
    for (i, j), cf in zip(PAIRS, (c00, c01, c02, c11, c12, c22)):
        M[:, i, j] = M[:, j, i] = cf / det
    return dict(considered=considered, valid=valid, index=v, p=p[v], r=r, Sigma=Sg, M=M, N=cnt[v].astype(f64), cell=idx[v])


def jacobian(p):
    """J = [-[p]x | I] in fp64, (n, 3, 6)."""
    q = np.asarray(p).astype(f64)
    z = np.zeros(len(q))
    A = np.stack([np.stack([z, q[:, 2], -q[:, 1]], 1), np.stack([-q[:, 2], z, q[:, 0]], 1), np.stack([q[:, 1], -q[:, 0], z], 1)], 1)
    return np.concatenate([A, np.broadcast_to(np.eye(3), (len(q), 3, 3))], 2)


def system(g, src, src_normals, pose, eps, min_points=1, **_):
    """icp_vgicp_system: ((considered, valid), sums (28,) fp64, sum of |term| per sum (28,))."""
    t = point_terms(g, src, src_normals, pose, eps, min_points)
    J = jacobian(t["p"]); M = t["M"]; r = t["r"]; N = t["N"]
    MJ = np.einsum("nab,nbj->naj", M, J)
    H = np.einsum("nai,naj->nij", J, MJ)
    Mr = np.einsum("nab,nb->na", M, r)
    gv = np.einsum("nai,na->ni", J, Mr)
    terms = np.empty((28, len(N)), f64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            terms[k] = N * H[:, i, j]; k += 1
    for i in range(6):
        terms[21 + i] = N * gv[:, i]
    terms[27] = N * np.einsum("na,na->n", r, Mr)
    return (int(t["considered"].sum()), int(t["valid"].sum())), terms.sum(1), np.abs(terms).sum(1)


step = SR.step
stopped = SR.stopped


def align(g, src, src_normals, pose, eps, **kw):
    """icp_vgicp_align: (pose, record, trace).  A failed alignment carries the pose it started with."""
    o = options(**{k: v for k, v in kw.items() if k in DEFAULTS})
    start = np.asarray(pose, f32).copy(); cur = start.copy()
    rec = dict(n_depth=0, n_valid_first=0, n_valid_last=0, iterations=0, status=OK, cost_first=0.0, cost_last=0.0)
    trace = []
    for it in range(o["n_iterations"]):
        counts, sums, _ = system(g, src, src_normals, cur, eps, o["min_points"])
        if it == 0:
            rec.update(n_depth=counts[0], n_valid_first=counts[1], cost_first=float(sums[27]))
        rec.update(n_valid_last=counts[1], cost_last=float(sums[27]), iterations=it + 1)
        new, x = (None, None) if counts[0] == 0 else step(sums, counts, cur, min_valid=o["min_valid"])
        if new is None:
            rec["status"] = ERR_NO_SOURCE if counts[0] == 0 else ERR_NO_CORRESPONDENCES
            trace.append(dict(n_valid=counts[1], status=rec["status"], cost=float(sums[27]), pose=cur.copy()))
            cur = start.copy()
            break
        cur = new
        trace.append(dict(n_valid=counts[1], status=OK, cost=float(sums[27]), pose=cur.copy()))
        if stopped(x, stop_rotation=o["stop_rotation"], stop_translation=o["stop_translation"]):
            break
    rec["pose"] = cur.copy()
    return cur, rec, trace
