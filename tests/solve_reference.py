"""Plain fp64 numpy reference of the three linear solves, and the degenerate / ill-conditioned input families that go with it.

TEST INFRASTRUCTURE ONLY: numpy, no oracle and no device code.  Input of every solve: the compacted correspondence arrays
(s, d, target / source normals, w; all fp32) as oracle.compact returns them.  The fp32 rows are built exactly as the reference builds
them (point-to-plane ICPOptimizer.h:687-751, symmetric :800-853, Procrustes ProcrustesAligner.h:50-55), widened to fp64, and solved
with numpy.  Means follow the device contract: fp64 sums over the valid pairs, divided by n, rounded once to fp32, unweighted.

Classes (classify): from the REFERENCE's normalised spectrum only.
  W  every ratio >= 2e-4, or every kept ratio >= 2e-4 and every dropped one <= CUT / 2 with at least one kept ... see T
  I  smallest ratio in (2 CUT, 2e-4): nothing dropped, but the weak direction is not comparable as x; the cost is
  T  some ratio <= CUT / 2 (dropped), kept ones >= 2e-4
  a ratio inside [CUT / 2, 2 CUT] is an error: there the rank rule's outcome flips on rounding.
CUT = 6 eps_f32 = 7.15e-7 (JacobiSVD / FullPivLU threshold of a 6-column system, ICPOptimizer.h:757-758, :866-868).
"""
import numpy as np

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
CUT = 6.0 * EPS32
WELL = 2e-4
CUT3 = 3.0 * EPS32          # the same rule for the 3 x 3 Procrustes matrix (diagSize = 3)


# ------------------------------------------------------------------------------------------------ rows
def means_f32(s, d):
    n = len(s)
    return (s.astype(np.float64).sum(0) / n).astype(f32), (d.astype(np.float64).sum(0) / n).astype(f32)


def plane_rows(s, d, n, w, symmetric=False):
    """(4n x 6 fp32, 4n fp32): row order [plane rows | x rows | y rows | z rows] (the order does not matter to any result here).
    symmetric=True: s, d already centred, n = n_t + n_s (ICPOptimizer.h:806-815)."""
    s = np.asarray(s, f32); d = np.asarray(d, f32); n = np.asarray(n, f32); w = np.asarray(w, f32)
    if symmetric:
        sd = s + d; ds = d - s
        A0 = np.stack([sd[:, 1] * n[:, 2] - sd[:, 2] * n[:, 1], sd[:, 2] * n[:, 0] - sd[:, 0] * n[:, 2], sd[:, 0] * n[:, 1] - sd[:, 1] * n[:, 0],
                       n[:, 0], n[:, 1], n[:, 2]], 1)
        b0 = ds[:, 0] * n[:, 0] + (ds[:, 1] * n[:, 1] + ds[:, 2] * n[:, 2])
    else:
        A0 = np.stack([n[:, 2] * s[:, 1] - n[:, 1] * s[:, 2], n[:, 0] * s[:, 2] - n[:, 2] * s[:, 0], n[:, 1] * s[:, 0] - n[:, 0] * s[:, 1],
                       n[:, 0], n[:, 1], n[:, 2]], 1)
        b0 = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) - ((n[:, 0] * s[:, 0] + n[:, 1] * s[:, 1]) + n[:, 2] * s[:, 2])
    f0 = f32(1.0) * w; f1 = f32(0.1) * w
    z, o = np.zeros_like(w), np.ones_like(w)
    rows = [A0 * f0[:, None], np.stack([z, s[:, 2], -s[:, 1], o, z, z], 1) * f1[:, None],
            np.stack([-s[:, 2], z, s[:, 0], z, o, z], 1) * f1[:, None], np.stack([s[:, 1], -s[:, 0], z, z, z, o], 1) * f1[:, None]]
    rhs = [b0 * f0, (d[:, 0] - s[:, 0]) * f1, (d[:, 1] - s[:, 1]) * f1, (d[:, 2] - s[:, 2]) * f1]
    A = np.concatenate(rows); b = np.concatenate(rhs)
    assert A.dtype == f32 and b.dtype == f32
    return A, b


def compacted(orc, case, weighting):
    """The compacted correspondences of one case at its incoming pose, through the oracle's own stages (transform, exact k-NN, weights,
    compaction): (s, d, w, target normals, source normals), after asserting that the match is the one the case was built for."""
    P = case["pose"]
    q = orc.transform_points(case["src_pts"], P); qn = orc.transform_normals(case["src_nrm"], P)
    m, _ = orc.knn3(q, case["tgt_pts"], MAX_DISTANCE)
    assert np.array_equal(m["idx"], case["idx"]), case["name"]
    m = orc.apply_weights(weighting, MAX_DISTANCE, q, case["tgt_pts"], qn, case["tgt_nrm"], None, None, m)
    out = orc.compact(q, qn, case["tgt_pts"], case["tgt_nrm"], m)
    assert len(out[0]) == case["n_valid"], case["name"]
    return out


def _sums_header(s, d):
    out = np.zeros(64)
    out[0] = len(s); out[1:4] = s.astype(np.float64).sum(0); out[4:7] = d.astype(np.float64).sum(0)
    return out


# ------------------------------------------------------------------------------------------------ point-to-plane
def solve_plane(s, d, nt, w):
    A32, b32 = plane_rows(s, d, nt, w)
    A = A32.astype(np.float64); b = b32.astype(np.float64)
    U, sv, Vt = np.linalg.svd(A, full_matrices=False)
    keep = sv > CUT * sv[0]
    x = Vt[keep].T @ ((U[:, keep].T @ b) / sv[keep])
    sums = _sums_header(s, d)
    sums[7:28] = (A.T @ A)[np.triu_indices(6)]; sums[28:34] = A.T @ b
    sabs = np.zeros(64); sabs[7:28] = (np.abs(A).T @ np.abs(A))[np.triu_indices(6)]; sabs[28:34] = np.abs(A).T @ np.abs(b)
    return dict(x=x, spectrum=sv / sv[0] if sv[0] > 0 else sv, keep=keep, Vt=Vt, cost=float(np.sum((A @ x - b) ** 2)), A=A, b=b, sums=sums, sums_abs=sabs)


def excess_cost(ref, x):
    """||A x - b||^2 - ||A x_ref - b||^2 through the normal form (x - x_ref)^T A^T A (x - x_ref) + 2 (x - x_ref)^T A^T (A x_ref - b):
    no cancellation between two large costs."""
    A, b = ref["A"], ref["b"]
    dx = np.asarray(x, np.float64) - ref["x"]
    return float(np.sum((A @ dx) ** 2) + 2.0 * (A @ dx) @ (A @ ref["x"] - b))


def classify(spectrum):
    r = np.asarray(spectrum, np.float64)
    band = (r >= CUT / 2) & (r <= 2 * CUT)
    if band.any():
        raise AssertionError("ratio inside the excluded band: %r" % (r,))
    dropped = r < CUT / 2
    kept = r[~dropped]
    if (kept >= WELL).all():
        return "T" if dropped.any() else "W"
    if dropped.any():
        raise AssertionError("dropped directions AND kept ratios below 2e-4: %r" % (r,))
    return "I"


# ------------------------------------------------------------------------------------------------ pose algebra
def rot_xyz(al, be, ga):
    ca, sa, cb, sb, cg, sg = np.cos(al), np.sin(al), np.cos(be), np.sin(be), np.cos(ga), np.sin(ga)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]); Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def pose_from_x(x):
    """dT = [Rx Ry Rz | t] (ICPOptimizer.h:768-775) in fp64."""
    T = np.eye(4); T[:3, :3] = rot_xyz(x[0], x[1], x[2]); T[:3, 3] = x[3:6]
    return T


def pose_from_x_f32(x):
    """The same with the reference's roundings: fp32 angles, fp32 sines / cosines, fp32 products."""
    a = np.asarray(x, np.float64).astype(f32)
    c = np.cos(a[:3].astype(np.float64)).astype(f32); s = np.sin(a[:3].astype(np.float64)).astype(f32)
    o, z = f32(1), f32(0)
    Rx = np.array([[o, z, z], [z, c[0], -s[0]], [z, s[0], c[0]]], f32); Ry = np.array([[c[1], z, s[1]], [z, o, z], [-s[1], z, c[1]]], f32)
    Rz = np.array([[c[2], -s[2], z], [s[2], c[2], z], [z, z, o]], f32)
    T = np.eye(4, dtype=f32); T[:3, :3] = (Rx @ Ry) @ Rz; T[:3, 3] = a[3:6]
    return T


def angles_from_pose(dT):
    """(alpha, beta, gamma, t) of dT = [Rx Ry Rz | t]: the x the solve returned, when the incoming pose was the identity."""
    R = np.asarray(dT, np.float64)[:3, :3]
    be = np.arctan2(R[0, 2], np.hypot(R[0, 0], R[0, 1]))
    al = np.arctan2(-R[1, 2], R[2, 2]); ga = np.arctan2(-R[0, 1], R[0, 0])
    return np.array([al, be, ga, dT[0, 3], dT[1, 3], dT[2, 3]], np.float64)


def rigid_defect(T):
    T = np.asarray(T, np.float64); R = T[:3, :3]
    return max(float(np.abs(R @ R.T - np.eye(3)).max()), abs(float(np.linalg.det(R)) - 1.0), float(np.abs(T[3] - [0, 0, 0, 1]).max()))


# ------------------------------------------------------------------------------------------------ point-to-point
def minimal_rotation(v, u, kmin_axis=True):
    """The rotation by the smallest angle that takes the unit vector v to the unit vector u (axis v x u); for u = -v the half turn
    about the axis perpendicular to v that the project's kmin rule picks (e_k - (e_k . v) v with k the smallest |v_k|, the LAST index
    winning a tie between 0 / 1 and 2, the first between 0 and 1 -- the ternary of procrustes_rotation)."""
    v = np.asarray(v, np.float64); u = np.asarray(u, np.float64)
    c = float(v @ u)
    if 1.0 + c < 1e-8:
        a = np.abs(v)
        k = (0 if a[0] < a[2] else 2) if a[0] < a[1] else (1 if a[1] < a[2] else 2)
        e = np.zeros(3); e[k] = 1.0
        ax = e - v[k] * v; ax /= np.linalg.norm(ax)
        return 2.0 * np.outer(ax, ax) - np.eye(3)
    k = np.cross(v, u)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + K + (K @ K) / (1.0 + c)


def solve_p2p(s, d, w):
    """Kabsch through numpy's SVD, D = diag(1, 1, det(U V^T)) -- an independent reference for rank 2 and 3.  For rank <= 1 there is nothing
    to be independent of: the optimum is a family and the rule below is a DEFINITION (icp_hip.h), restated here a third time; agreement
    shows a consistent transcription, and what makes the rule sound is checked on its own (test_minimal_rotation_rule, and R v_1 = u_1).
    The project's rule (icp_hip.h, icp_iterate):
    rank 0 (sigma_1 <= (3 eps_f32)^2 x the largest uncentred moment |sum w d_j s_k|) -> R = I;
    rank 1 (sigma_2 <= 3 eps_f32 sigma_1) -> minimal_rotation(v_1, u_1)."""
    s = np.asarray(s, f32); d = np.asarray(d, f32); w = np.asarray(w, f32)
    sm, dm = means_f32(s, d)
    sr = w[:, None] * (s - sm); dr = d - dm
    assert sr.dtype == f32 and dr.dtype == f32
    A = dr.astype(np.float64).T @ sr.astype(np.float64)
    U, sv, Vt = np.linalg.svd(A)
    s64, d64, w64 = s.astype(np.float64), d.astype(np.float64), w.astype(np.float64)
    moment = (d64 * w64[:, None]).T @ s64
    floor = CUT3 * CUT3 * float(np.abs(moment).max())
    if sv[0] <= floor:
        rank = 0; R = np.eye(3)
    elif sv[1] <= max(CUT3 * sv[0], floor):
        rank = 1; R = minimal_rotation(Vt[0], U[:, 0])
    else:
        rank = 3 if sv[2] > CUT3 * sv[0] else 2
        R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = dm.astype(np.float64) - R @ sm.astype(np.float64)
    sums = _sums_header(s, d)
    sums[7] = w64.sum(); sums[8:11] = (w64[:, None] * s64).sum(0); sums[11:14] = (w64[:, None] * d64).sum(0); sums[14:23] = moment.reshape(9)
    sabs = np.zeros(64); sabs[7] = np.abs(w64).sum(); sabs[8:11] = np.abs(w64[:, None] * s64).sum(0); sabs[11:14] = np.abs(w64[:, None] * d64).sum(0)
    sabs[14:23] = (np.abs(d64 * w64[:, None]).T @ np.abs(s64)).reshape(9)
    return dict(sums_abs=sabs, pose=T, R=R, sv=sv, rank=rank, u=U[:, 0], v=Vt[0], det=float(np.linalg.det(U @ Vt)), A=A, sums=sums, mean_s=sm, mean_d=dm)


# ------------------------------------------------------------------------------------------------ symmetric
def _fullpiv_lu(M, g):
    """FullPivLU::solve with its rank rule (ICPOptimizer.h:866-868): returns (x, |pivots| / max pivot)."""
    M = M.copy(); g = g.copy(); n = 6
    colp = list(range(n)); piv = []
    for k in range(n):
        sub = np.abs(M[k:, k:]); i, j = np.unravel_index(np.argmax(sub), sub.shape); i += k; j += k
        if sub.max() == 0.0:
            break
        M[[k, i]] = M[[i, k]]; g[[k, i]] = g[[i, k]]
        M[:, [k, j]] = M[:, [j, k]]; colp[k], colp[j] = colp[j], colp[k]
        piv.append(abs(M[k, k]))
        for r in range(k + 1, n):
            f = M[r, k] / M[k, k]; M[r, k + 1:] -= f * M[k, k + 1:]; M[r, k] = 0.0; g[r] -= f * g[k]
    piv = np.array(piv + [0.0] * (n - len(piv))); mx = piv.max()
    r = 0
    while r < n and piv[r] > mx * CUT:
        r += 1
    y = np.zeros(n)
    for k in range(r - 1, -1, -1):
        y[k] = (g[k] - M[k, k + 1:r] @ y[k + 1:r]) / M[k, k]
    x = np.zeros(n)
    for k in range(n):
        x[colp[k]] = y[k] if k < r else 0.0
    return x, piv / mx


def solve_symmetric(s, d, ns, nt, w):
    s = np.asarray(s, f32); d = np.asarray(d, f32); w = np.asarray(w, f32)
    sm, dm = means_f32(s, d)
    A32, b32 = plane_rows(s - sm, d - dm, np.asarray(nt, f32) + np.asarray(ns, f32), w, symmetric=True)
    A = A32.astype(np.float64); b = b32.astype(np.float64)
    AtA = A.T @ A; Atb = A.T @ b
    l2 = f32(0.0001) * f32(0.0001)
    x, ratios = _fullpiv_lu(AtA + float(l2) * np.eye(6), Atb)
    with np.errstate(all="ignore"):
        at = x[:3].astype(f32); tt = x[3:].astype(f32)
        tan = np.sqrt(at[0] * at[0] + (at[1] * at[1] + at[2] * at[2]))
        ax = at / tan
        sin = f32(float(tan) / np.sqrt(1.0 + float(tan * tan))); cos = sin / tan
        t = tt * cos
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], f32)
        Rod = np.eye(3, dtype=f32) + (sin * K + ((f32(1) - cos) * K) @ K)

        def tr(R, v):
            T = np.eye(4, dtype=f32); T[:3, :3] = R; T[:3, 3] = v
            return T
        I3 = np.eye(3, dtype=f32); Rm = tr(Rod, np.zeros(3, f32))
        T = (((tr(I3, dm) @ Rm) @ tr(I3, t)) @ Rm) @ tr(I3, -sm)
    sums = _sums_header(s, d)
    sums[7:28] = AtA[np.triu_indices(6)]; sums[28:34] = Atb
    sabs = np.zeros(64); sabs[7:28] = (np.abs(A).T @ np.abs(A))[np.triu_indices(6)]; sabs[28:34] = np.abs(A).T @ np.abs(b)
    return dict(sums_abs=sabs, pose=T, x=x, ratios=ratios, sums=sums, mean_s=sm, mean_d=dm)


# ------------------------------------------------------------------------------------------------ input families
MAX_DISTANCE = 0.01          # (0.1 m)^2: the matcher's threshold is a squared distance
N_DECOYS = 5


def _finish(name, tp, tn, sp, sn, expected=None, metrics=("p2p", "plane", "sym"), pose=None, **kw):
    """Adds the decoys (sources >= 10 m from every target; they must stay unmatched) and checks the spacing rule: targets >= 0.5 m
    apart, every source within a quarter of the smallest target spacing (and within 0.1 m) of ITS target."""
    tp = np.asarray(tp, f32); sp = np.asarray(sp, f32); tn = np.asarray(tn, f32); sn = np.asarray(sn, f32)
    expected = np.arange(len(sp), dtype=np.int32) if expected is None else np.asarray(expected, np.int32)
    if len(tp) > 1:
        dd = np.linalg.norm(tp[:, None].astype(np.float64) - tp[None].astype(np.float64), axis=2); np.fill_diagonal(dd, np.inf)
        spacing = dd.min()
        assert spacing >= 0.5, (name, spacing)
    else:
        spacing = 0.5
    pose = np.eye(4, dtype=f32) if pose is None else np.asarray(pose, f32)
    q = sp.astype(np.float64) @ pose[:3, :3].astype(np.float64).T + pose[:3, 3].astype(np.float64)
    disp = np.linalg.norm(q - tp[expected].astype(np.float64), axis=1)
    assert disp.max() <= min(spacing / 4, 0.09), (name, disp.max())
    centre = tp.astype(np.float64).mean(0); radius = np.linalg.norm(tp - centre, axis=1).max()
    dirs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)
    decoys_world = centre + dirs * (radius + 16.0 + 2.0 * np.arange(N_DECOYS)[:, None])
    decoys = (decoys_world - pose[:3, 3].astype(np.float64)) @ pose[:3, :3].astype(np.float64)      # so that pose * decoy lands there
    sp_all = np.concatenate([sp[:len(sp) // 2], decoys[:2].astype(f32), sp[len(sp) // 2:], decoys[2:].astype(f32)])
    sn_all = np.concatenate([sn[:len(sp) // 2], np.tile(f32([0, 0, 1]), (2, 1)), sn[len(sp) // 2:], np.tile(f32([0, 0, 1]), (N_DECOYS - 2, 1))])
    idx = np.concatenate([expected[:len(sp) // 2], [-1, -1], expected[len(sp) // 2:], [-1] * (N_DECOYS - 2)]).astype(np.int32)
    return dict(name=name, tgt_pts=tp, tgt_nrm=tn, src_pts=sp_all, src_nrm=sn_all, idx=idx, n_valid=len(sp), metrics=metrics, pose=pose, **kw)


def _axis_normals(n, pattern):
    e = np.eye(3, dtype=f32)
    return np.stack([e[pattern[i % len(pattern)]] for i in range(n)])


def _dy(a, bits=8):
    """round to multiples of 2^-bits: exact in fp32, and every product / moment of such values exact in fp64"""
    return (np.round(np.asarray(a, np.float64) * (1 << bits)) / (1 << bits)).astype(f32)


def _general_cloud(seed, n, extent, offset):
    """n points on a jittered grid (spacing >= 0.5 m) of half-width `extent`, shifted by `offset` along (1, 1, 1) / sqrt 3; unit
    normals in general position; source = target moved by a small rigid motion + noise."""
    rng = np.random.default_rng(seed)
    g = int(np.ceil(n ** (1 / 3)))
    step = 2.0 * extent / max(g - 1, 1)
    assert step >= 0.65
    grid = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(g ** 3)[:n]]
    tp = grid * step - extent + rng.uniform(-0.05, 0.05, (n, 3)) + offset / np.sqrt(3.0)
    tn = rng.normal(size=(n, 3)); tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    c = tp.mean(0)
    R = rot_xyz(*(rng.uniform(-1, 1, 3) * 0.01))
    sp = (tp - c) @ R.T + c + rng.uniform(-1, 1, 3) * 0.02 + rng.normal(size=(n, 3)) * 0.003
    sn = tn @ R.T + rng.normal(size=(n, 3)) * 0.02; sn /= np.linalg.norm(sn, axis=1, keepdims=True)
    return tp, tn, sp, sn


LADDER = (1e-1, 3e-2, 1e-2, 1e-3, 1e-4, 3e-6, 1e-6, 1e-7)          # lateral spread of the near-collinear line [m]; 1e-5 lands inside the excluded band (4.9e-7)
OFFSETS = (0.0, 30.0, 300.0, 2000.0, 3000.0)


def make_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))      # a fixed seed per case name
    if name in ("one", "two", "three"):
        k = {"one": 1, "two": 2, "three": 3}[name]
        tp = _dy([[1.5, -0.75, 2.25], [2.5, 0.25, 2.0], [1.25, 1.0, 3.5]])[:k]
        tn = _axis_normals(k, (2, 0, 1))
        sp = tp + _dy([[0.03125, -0.015625, 0.0234375], [-0.0234375, 0.03125, 0.015625], [0.015625, 0.0234375, -0.03125]])[:k]
        return _finish(name, tp, tn, sp, tn.copy(), metrics=("p2p", "plane", "sym"), exact=True)
    if name == "coincident16":
        tp = _dy([[1.5, -0.75, 2.25], [4.0, 3.0, 2.0]]); tn = _axis_normals(2, (2, 0))
        sp = np.tile(tp[:1] + _dy([[0.03125, -0.015625, 0.0234375]]), (16, 1)); sn = np.tile(tn[:1], (16, 1))
        return _finish(name, tp, tn, sp, sn, expected=np.zeros(16, np.int32), metrics=("p2p", "plane"), exact=True)
    if name == "collinear64":
        i = np.arange(64)
        tp = _dy(np.stack([0.5 * i - 16.0, np.full(64, 0.75), np.full(64, -1.25)], 1))      # along x: 32 m long at 0.5 m spacing
        tn = _axis_normals(64, (1, 2, 1, 1, 2))
        xs = tp[:, 0] + _dy(0.03125 * np.cos(i)) + f32(0.015625)                             # slides along the line ...
        sp = np.stack([xs, f32(0.75) + xs * f32(2.0 ** -8), np.full(64, -1.25, f32)], 1)     # ... which is turned about z by a slope of 2^-8: still a line
        return _finish(name, tp, tn, sp, tn.copy(), metrics=("p2p", "plane", "sym"), exact=True)
    if name == "collinear_far":
        # a line ~1000 m from the origin in a general direction: collinear only up to the fp32 rounding of its coordinates (6e-5 m there),
        # and uncentred moments 1e6 times the centred ones -- the cancellation noise of the device's moment expansion
        i = np.arange(64)
        dirn = np.array([2.0, -1.0, 2.0]) / 3.0
        tp = (np.array([600.0, -550.0, 580.0]) + np.outer(0.75 * i - 24.0, dirn)).astype(f32)
        tn = _axis_normals(64, (1, 2, 0, 1, 2))
        sp = (tp.astype(np.float64) + np.outer(0.02 * np.cos(i) + 0.01, dirn)).astype(f32)
        return _finish(name, tp, tn, sp, tn.copy(), metrics=("p2p",), exact=False)
    if name.startswith("ladder_"):
        eps = float(name[len("ladder_"):])
        i = np.arange(64)
        lat = rng.uniform(-1, 1, (64, 2)) * eps
        tp = np.stack([0.5 * i - 16.0, 0.75 + lat[:, 0], -1.25 + lat[:, 1]], 1)
        tn = rng.normal(size=(64, 3)); tn /= np.linalg.norm(tn, axis=1, keepdims=True)
        # the rows are built from the SOURCE points: its lateral spread is what the weak direction (the turn about the line) sees.  The
        # source is a small rigid motion of the target plus noise that scales with eps as well, so that the turn about the line that
        # the linearised solve asks for stays a fraction of a radian on every rung (a residual of centimetres over a lever of eps
        # metres would ask for many turns, which no pose can be read back from)
        c0 = np.array([0.0, 0.75, -1.25]); R0 = rot_xyz(0.05, 0.001, -0.001)
        sp = (tp - c0) @ R0.T + c0 + [0.01, -0.008, 0.006] + rng.uniform(-0.2, 0.2, (64, 3)) * eps
        return _finish(name, tp, tn, sp, tn.copy(), metrics=("plane",) if name == "ladder_0.01" else ("p2p", "plane"), exact=False)
    if name == "planar":
        gx, gy = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
        tp = _dy(np.stack([0.5 * gx.ravel() - 1.75, 0.5 * gy.ravel() - 1.25, np.full(64, 2.5)], 1))
        tn = _axis_normals(64, (2,))
        j = np.arange(64)
        sp = tp + _dy(np.stack([0.03125 * np.cos(j), 0.03125 * np.sin(1.7 * j), np.zeros(64)], 1)) + _dy([0.015625, -0.0078125, 0.03125])
        return _finish(name, tp, tn, sp, tn.copy(), metrics=("p2p", "plane", "sym"), exact=True)
    if name == "mirror":
        gx, gy = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
        z = rng.uniform(-0.04, 0.04, 49)
        tp = np.stack([0.7 * gx.ravel() - 2.1 + rng.uniform(-0.05, 0.05, 49), 0.8 * gy.ravel() - 2.4 + rng.uniform(-0.05, 0.05, 49), z], 1)
        sp = tp * [1, 1, -1] + rng.normal(size=(49, 3)) * 0.0005               # thin slab, z flipped: the best orthogonal map is a reflection
        tn = _axis_normals(49, (2,))
        return _finish(name, tp, tn, sp, tn.copy(), metrics=("p2p",), exact=False)
    if name.startswith("offset_"):
        off = float(name[len("offset_"):])
        tp, tn, sp, sn = _general_cloud(11, 48, 1.0, off)
        return _finish(name, tp, tn, sp, sn, metrics=("p2p", "plane", "sym"), exact=False)
    if name == "aligned":
        tp, tn, _, _ = _general_cloud(5, 40, 1.0, 0.0)
        tp = tp.astype(f32); tn = tn.astype(f32)
        return _finish(name, tp, tn, tp.copy(), tn.copy(), metrics=("p2p", "plane", "sym"), exact=False)
    if name == "control":
        tp, tn, sp, sn = _general_cloud(7, 60, 1.0, 0.0)
        P = np.eye(4); P[:3, :3] = rot_xyz(0.3, -0.2, 0.5); P[:3, 3] = [0.4, -0.3, 0.2]
        P = P.astype(f32)
        Pi = np.linalg.inv(P.astype(np.float64))
        sp0 = sp @ Pi[:3, :3].T + Pi[:3, 3]; sn0 = sn @ Pi[:3, :3].T
        return _finish(name, tp, tn, sp0, sn0, metrics=("p2p", "plane", "sym"), pose=P, exact=False)
    raise KeyError(name)


CASES = ("one", "two", "three", "coincident16", "collinear64", "collinear_far") + tuple("ladder_%g" % e for e in LADDER) + ("planar", "mirror") \
    + tuple("offset_%g" % o for o in OFFSETS) + ("aligned", "control")

# The class every point-to-plane case was DESIGNED for; the tests assert classify(reference spectrum) == this.
PLANE_CLASS = {"one": "T", "two": "T", "three": "W", "coincident16": "T", "collinear64": "T", "planar": "W",
               "ladder_0.1": "W", "ladder_0.03": "W", "ladder_0.01": "W", "ladder_0.001": "I", "ladder_0.0001": "I", "ladder_3e-06": "T", "ladder_1e-06": "T", "ladder_1e-07": "T",
               "offset_0": "W", "offset_30": "W", "offset_300": "I", "offset_2000": "T", "offset_3000": "T", "aligned": "W", "control": "W"}
# Point-to-point (p2p_class): R0 / R1 = the rank rule decides, U = unique optimum, I = in between.  ladder_0.01 has sigma_2 / sigma_1 =
# 4.1e-7, inside the excluded band around 3 eps_f32, so that rung is not a point-to-point case.
P2P_CLASS = {"one": "R0", "two": "R1", "three": "U", "coincident16": "R0", "collinear64": "R1", "collinear_far": "R1", "planar": "U", "mirror": "U",
             "ladder_0.1": "I", "ladder_0.03": "I", "ladder_0.001": "R1", "ladder_0.0001": "R1", "ladder_3e-06": "R1", "ladder_1e-06": "R1", "ladder_1e-07": "R1",
             "offset_0": "U", "offset_30": "U", "offset_300": "U", "offset_2000": "U", "offset_3000": "U", "aligned": "U", "control": "U"}
# Symmetric (sym_class): N = tan_theta is exactly 0 (all-NaN pose, the reference's quirk), T = pivots dropped, F = none dropped
SYM_CLASS = {"one": "N", "two": "F", "three": "F", "collinear64": "T", "planar": "F", "offset_0": "F", "offset_30": "F", "offset_300": "F", "offset_2000": "F", "offset_3000": "F",
             "aligned": "N", "control": "F"}


# ------------------------------------------------------------------------------------------------ what is asserted in each class
POSE_TOL = 1e-5                       # the project's bar: 1e-5 rad, 1e-5 m
RIGID_TOL = 16 * EPS32                # a rotation written in fp32 through a handful of fp32 products
FAR = ("offset_30", "offset_300", "offset_2000", "offset_3000", "collinear_far")      # translations compared at the source centroid (see rot_trans_error)


def rot_trans_error(A, B, at):
    """(rotation angle between A and B [rad], |A at - B at| [m]).  A pose written in fp32 cannot hold 1e-5 m in its translation column
    when the cloud is 3000 m from the origin (one ulp there is 2.4e-4 m); what it can hold is where it sends the cloud."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64)
    R = A[:3, :3] @ B[:3, :3].T
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(s, (np.trace(R) - 1) / 2)), float(np.linalg.norm((A[:3, :3] - B[:3, :3]) @ at + A[:3, 3] - B[:3, 3]))


def delta_pose(pose_out, pose_in):
    return np.asarray(pose_out, np.float64) @ np.linalg.inv(np.asarray(pose_in, np.float64))


# Excess-cost margins of class I (point-to-plane): 16 x the largest excess cost, over the family, of the REFERENCE solution after it went
# through the fp32 pose (pose_from_x_f32) and back (angles_from_pose) -- the floor that an fp32 pose imposes on any implementation.
# Measured with `python tests/test_solve_host.py --measure` (floors 3.4e-16 and 6.0e-13); solving with one direction too few costs
# 3.7e-10 .. 4.3e-8 (ladder) and 1.2e-4 (offset_300): 5 and 7 orders of magnitude above the margins.
PLANE_I_MARGIN = {"ladder": 16 * 3.5e-16, "offset": 16 * 6.1e-13}
# Point-to-point, class I (sigma_2 / sigma_1 between 2 x 3 eps_f32 and 2e-4): loss of the Procrustes objective tr(R A^T) / sigma_1 against
# Kabsch; floor = the same for Kabsch's R rounded to fp32 (measured 2.8e-8 by the same command), margin 16 x.
P2P_I_MARGIN = 16 * 2.8e-8


def family(name):
    return name.split("_")[0]


def p2p_class(ref):
    """'R0' / 'R1' (the rank rule decides), 'U' (unique optimum: sigma_2 / sigma_1 >= 2e-4), 'I' (in between); a ratio inside
    [3 eps_f32 / 2, 2 x 3 eps_f32] is an error, as for the other metrics."""
    sv = ref["sv"]
    if ref["rank"] == 0:
        return "R0"
    r = sv[1] / sv[0]
    assert not (CUT3 / 2 <= r <= 2 * CUT3), "sigma_2 / sigma_1 = %g inside the excluded band" % r
    return "R1" if ref["rank"] == 1 else ("U" if r >= WELL else "I")


def sym_class(ref):
    """'N' (the rotation part of x is exactly zero: the reference divides by tan_theta = 0), 'T' / 'F' (pivots dropped / none dropped; the
    W and T of the other metrics: every kept pivot ratio is asserted well-posed, so there is no class I here)."""
    if not np.any(ref["x"][:3]):
        return "N"
    r = ref["ratios"]
    assert not ((r >= CUT / 2) & (r <= 2 * CUT)).any(), "pivot ratio inside the excluded band: %r" % (r,)
    kept = r[r > CUT]
    # the pivots of A^T A + lambda^2 I scale as sigma^2: the 2e-4 below which the 1e-5 bar is no property of a correct implementation
    # (fp64 normal equations lose cond^2 x 1e-16) is 4e-8 on them
    assert (kept >= WELL * WELL).all(), "kept pivot ratio below (2e-4)^2: not comparable at 1e-5: %r" % (r,)
    return "T" if (r < CUT / 2).any() else "F"


def check_close(label, got, want, at, far, noise=0.0, noise_rot=0.0):
    """noise / noise_rot: the distance between the oracle's mode 0 and mode 1 on the same input, the standing measure of the reference's
    own rounding noise; 16 x it is allowed on top of the bar (far-offset clouds only; noise_rot only where poses are chained)."""
    ang, tr = rot_trans_error(got, want, at)
    print("%s: rotation %.3g rad, translation at the centroid %.3g m (noise %.3g)" % (label, ang, tr, noise))
    assert np.isfinite(np.asarray(got)).all(), label
    assert ang <= POSE_TOL + 16 * noise_rot, (label, ang, noise_rot)
    assert tr <= POSE_TOL + 16 * noise, (label, tr, noise)
    if not far:
        t0 = float(np.linalg.norm(np.asarray(got, np.float64)[:3, 3] - np.asarray(want, np.float64)[:3, 3]))
        assert t0 <= POSE_TOL, (label, t0)


def check_plane(label, name, cls, ref, dT, at, noise=0.0):
    """dT: the delta pose an implementation produced (fp64 copy of its fp32 pose, incoming pose divided out)."""
    x = angles_from_pose(dT)
    if cls in ("W", "T"):
        # x_ref through the reference's own fp32 pose algebra (ICPOptimizer.h:768-775): the entries of a rotation written in fp32 are
        # off by 3e-8, which 3000 m from the origin is 1e-4 m at the cloud -- a property of the format, not of the solve
        check_close(label, dT, pose_from_x_f32(ref["x"]), at, name in FAR, noise)
        leak = float(np.abs(ref["Vt"][~ref["keep"]] @ x).max()) if (~ref["keep"]).any() else 0.0
        print("%s: dropped directions carry %.3g" % (label, leak))
        assert leak <= POSE_TOL, (label, leak)
    else:
        assert np.isfinite(dT).all() and rigid_defect(dT) <= RIGID_TOL, (label, rigid_defect(dT))
        exc = excess_cost(ref, x); margin = PLANE_I_MARGIN[family(name)]
        print("%s: excess cost %.3g (margin %.3g)" % (label, exc, margin))
        assert exc <= margin, (label, exc, margin)


def p2p_objective_loss(ref, R):
    return float(np.trace((ref["R"] - np.asarray(R, np.float64)) @ ref["A"].T) / ref["sv"][0])


def check_p2p(label, name, cls, ref, dT, at, noise=0.0):
    if cls == "I":
        assert np.isfinite(dT).all() and rigid_defect(dT) <= RIGID_TOL, (label, rigid_defect(dT))
        loss = p2p_objective_loss(ref, dT[:3, :3]); lead = float(np.abs(dT[:3, :3] @ ref["v"] - ref["u"]).max())
        print("%s: objective loss %.3g (margin %.3g), |R v1 - u1| %.3g" % (label, loss, P2P_I_MARGIN, lead))
        assert loss <= P2P_I_MARGIN, (label, loss)
        assert lead <= POSE_TOL, (label, lead)            # every optimal rotation takes v_1 to u_1
    else:
        check_close(label, dT, ref["pose"], at, name in FAR, noise)
