"""fp64 numpy restatement of Generalized-ICP in its plane-to-plane form, written from the contract in DESIGN.md (section 6e) and
include/icp_hip.h.  Test infrastructure only.

  normals(pts, k)                  GICP normals: k smallest (fp32 d2, index) pairs over the finite points, fp64 PCA (numpy eigh)
  plane_cov(n, eps)                I - (1 - eps) n n^T
  pair_terms(p, q, a, b, w, eps)   per pair: validity, Sigma, M, J, r and the contributions w^2 J^T M J, w^2 J^T M r
  sums(...)                        the 34 sums of icp_correspond (n, sum s, sum d, upper triangle of H, g) and their absolute sums
  solve(s)                         H x = g
  compose(x, pose)                 the point-to-plane composition in fp32: Rx Ry Rz from three small angles, then dT * pose
  mul_pose(D, pose)                D * pose in fp32, the product compose ends with
  step(...)                        one ICP step on given correspondences
"""
import numpy as np
from scipy.spatial import cKDTree

f32 = np.float32
TRIU = [(a, c) for a in range(6) for c in range(a, 6)]


def _d2_f32(p, q):
    """(dx*dx + dy*dy) + dz*dz in fp32, one rounding per operation (the device's order)."""
    d = (p.astype(f32) - q.astype(f32)).astype(f32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)


def neighbours(pts, k):
    """(n, min(k, finite)) indices of the k smallest (fp32 d2, index) pairs of every finite point over the finite points (-1 rows for
    non-finite points, or when fewer than 3 points are finite)."""
    pts = np.ascontiguousarray(pts, f32)
    n = len(pts)
    fin = np.nonzero(np.isfinite(pts).all(1))[0]
    kk = min(k, len(fin))
    out = np.full((n, max(kk, 1)), -1, np.int64)
    if len(fin) < 3:
        return out[:, :kk] if kk else out[:, :0]
    tree = cKDTree(pts[fin].astype(np.float64))
    kq = min(len(fin), kk + 8)
    dist, loc = tree.query(pts[fin].astype(np.float64), k=kq)
    dist = dist.reshape(len(fin), kq); loc = loc.reshape(len(fin), kq)
    cand = fin[loc]
    d2 = _d2_f32(pts[fin][:, None, :], pts[cand])
    order = np.lexsort((cand, d2), axis=1)
    cand = np.take_along_axis(cand, order, 1); d2 = np.take_along_axis(d2, order, 1)
    t = d2[:, kk - 1].astype(np.float64)
    # complete when every point outside the candidates is provably farther than the k-th fp32 distance (fp32 d2 is within 1e-6 relative)
    complete = (kq == len(fin)) | (dist[:, -1] ** 2 > t * (1 + 1e-5) + 1e-37)
    for r in np.nonzero(~complete)[0]:
        i = fin[r]
        ids = fin[tree.query_ball_point(pts[i].astype(np.float64), np.sqrt(t[r] * (1 + 1e-4)) + 1e-30)]
        dd = _d2_f32(pts[i][None, :], pts[ids])
        o = np.lexsort((ids, dd))
        cand[r, :kk] = ids[o][:kk]
    out[fin] = cand[:, :kk]
    return out


def normals(pts, k, nb=None, cov=False):
    """GICP normals (n, 3) fp32 and the ascending eigenvalues (n, 3) fp64 of every point's neighbourhood covariance (NaN where undefined).
    nb: neighbours(pts, k) when the caller has it; cov: the fp64 covariances (n, 3, 3) as a third result."""
    pts = np.ascontiguousarray(pts, f32)
    if nb is None:
        nb = neighbours(pts, k)
    n = len(pts)
    nrm = np.full((n, 3), np.nan, f32); ev = np.full((n, 3), np.nan); covs = np.full((n, 3, 3), np.nan)
    ok = (nb >= 0).all(1) & (nb.shape[1] >= 3)
    if not ok.any():
        return (nrm, ev, covs) if cov else (nrm, ev)
    X = pts[nb[ok]].astype(np.float64)                       # (m, k, 3)
    D = X - X.mean(1, keepdims=True)
    C = np.einsum("mki,mkj->mij", D, D) / X.shape[1]
    w, V = np.linalg.eigh(C)
    v = V[:, :, 0].copy()
    zero = ~(np.abs(C).reshape(len(C), 9) > 0).any(1)         # coincident neighbours: Jacobi's first axis
    v[zero] = (1.0, 0.0, 0.0)
    nrm[ok] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    ev[ok] = w; covs[ok] = C
    return (nrm, ev, covs) if cov else (nrm, ev)


def plane_cov(n, eps):
    eps = float(f32(eps))
    n = np.asarray(n, np.float64)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    return np.eye(3) - (1.0 - eps) * n[..., :, None] * n[..., None, :]


def skew(p):
    p = np.asarray(p, np.float64)
    z = np.zeros(p.shape[:-1])
    return np.stack([np.stack([z, -p[..., 2], p[..., 1]], -1), np.stack([p[..., 2], z, -p[..., 0]], -1), np.stack([-p[..., 1], p[..., 0], z], -1)], -2)


def pair_terms(p, q, a, b, w, eps):
    """p: fp32 transformed source points, q: fp32 target points, a: target GICP normals, b: source GICP normals moved by the pose (fp32),
    w: weights.  Returns (ok, H (m, 6, 6), g (m, 6), Sigma, M, J, r) for the pairs with finite, non-zero a and b (ok mask over the input)."""
    eps = float(f32(eps))                                    # icp_gicp_options.epsilon is an fp32 field
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    la = np.linalg.norm(a, axis=1); lb = np.linalg.norm(b, axis=1)
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1) & (la > 0) & (lb > 0)
    a = a[ok] / la[ok, None]; b = b[ok] / lb[ok, None]
    P = np.asarray(p, f32)[ok].astype(np.float64); Q = np.asarray(q, f32)[ok].astype(np.float64)
    W2 = np.asarray(w, f32)[ok].astype(np.float64) ** 2
    S = 2.0 * np.eye(3) - (1.0 - eps) * (a[:, :, None] * a[:, None, :] + b[:, :, None] * b[:, None, :])
    M = np.linalg.inv(S)
    J = np.concatenate([-skew(P), np.broadcast_to(np.eye(3), (len(P), 3, 3))], axis=2)
    r = Q - P
    JtM = np.einsum("mki,mkl->mil", J, M)
    H = W2[:, None, None] * np.einsum("mil,mlj->mij", JtM, J)
    g = W2[:, None] * np.einsum("mil,ml->mi", JtM, r)
    return ok, H, g, S, M, J, r


def sums(p, q, a, b, w, eps, valid):
    """The 34 sums icp_correspond returns for GICP, and the sums of the absolute contributions (the scale of each sum's rounding error).
    valid: the validity filter (record idx >= 0, finite p and q); a / b / w as in pair_terms."""
    p = np.asarray(p, f32)[valid]; q = np.asarray(q, f32)[valid]
    ok, H, g, *_ = pair_terms(p, q, np.asarray(a)[valid], np.asarray(b)[valid], np.asarray(w)[valid], eps)
    s = np.zeros(34); sa = np.zeros(34)
    s[0] = ok.sum(); sa[0] = s[0]
    s[1:4] = p[ok].astype(np.float64).sum(0); sa[1:4] = np.abs(p[ok].astype(np.float64)).sum(0)
    s[4:7] = q[ok].astype(np.float64).sum(0); sa[4:7] = np.abs(q[ok].astype(np.float64)).sum(0)
    for t, (i, j) in enumerate(TRIU):
        s[7 + t] = H[:, i, j].sum(); sa[7 + t] = np.abs(H[:, i, j]).sum()
    s[28:34] = g.sum(0); sa[28:34] = np.abs(g).sum(0)
    return s, sa


def unpack(s):
    H = np.zeros((6, 6))
    for t, (i, j) in enumerate(TRIU):
        H[i, j] = H[j, i] = s[7 + t]
    return H, np.asarray(s[28:34], np.float64)


def solve(s, lstsq=False):
    """lstsq: the minimum-norm step with the point-to-plane solve's rank rule (eigenvalues <= (6 eps_f32)^2 lambda_max of H dropped) --
    for systems that one or two pairs leave rank-deficient."""
    H, g = unpack(s)
    if not lstsq:
        return np.linalg.solve(H, g)
    ev, V = np.linalg.eigh(H)
    keep = ev > (6.0 * float(np.finfo(f32).eps)) ** 2 * ev.max()
    return V[:, keep] @ ((V[:, keep].T @ g) / ev[keep])


def delta_f32(x):
    """dT of ICPOptimizer.h:768-773 in fp32: Rx Ry Rz of the fp32 angles (fp64 sin / cos rounded once), translation x[3:6]."""
    al, be, ga = (f32(v) for v in x[:3])
    ca, sa = f32(np.cos(np.float64(al))), f32(np.sin(np.float64(al)))
    cb, sb = f32(np.cos(np.float64(be))), f32(np.sin(np.float64(be)))
    cg, sg = f32(np.cos(np.float64(ga))), f32(np.sin(np.float64(ga)))
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]], f32)
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]], f32)
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]], f32)

    def mul3(A, B):                                          # e0 + (e1 + e2)
        return np.array([[A[r, 0] * B[0, c] + (A[r, 1] * B[1, c] + A[r, 2] * B[2, c]) for c in range(3)] for r in range(3)], f32)
    D = np.eye(4, dtype=f32)
    D[:3, :3] = mul3(mul3(Rx, Ry), Rz); D[:3, 3] = np.asarray(x[3:6], np.float64).astype(f32)
    return D


def compose(x, pose):
    """dT * pose in fp32, sequential over k (mat4_mul_f32)."""
    return mul_pose(delta_f32(x), pose)


def mul_pose(D, pose):
    """D * pose in fp32, sequential over k (mat4_mul_f32)."""
    D = np.asarray(D, f32); P = np.asarray(pose, f32)
    out = np.zeros((4, 4), f32)
    for r in range(4):
        for c in range(4):
            acc = f32(D[r, 0] * P[0, c])
            for k in range(1, 4):
                acc = f32(acc + f32(D[r, k] * P[k, c]))
            out[r, c] = acc
    return out


def transform(pose, pts):
    """utils.h:113-115 in fp32: ((R_i0 x + R_i1 y) + R_i2 z) + t_i."""
    P = np.asarray(pose, f32); x = np.asarray(pts, f32)
    return np.stack([((P[i, 0] * x[:, 0] + P[i, 1] * x[:, 1]) + P[i, 2] * x[:, 2]) + P[i, 3] for i in range(3)], 1).astype(f32)


def step(pose, src, tgt, src_n, tgt_n, w, eps):
    """One GICP iteration on given correspondences src[i] <-> tgt[i] (fp64 normal matrix for the source normals): the new fp32 pose."""
    p = transform(pose, src)
    Rn = np.linalg.inv(np.asarray(pose, np.float64)[:3, :3]).T
    b = (np.asarray(src_n, np.float64) @ Rn.T).astype(f32)
    valid = np.isfinite(p).all(1) & np.isfinite(np.asarray(tgt, f32)).all(1)
    s, _ = sums(p, tgt, tgt_n, b, w, eps, valid)
    return compose(solve(s), pose), s
