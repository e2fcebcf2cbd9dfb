"""fp64 numpy restatement of colored ICP (Park, Zhou, Koltun, ICCV 2017), written from the contract in DESIGN.md (section 6g) and
include/icp_hip.h.  Test infrastructure only.

  intensity(rgba)                              (R + G + B) / 765 in fp64
  gradients(pts, nrm, rgba, k)                 the target's colour gradients (fp32) and each point's det / threshold margin
  pair_terms(p, q, n, d, di, w, lam)           per pair: validity, the geometric and photometric rows and residuals, H and g
  sums(...)                                    the 34 sums of icp_correspond and their absolute sums
  solve(s), compose(x, pose), transform(...)   gicp_restatement's (point-to-plane's solve convention H x = g, then dT * pose in fp32)
  step(...)                                    one colored ICP step on given correspondences
"""
import numpy as np

import gicp_restatement as G

f32 = np.float32
TRIU = G.TRIU
solve, compose, transform, unpack, skew = G.solve, G.compose, G.transform, G.unpack, G.skew


def intensity(rgba):
    """(R + G + B) / 765.0 in fp64 of (n, 4) uint8 colours."""
    c = np.asarray(rgba, np.uint8).reshape(-1, 4)
    return (c[:, 0].astype(np.int64) + c[:, 1] + c[:, 2]).astype(np.float64) / 765.0


def intensity_diff(src_rgba, tgt_rgba):
    """I_s - I_q as the post stage forms it: ((R + G + B)_s - (R + G + B)_q) / 765.0, one rounding."""
    a = np.asarray(src_rgba, np.uint8).reshape(-1, 4).astype(np.int64); b = np.asarray(tgt_rgba, np.uint8).reshape(-1, 4).astype(np.int64)
    return (a[:, :3].sum(1) - b[:, :3].sum(1)).astype(np.float64) / 765.0


def _unit(v, recip=False):
    """fp32 vectors -> fp64 unit vectors and the mask of the finite, non-zero ones (v / |v|; recip: v * (1 / |v|), the post stage's form)."""
    v = np.asarray(v, f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    ok = np.isfinite(v).all(1) & (ln > 0)
    u = np.zeros_like(v)
    u[ok] = v[ok] * (1.0 / ln[ok, None]) if recip else v[ok] / ln[ok, None]
    return u, ok


def gradients(pts, nrm, rgba, k, nb=None, full=False):
    """Colour gradients (n, 3) fp32 of the target (NaN: non-finite point or normal, zero normal; 0: fewer than 3 neighbours or a
    determinant at or below the threshold), and det / threshold per point (NaN where no system was solved).  nb: G.neighbours(pts, k)
    when the caller has it; full: as a third result the gradients solved without the threshold (fp32; NaN where det <= 0 or no system
    was solved) -- what a kernel whose determinant lands on the other side of the threshold returns."""
    pts = np.ascontiguousarray(pts, f32)
    n = len(pts)
    nu, nok = _unit(nrm)
    I = intensity(rgba)
    out = np.full((n, 3), np.nan, f32)
    margin = np.full(n, np.nan)
    solved = np.full((n, 3), np.nan, f32)
    live = np.isfinite(pts).all(1) & nok
    out[live] = 0.0
    if nb is None:
        nb = G.neighbours(pts, k)
    m = nb.shape[1]
    use = live & (nb >= 0).all(1) if m >= 3 else np.zeros(n, bool)
    if not use.any():
        return (out, margin, solved) if full else (out, margin)
    ids = np.nonzero(use)[0]
    P = pts[ids].astype(np.float64); N = nu[ids]
    Q = pts[nb[ids]].astype(np.float64)                              # (u, m, 3)
    V = Q - P[:, None, :]
    t = np.einsum("umi,ui->um", V, N)
    E = V - N[:, None, :] * t[:, :, None]                           # q'_j - p
    b = I[nb[ids]] - I[ids][:, None]
    self_row = nb[ids] == ids[:, None]                              # the point itself: no row
    E[self_row] = 0.0; b[self_row] = 0.0
    A = np.einsum("umi,umj->uij", E, E) + float(m - 1) ** 2 * N[:, :, None] * N[:, None, :]
    Ab = np.einsum("umi,um->ui", E, b)
    det = np.linalg.det(A)
    tr3 = np.trace(A, axis1=1, axis2=2) / 3.0
    thr = 1e-12 * tr3 ** 3
    adj = np.stack([np.cross(A[:, 1], A[:, 2]), np.cross(A[:, 2], A[:, 0]), np.cross(A[:, 0], A[:, 1])], 2)   # adj(A) = (cof A)^T, A symmetric
    ok = det > thr
    x = np.zeros((len(ids), 3))
    x[ok] = np.einsum("uij,uj->ui", adj[ok], Ab[ok]) / det[ok, None]
    out[ids] = x.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin[ids] = det / thr
    pos = det > 0
    free = np.full((len(ids), 3), np.nan)
    free[pos] = np.einsum("uij,uj->ui", adj[pos], Ab[pos]) / det[pos, None]
    solved[ids] = free.astype(f32)
    return (out, margin, solved) if full else (out, margin)


def pair_terms(p, q, n, d, di, w, lam):
    """p: fp32 transformed source points, q: fp32 target points, n: target normals, d: target gradients (fp32), di = I_s - I_q,
    w: weights, lam: lambda_geometric (an fp32 field).  Returns (ok, H (m, 6, 6), g (m, 6), jG, rG, jC, rC) for the pairs with a finite,
    non-zero n and a finite d (ok mask over the input)."""
    lam = float(f32(lam))
    nu, nok = _unit(n, recip=True)
    d = np.asarray(d, f32).astype(np.float64)
    ok = nok & np.isfinite(d).all(1)
    nu = nu[ok]; d = d[ok]
    P = np.asarray(p, f32)[ok].astype(np.float64); Q = np.asarray(q, f32)[ok].astype(np.float64)
    W2 = np.asarray(w, f32)[ok].astype(np.float64) ** 2
    DI = np.asarray(di, np.float64)[ok]
    J = np.concatenate([-skew(P), np.broadcast_to(np.eye(3), (len(P), 3, 3))], axis=2)
    u = d - nu * np.einsum("mi,mi->m", nu, d)[:, None]             # (I - n n^T) d
    jG = np.einsum("mi,mij->mj", nu, J); rG = np.einsum("mi,mi->m", nu, Q - P)
    jC = np.einsum("mi,mij->mj", u, J); rC = DI - np.einsum("mi,mi->m", u, P - Q)
    H = W2[:, None, None] * (lam * jG[:, :, None] * jG[:, None, :] + (1.0 - lam) * jC[:, :, None] * jC[:, None, :])
    g = W2[:, None] * (lam * jG * rG[:, None] + (1.0 - lam) * jC * rC[:, None])
    return ok, H, g, jG, rG, jC, rC


def sums(p, q, n, d, di, w, lam, valid):
    """The 34 sums icp_correspond returns for colored ICP, and the sums of the absolute contributions (the scale of each sum's rounding
    error).  valid: the validity filter (record idx >= 0, finite p and q); n / d / di / w as in pair_terms."""
    p = np.asarray(p, f32)[valid]; q = np.asarray(q, f32)[valid]
    ok, H, g, *_ = pair_terms(p, q, np.asarray(n)[valid], np.asarray(d)[valid], np.asarray(di)[valid], np.asarray(w)[valid], lam)
    s = np.zeros(34); sa = np.zeros(34)
    s[0] = ok.sum(); sa[0] = s[0]
    s[1:4] = p[ok].astype(np.float64).sum(0); sa[1:4] = np.abs(p[ok].astype(np.float64)).sum(0)
    s[4:7] = q[ok].astype(np.float64).sum(0); sa[4:7] = np.abs(q[ok].astype(np.float64)).sum(0)
    for t, (i, j) in enumerate(TRIU):
        s[7 + t] = H[:, i, j].sum(); sa[7 + t] = np.abs(H[:, i, j]).sum()
    s[28:34] = g.sum(0); sa[28:34] = np.abs(g).sum(0)
    return s, sa


def record_sums(ctx_recs, pose, src, tgt, tgt_n, grad, src_rgba, tgt_rgba, lam):
    """sums() on a list of records (idx, weight per source point, original order) at `pose`."""
    p = transform(pose, src)
    idx = np.asarray(ctx_recs["idx"]); j = np.maximum(idx, 0)
    q = np.asarray(tgt, f32)[j]
    valid = (idx >= 0) & np.isfinite(p).all(1) & np.isfinite(q).all(1)
    di = intensity_diff(src_rgba, np.asarray(tgt_rgba)[j])
    return sums(p, q, np.asarray(tgt_n, f32)[j], np.asarray(grad, f32)[j], di, ctx_recs["weight"], lam, valid)


def step(pose, src, tgt, tgt_n, grad, src_rgba, tgt_rgba, w, lam, lstsq=False):
    """One colored ICP iteration on given correspondences src[i] <-> tgt[i] (grad: the gradients of those target points): the new fp32
    pose and the sums.  lstsq: the minimum-norm step (for lambda = 1, whose H is singular on a plane)."""
    p = transform(pose, src)
    valid = np.isfinite(p).all(1) & np.isfinite(np.asarray(tgt, f32)).all(1)
    di = intensity_diff(src_rgba, tgt_rgba)
    s, _ = sums(p, tgt, tgt_n, grad, di, w, lam, valid)
    if lstsq:
        H, g = unpack(s)
        x = np.linalg.lstsq(H, g, rcond=1e-10)[0]
    else:
        x = solve(s)
    return compose(x, pose), s


def textured_plane(seed=0, n_src=20000, pitch=0.005):
    """The capability fixture: a 1 m x 1 m target plane (z = 0, normals +z) at `pitch` with a smooth uint8 grey texture, and `n_src`
    jittered points of the same plane and texture moved by T^-1 (T: 2 deg of yaw and (3 cm, -2 cm, 0)).  Aligning the source onto the
    target recovers T.  Returns dict(src_pts, src_nrm, src_rgba, tgt_pts, tgt_nrm, tgt_rgba, gt=T)."""
    def tex(x, y):
        t = 0.5 + 0.25 * np.sin(2 * np.pi * x / 0.2) + 0.2 * np.cos(2 * np.pi * (0.6 * x + y) / 0.15)
        g = np.clip(np.round(255.0 * t), 0, 255).astype(np.uint8)
        return np.stack([g, g, g, np.full_like(g, 255)], 1)
    ax = np.arange(-0.5, 0.5 + 1e-9, pitch)
    X, Y = np.meshgrid(ax, ax, indexing="ij")
    tp = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1)
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.42, 0.42, size=(n_src, 2))
    wp = np.stack([w[:, 0], w[:, 1], np.zeros(n_src)], 1)
    a = np.deg2rad(2.0)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = (0.03, -0.02, 0.0)
    Ti = np.linalg.inv(T)
    sp = wp @ Ti[:3, :3].T + Ti[:3, 3]
    nz = np.tile(np.array([0.0, 0.0, 1.0], f32), (len(tp), 1))
    return dict(src_pts=sp.astype(f32), src_nrm=np.tile(np.array([0.0, 0.0, 1.0], f32), (n_src, 1)), src_rgba=tex(w[:, 0], w[:, 1]),
                tgt_pts=tp.astype(f32), tgt_nrm=nz, tgt_rgba=tex(tp[:, 0], tp[:, 1]), gt=T)
