"""numpy restatement of trimmed ICP and the robust kernels, written from the contract in DESIGN.md (section 6f) and include/icp_hip.h.
Test infrastructure only.

  keys(idx, p, q)                        the r^2 key of every record (SKIP where the pair does not enter) and the entering mask
  select(keys, overlap)                  m, K, ceil(K/2), t, med and M by sorting
  scale(sigma_opt, med)                  sigma: the fixed one or 1.4826 sqrt(med), fp64
  rho(kernel, c, sigma, r2)              the robust factor, fp64, the contract's operation order
  apply(recs, keys, ...)                 the final records (trimmed: idx -1; kept: reweighted)
  robust(recs, p, q, opt, metric)        all of the above in one call, with the icp_robust_stats record
  sums(metric, p, q, recs, ...)          the 34 fp64 sums of icp_correspond on given records, and their absolute sums
  step(...)                              one point-to-plane ICP step with a nearest-neighbour matcher (the partial-overlap fixture)
"""
import numpy as np

import gicp_restatement as G

f32 = np.float32
SKIP = np.uint32(0xFFFFFFFF)
NONE, HUBER, CAUCHY, TUKEY = 0, 1, 2, 3
STANDARD = {NONE: 0.0, HUBER: 1.345, CAUCHY: 2.3849, TUKEY: 4.6851}


def r2_f32(p, q):
    """((e0*e0 + e1*e1) + e2*e2) in fp32, e = p - q, one rounding per operation."""
    e = (np.asarray(p, f32) - np.asarray(q, f32)).astype(f32)
    with np.errstate(over="ignore"):
        return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(f32)


def keys(idx, p, q):
    """idx: the records' indices after weighting and rejection; p: transformed source points; q: target points of the records (any row
    where idx < 0).  A pair enters when idx >= 0 and p, q are finite."""
    idx = np.asarray(idx)
    ent = (idx >= 0) & np.isfinite(p).all(1) & np.isfinite(q).all(1)
    k = np.full(len(idx), SKIP, np.uint32)
    k[ent] = r2_f32(np.asarray(p)[ent], np.asarray(q)[ent]).view(np.uint32)
    return k, ent


def select(k, overlap):
    """(m, K, Kmed, t, med, M) of the keys (t, med as uint32 patterns; None when m = 0)."""
    v = np.sort(k[k != SKIP])
    m = len(v)
    if m == 0:
        return 0, 0, 0, None, None, 0
    K = int(min(max(np.ceil(np.float64(np.float32(overlap)) * m), 1), m))
    Km = (K + 1) // 2
    t, med = v[K - 1], v[Km - 1]
    return m, K, Km, t, med, int(np.count_nonzero(v <= t))


def tuning(kernel, c):
    """c as the device uses it: the float option, or the kernel's standard constant rounded to fp32."""
    c = float(np.float32(c))
    return float(np.float32(STANDARD[kernel])) if c == 0.0 else c


def scale(sigma_opt, med):
    s = float(np.float32(sigma_opt))
    return s if s > 0 else 1.4826 * np.sqrt(np.float64(np.uint32(med).view(f32)))


def rho(kernel, c, sigma, r2):
    r2 = np.asarray(r2, f32)
    if kernel == NONE or sigma == 0.0 or np.isinf(sigma):
        return np.ones(r2.shape, np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        u = np.sqrt(r2.astype(np.float64)) / sigma
        q = u / c
        if kernel == HUBER:
            return np.where(u <= c, 1.0, c / u)
        if kernel == CAUCHY:
            return 1.0 / (1.0 + q * q)
        return np.where(u < c, (1.0 - q * q) * (1.0 - q * q), 0.0)


def apply(recs, k, t, kernel, c, sigma, metric):
    out = recs.copy()
    if t is None:
        return out
    ent = k != SKIP
    trim = ent & (k > t)
    out["idx"][trim] = -1
    keep = ent & ~trim
    if kernel != NONE and keep.any():
        r = rho(kernel, c, sigma, k[keep].view(f32))
        w = recs["weight"][keep].astype(np.float64)
        out["weight"][keep] = (w * r if metric == 0 else w * np.sqrt(r)).astype(f32)
    return out


def robust(recs, p, tgt, opt, metric):
    """recs: robust-off records (after weighting and rejection); p: transformed source points; tgt: target xyz.  opt: dict(kernel, tuning,
    sigma, overlap).  Returns dict(keys, m, K, Kmed, t, med, M, sigma, recs, stats)."""
    q = np.asarray(tgt, f32)[np.maximum(recs["idx"], 0)]
    k, ent = keys(recs["idx"], p, q)
    kern = int(opt.get("kernel", 0))
    m, K, Km, t, med, M = select(k, opt.get("overlap", 1.0))
    sig = scale(opt.get("sigma", 0.0), med) if m else 0.0
    c = tuning(kern, opt.get("tuning", 0.0))
    fin = apply(recs, k, t, kern, c, sig, metric)
    st = dict(n_entering=m, n_kept=M, trim_d2=float(np.uint32(t).view(f32)) if m else -1.0,
              sigma=float(np.float32(sig)) if (m and kern != NONE) else -1.0)
    return dict(keys=k, entering=ent, m=m, K=K, Kmed=Km, t=t, med=med, M=M, sigma=sig, c=c, recs=fin, stats=st)


def _rows(kind, s, d, n, w):
    """(n, 4, 7) fp32 rows of build_rows (dev_post.hpp): row 0 dense, rows 1-3 the point rows, scaled by w and 0.1 w."""
    s = s.astype(f32); d = d.astype(f32); n = n.astype(f32); w = w.astype(f32)
    s0, s1, s2 = s[:, 0], s[:, 1], s[:, 2]; d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]; n0, n1, n2 = n[:, 0], n[:, 1], n[:, 2]
    if kind == 0:
        A = [n2 * s1 - n1 * s2, n0 * s2 - n2 * s0, n1 * s0 - n0 * s1]
        b0 = ((n0 * d0 + n1 * d1) + n2 * d2) - ((n0 * s0 + n1 * s1) + n2 * s2)
    else:
        e0, e1, e2 = s0 + d0, s1 + d1, s2 + d2
        g0, g1, g2 = d0 - s0, d1 - s1, d2 - s2
        A = [e1 * n2 - e2 * n1, e2 * n0 - e0 * n2, e0 * n1 - e1 * n0]
        b0 = g0 * n0 + (g1 * n1 + g2 * n2)
    f0 = f32(1.0) * w; f1 = f32(0.1) * w
    R = np.zeros((len(s), 4, 7), f32)
    for c_, a in enumerate(A + [n0, n1, n2]):
        R[:, 0, c_] = a * f0
    R[:, 0, 6] = b0 * f0
    g = f32(1.0) * f1
    R[:, 1, 1] = s2 * f1; R[:, 1, 2] = (-s1) * f1; R[:, 1, 3] = g; R[:, 1, 6] = (d0 - s0) * f1
    R[:, 2, 0] = (-s2) * f1; R[:, 2, 2] = s0 * f1; R[:, 2, 4] = g; R[:, 2, 6] = (d1 - s1) * f1
    R[:, 3, 0] = s1 * f1; R[:, 3, 1] = (-s0) * f1; R[:, 3, 5] = g; R[:, 3, 6] = (d2 - s2) * f1
    return R


def _slot_terms(R):
    R = R.astype(np.float64)
    cols = [(a, c) for a in range(6) for c in range(a, 6)] + [(a, 6) for a in range(6)]
    return np.stack([(R[:, :, a] * R[:, :, c]).sum(1) for a, c in cols], 1)        # (n, 27)


def sums(metric, p, tgt, recs, tgt_nrm=None, src_nrm_t=None, means=None, gicp=None, terms=False):
    """The 34 sums of icp_correspond for the final records: [0] n, [1..3] sum s, [4..6] sum d, [7..] the metric's block; and the sums of
    their absolute terms (the scale of a tolerance).  tgt_nrm: target normals (point-to-plane, symmetric); src_nrm_t: source normals moved
    by the pose in fp32 (symmetric); means: (mean s, mean d) fp32 of the symmetric pass (default: from these records); gicp: dict(a, b, eps)
    (GICP normals of the targets of the records and of the moved sources; sums from tests/gicp_restatement.py).  terms=True (not GICP): also
    the (n_valid, 34) fp64 terms the sums are folded from, one row per valid pair, and the positions of those pairs."""
    p = np.asarray(p, f32)
    idx = recs["idx"]; j = np.maximum(idx, 0)
    q = np.asarray(tgt, f32)[j]
    valid = (idx >= 0) & np.isfinite(p).all(1) & np.isfinite(q).all(1)
    w = recs["weight"]
    if metric == 3:
        return G.sums(p, q, gicp["a"], gicp["b"], w, gicp["eps"], valid)
    s, d, wv = p[valid], q[valid], w[valid]
    T = [np.ones((len(s), 1)), s.astype(np.float64), d.astype(np.float64)]
    if metric == 0:
        wd = wv.astype(np.float64)[:, None]
        ws = wd * s.astype(np.float64)
        T += [wd, ws, wd * d.astype(np.float64), (d.astype(np.float64)[:, :, None] * ws[:, None, :]).reshape(len(s), 9)]
    elif metric == 1:
        T.append(_slot_terms(_rows(0, s, d, np.asarray(tgt_nrm, f32)[j][valid], wv)))
    else:
        n = (np.asarray(tgt_nrm, f32)[j][valid] + np.asarray(src_nrm_t, f32)[valid]).astype(f32)
        if means is None:
            means = ((s.astype(np.float64).sum(0) / len(s)).astype(f32), (d.astype(np.float64).sum(0) / len(s)).astype(f32))
        ms, md = np.asarray(means[0], f32), np.asarray(means[1], f32)
        T.append(_slot_terms(_rows(1, (s - ms).astype(f32), (d - md).astype(f32), n, wv)))
    X = np.concatenate(T, 1)
    out = np.zeros(34); ab = np.zeros(34)
    out[:X.shape[1]] = X.sum(0); ab[:X.shape[1]] = np.abs(X).sum(0)
    if terms:
        Xp = np.zeros((len(X), 34)); Xp[:, :X.shape[1]] = X
        return out, ab, Xp, np.flatnonzero(valid)
    return out, ab


def step(pose, src, src_n, tgt, tgt_n, tree, max_distance, opt, weighting=0):
    """One point-to-plane iteration (matcher: nearest neighbour within max_distance in fp64; constant weights; no rejection), robust mode
    as opt, then the point-to-plane solve and composition.  Returns the new pose and the robust record."""
    p = G.transform(pose, src)
    dist, j = tree.query(p.astype(np.float64), k=1)
    idx = np.where(dist * dist <= max_distance, j, -1).astype(np.int32)
    recs = np.zeros(len(src), dtype=[("idx", np.int32), ("weight", f32)])
    recs["idx"] = idx; recs["weight"] = 1.0
    r = robust(recs, p, tgt, opt, 1)
    s, _ = sums(1, p, tgt, r["recs"], tgt_nrm=tgt_n)
    return G.compose(G.solve(s), pose), r["stats"]
