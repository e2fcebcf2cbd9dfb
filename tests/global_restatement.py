"""Numpy restatement of global registration as include/icp_hip.h states it (icp_global_options): the neighbour lists, the fp64 pair
features and their bins, the integer SPFH, the FPFH rows (fp64 sums, one rounding to fp32), the 33-D matcher (a sequential fp32 loop over
the bins, lowest index on ties), the RANSAC draws, statuses, three-point fit (numpy.linalg.svd), fp32 scoring and ranking.  Written from
the contract alone, so that the device's results can be compared with it -- exactly where the contract pins every rounding."""
import numpy as np

from nss_restatement import select_hash

BINS, DIM = 11, 33
VALID, REPEATED, EDGES, DEGENERATE = 0, 1, 2, 3


def neighbour_lists(pts, k, rows=None):
    """(idx (n, k) int32, d2 (n, k) float32): the k smallest (fp32 d2, index) pairs over the finite points, the point itself included, in
    ascending order; unfilled slots (-1, inf); a non-finite point has none.  d2 = (dx dx + dy dy) + dz dz in fp32.  rows: the lists of
    these points only, (len(rows), k) -- the rows of the full call."""
    p = np.asarray(pts, np.float32)
    n = len(p)
    fin = np.isfinite(p).all(axis=1)
    ids = np.flatnonzero(fin)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    idx = np.full((len(rows), k), -1, np.int32); d2 = np.full((len(rows), k), np.inf, np.float32)
    q = p[ids]
    for r, i in enumerate(rows):
        if not fin[i]:
            continue
        dx = p[i, 0] - q[:, 0]; dy = p[i, 1] - q[:, 1]; dz = p[i, 2] - q[:, 2]
        d = (dx * dx + dy * dy) + dz * dz
        cand = np.flatnonzero(d <= np.partition(d, k - 1)[k - 1]) if len(d) > k else np.arange(len(d))      # (the k-th smallest and its ties)
        order = cand[np.lexsort((ids[cand], d[cand]))][:k]
        idx[r, :len(order)] = ids[order]; d2[r, :len(order)] = d[order]
    return idx, d2


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _bin(x, lo, hi):
    t = 11.0 * (x - lo) / (hi - lo)
    b = np.clip(np.floor(t), 0, 10)
    margin = np.abs(t - np.clip(np.round(t), 1, 10))          # distance to the nearest boundary between two bins, in bin units
    return b, margin


def pair_features(p, n_p, q, n_q):
    """Arrays of pairs (fp32 inputs).  Returns dict(ok, bins (.., 3) int, margin (..): the smallest distance of f1, f2, f3 to a bin boundary
    in bin units, gap (..): ||a1| - |a2||, inf between bit-equal normals); fp64 throughout."""
    with np.errstate(all="ignore"):
        p = np.asarray(p, np.float32); q = np.asarray(q, np.float32); n_p = np.asarray(n_p, np.float32); n_q = np.asarray(n_q, np.float32)
        fin = np.isfinite(p).all(-1) & np.isfinite(q).all(-1) & np.isfinite(n_p).all(-1) & np.isfinite(n_q).all(-1)
        dp = q.astype(np.float64) - p.astype(np.float64)
        n1 = n_p.astype(np.float64); n2 = n_q.astype(np.float64)
        f4 = np.sqrt(_dot(dp, dp))
        a1 = _dot(n1, dp) / f4; a2 = _dot(n2, dp) / f4
        sw = np.abs(a1) < np.abs(a2)
        n1s = np.where(sw[..., None], n2, n1); n2s = np.where(sw[..., None], n1, n2)
        dps = np.where(sw[..., None], -dp, dp)
        f3 = np.where(sw, -a2, a1)
        v = _cross(dps, n1s)
        vn = np.sqrt(_dot(v, v))
        ok = fin & (vn > 0.0)
        v = v / vn[..., None]
        w = _cross(n1s, v)
        f1 = _dot(v, n2s)
        f2 = np.arctan2(_dot(w, n2s), _dot(n1s, n2s))
        b1, m1 = _bin(f1, -1.0, 1.0); b2, m2 = _bin(f2, -np.pi, np.pi); b3, m3 = _bin(f3, -1.0, 1.0)
        bins = np.stack([b1, b2, b3], axis=-1)
        bins = np.where(ok[..., None], bins, 0).astype(np.int64)
        margin = np.where(ok, np.minimum(m1, np.minimum(m2, m3)), np.inf)
        # (bit-equal normals: a1 and a2 are one expression of the same operands, so |a1| < |a2| is false whatever the rounding -- no gap to fall into)
        gap = np.where(fin & ~(n_p == n_q).all(-1), np.abs(np.abs(a1) - np.abs(a2)), np.inf)
    return dict(ok=ok, bins=bins, margin=margin, gap=gap)


def spfh(pts, nrm, nb_idx, nb_d2, rows=None):
    """(counts (n, 33) uint8, pairs (n,) int32, margin (n,), gap (n,)): the SPFH of every point from its neighbour list, and per point the
    smallest bin-boundary distance / ||a1| - |a2|| over its pairs (inf: no pair).  rows: nb_idx / nb_d2 are the lists of these points
    only, and so are the results -- the rows of the full call."""
    p = np.asarray(pts, np.float32); nr = np.asarray(nrm, np.float32)
    n, k = nb_idx.shape
    own = np.arange(len(p)) if rows is None else np.asarray(rows, np.int64)
    assert len(own) == n
    use = (nb_idx >= 0) & (nb_d2 > 0)
    j = np.where(use, nb_idx, 0)
    f = pair_features(p[own][:, None, :], nr[own][:, None, :], p[j], nr[j])
    ok = f["ok"] & use
    counts = np.zeros((n, DIM), np.int64)
    at = np.repeat(np.arange(n), k).reshape(n, k)
    for feat in range(3):
        np.add.at(counts, (at[ok], feat * BINS + f["bins"][..., feat][ok]), 1)
    margin = np.where(ok, f["margin"], np.inf).min(axis=1)
    gap = np.where(ok, f["gap"], np.inf).min(axis=1)
    return counts.astype(np.uint8), ok.sum(axis=1).astype(np.int32), margin, gap


def fpfh(pts, nrm, nb_idx, nb_d2, counts, pairs, stride=1):
    """(nk, 33) float32: F = h(p) + sum_i w_i h(q_i) for the keypoints 0, stride, 2 stride, ...; fp64 sums in the stored neighbour order."""
    p = np.asarray(pts, np.float32); nr = np.asarray(nrm, np.float32)
    n, k = nb_idx.shape
    key = np.arange(0, n, stride)
    h = counts.astype(np.float64) / np.maximum(pairs, 1).astype(np.float64)[:, None]
    ni = nb_idx[key]; nd = nb_d2[key]
    use = (ni >= 0) & (nd > 0)
    with np.errstate(all="ignore"):
        inv = np.where(use, 1.0 / np.sqrt(np.where(use, nd, 1).astype(np.float64)), 0.0)
        S = np.zeros(len(key))
        for q in range(k):
            S = np.where(use[:, q], S + inv[:, q], S)
        acc = h[key].copy()
        for q in range(k):
            w = inv[:, q] / S
            term = w[:, None] * h[np.where(use[:, q], ni[:, q], 0)]
            acc = np.where(use[:, q, None], acc + term, acc)
    out = acc.astype(np.float32)
    bad = ~(np.isfinite(p[key]).all(axis=1) & np.isfinite(nr[key]).all(axis=1) & (pairs[key] > 0))
    out[bad] = np.nan
    return out


def features(pts, nrm, k, stride=1):
    """The whole feature pass: dict(idx, d2, counts, pairs, margin, gap, F)."""
    idx, d2 = neighbour_lists(pts, k)
    counts, pairs, margin, gap = spfh(pts, nrm, idx, d2)
    return dict(idx=idx, d2=d2, counts=counts, pairs=pairs, margin=margin, gap=gap, F=fpfh(pts, nrm, idx, d2, counts, pairs, stride))


def match_rows(Q, T, with_second=False):
    """For every row of Q the row of T with the smallest d = sum_b (a_b - c_b)^2 -- fp32, the bins in order -- the lowest index on ties, -1
    when there is none (NaN rows never match and are never matched).  with_second: also (d_best, d_second)."""
    Q = np.asarray(Q, np.float32); T = np.asarray(T, np.float32)
    out = np.full(len(Q), -1, np.int64); best = np.full(len(Q), np.inf, np.float32); second = np.full(len(Q), np.inf, np.float32)
    if len(T) == 0:
        return (out, best, second) if with_second else out
    with np.errstate(all="ignore"):
        for s in range(0, len(Q), 256):
            q = Q[s:s + 256]
            d = np.zeros((len(q), len(T)), np.float32)
            for b in range(DIM):
                e = q[:, b, None] - T[None, :, b]
                d = d + e * e
            d = np.where(np.isnan(d), np.float32(np.inf), d)
            j = np.argmin(d, axis=1)                               # the first minimum: the lowest index
            m = d[np.arange(len(q)), j]
            out[s:s + 256] = np.where(np.isfinite(m), j, -1); best[s:s + 256] = m
            if len(T) > 1:
                second[s:s + 256] = np.partition(d, 1, axis=1)[:, 1]
    return (out, best, second) if with_second else out


def correspondences(Fs, Ft, stride=1, mutual=True):
    """(src_idx, tgt_idx): original point indices of the kept pairs, ascending in src_idx."""
    fwd = match_rows(Fs, Ft)
    keep = fwd >= 0
    if mutual:
        back = match_rows(Ft, Fs)
        keep &= back[np.where(keep, fwd, 0)] == np.arange(len(Fs))
    r = np.flatnonzero(keep)
    return (r * stride).astype(np.int32), (fwd[r] * stride).astype(np.int32)


def draws(seed, H, M):
    """(H, 3) int64: c_j = select_hash(seed, h, j) mod M."""
    out = np.zeros((H, 3), np.int64)
    for h in range(H):
        out[h] = select_hash(seed, h, np.arange(3)).astype(np.int64) % M
    return out


def _collinear(p):
    a = p[:, 1] - p[:, 0]; b = p[:, 2] - p[:, 0]
    c = _cross(a, b)
    return ~(_dot(c, c) > 1e-6 * (_dot(a, a) * _dot(b, b)))


def ransac_fit(cs, ct, dr, edge_similarity):
    """status (H,) and poses (H, 16) float32 column-major (identity unless VALID) of the hypotheses with draws dr over the pairs (cs, ct)."""
    s = np.asarray(cs, np.float32)[dr].astype(np.float64); t = np.asarray(ct, np.float32)[dr].astype(np.float64)      # (H, 3, 3)
    H = len(dr)
    status = np.full(H, VALID, np.int32)
    rep = (dr[:, 0] == dr[:, 1]) | (dr[:, 1] == dr[:, 2]) | (dr[:, 0] == dr[:, 2])
    es = np.float64(np.float32(edge_similarity))
    bad_edge = np.zeros(H, bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ds = s[:, b] - s[:, a]; dt = t[:, b] - t[:, a]
        ls = np.sqrt(_dot(ds, ds)); lt = np.sqrt(_dot(dt, dt))
        bad_edge |= ~(np.minimum(ls, lt) >= es * np.maximum(ls, lt))
    deg = _collinear(s) | _collinear(t)
    status[deg] = DEGENERATE; status[bad_edge] = EDGES; status[rep] = REPEATED
    poses = np.tile(np.eye(4, dtype=np.float32).T.reshape(16), (H, 1))
    v = np.flatnonzero(status == VALID)
    if len(v):
        sv, tv = s[v], t[v]
        sm = ((sv[:, 0] + sv[:, 1]) + sv[:, 2]) / 3.0; tm = ((tv[:, 0] + tv[:, 1]) + tv[:, 2]) / 3.0
        A = np.einsum("hjr,hjc->hrc", tv - tm[:, None], sv - sm[:, None])
        U, _, Vt = np.linalg.svd(A)
        d = np.linalg.det(U @ Vt)
        D = np.tile(np.eye(3), (len(v), 1, 1)); D[:, 2, 2] = d
        R = U @ D @ Vt
        tr = tm - np.einsum("hrc,hc->hr", R, sm)
        P = np.tile(np.eye(4), (len(v), 1, 1)); P[:, :3, :3] = R; P[:, :3, 3] = tr
        poses[v] = P.transpose(0, 2, 1).reshape(len(v), 16).astype(np.float32)
    return status, poses


def ransac_score(poses16, status, cs, ct, inlier_distance):
    """(n_inliers (H,) int32, sum_d2 (H,) float64) of the VALID hypotheses (0 elsewhere): fp32 transform and d2, fp64 sum."""
    P = np.asarray(poses16, np.float32); s = np.asarray(cs, np.float32); t = np.asarray(ct, np.float32)
    thr = np.float32(inlier_distance) * np.float32(inlier_distance)
    n = np.zeros(len(P), np.int32); sums = np.zeros(len(P), np.float64)
    x, y, z = s[None, :, 0], s[None, :, 1], s[None, :, 2]
    for lo in range(0, len(P), 512):
        p = P[lo:lo + 512]
        mv = [((p[:, r, None] * x + p[:, 4 + r, None] * y) + p[:, 8 + r, None] * z) + p[:, 12 + r, None] for r in range(3)]
        dx = mv[0] - t[None, :, 0]; dy = mv[1] - t[None, :, 1]; dz = mv[2] - t[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        inl = (d2 <= thr) & (status[lo:lo + 512, None] == VALID)
        n[lo:lo + 512] = inl.sum(axis=1)
        sums[lo:lo + 512] = np.where(inl, d2.astype(np.float64), 0.0).sum(axis=1)
    return n, sums


def ranking(status, n_inliers, sum_d2):
    """The valid hypotheses, best first: more inliers, then the smaller sum, then the lower h."""
    v = np.flatnonzero(np.asarray(status) == VALID)
    return v[np.lexsort((v, np.asarray(sum_d2)[v], -np.asarray(n_inliers, np.int64)[v]))]


def ransac(cs, ct, seed, H, edge_similarity, inlier_distance):
    """The whole RANSAC pass over the pairs (cs, ct): dict(draws, status, poses, n_inliers, sum_d2, order)."""
    dr = draws(seed, H, len(cs))
    status, poses = ransac_fit(cs, ct, dr, edge_similarity)
    n, sums = ransac_score(poses, status, cs, ct, inlier_distance)
    return dict(draws=dr, status=status, poses=poses, n_inliers=n, sum_d2=sums, order=ranking(status, n, sums))
