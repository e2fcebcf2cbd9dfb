"""numpy restatement of reciprocal (mutual nearest-neighbour) correspondence rejection, written from the contract in include/icp_hip.h and
DESIGN.md (section 6l).  fp32 with one rounding per operation, the contract's operation order, a brute-force lexicographic argmin: no tree.
Test infrastructure only.

  to_source_frame(pose, t)               q = R^T (t - T) in the contract's operation order
  d2_f32(q, s)                           ((dx dx + dy dy) + dz dz) in fp32, d = q - s
  mutual(q, i, src)                      per query: no finite source point j has (d2(j), j) < (d2(i), i)
  reciprocal(recs, pose, src, tgt, ...)  the filtered records and the icp_reciprocal_stats record of one iteration
  mutual_fp64(pose, src, tgt, idx)       the plain fp64 mutual test in the target's frame (for well-separated points)
  icp(...)                               a small point-to-plane ICP loop with a brute-force matcher (fixture selection)
"""
import numpy as np

f32 = np.float32
MATCH_DTYPE = np.dtype([("idx", np.int32), ("weight", f32)])


def to_source_frame(pose, t):
    """pose: 4x4 (row, col); t: (m, 3) target points.  d = t - P[12..14]; q_x = (P[0] d_x + P[1] d_y) + P[2] d_z, q_y with P[4..6], q_z with
    P[8..10], P column-major: the transpose of the 3x3 block applied to d."""
    P = np.ascontiguousarray(np.asarray(pose, f32).T).reshape(16)
    t = np.asarray(t, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d0, d1, d2 = (t[:, 0] - P[12]).astype(f32), (t[:, 1] - P[13]).astype(f32), (t[:, 2] - P[14]).astype(f32)
        q = [((P[4 * r] * d0 + P[4 * r + 1] * d1).astype(f32) + P[4 * r + 2] * d2).astype(f32) for r in range(3)]
    return np.stack(q, 1)


def d2_f32(q, s):
    """(dx dx + dy dy) + dz dz in fp32 with dx = q_x - s_x (broadcasting over the leading axes)."""
    with np.errstate(all="ignore"):
        e = (np.asarray(q, f32) - np.asarray(s, f32)).astype(f32)
        return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]).astype(f32) + e[..., 2] * e[..., 2]).astype(f32)


def mutual(q, i, src, chunk_elems=1 << 22):
    """q: (m, 3) target points in the source's frame; i: (m,) the original source index of each pair; src: the full-resolution source.
    True where no finite source point j has d2(j) < d2(i), or d2(j) == d2(i) with j < i.  Brute force over all of src, in chunks of queries."""
    q = np.asarray(q, f32).reshape(-1, 3); i = np.asarray(i, np.int64); src = np.asarray(src, f32).reshape(-1, 3)
    fin = np.isfinite(src).all(1)
    j = np.arange(len(src), dtype=np.int64)
    out = np.ones(len(q), bool)
    step = max(1, chunk_elems // max(len(src), 1))
    for a in range(0, len(q), step):
        qa, ia = q[a:a + step], i[a:a + step]
        di = d2_f32(qa, src[ia])[:, None]
        D = d2_f32(qa[:, None, :], src[None, :, :])
        with np.errstate(invalid="ignore"):
            rival = ((D < di) | ((D == di) & (j[None, :] < ia[:, None]))) & fin[None, :]
        out[a:a + step] = ~rival.any(1)
    return out


def mutual_by_nearest(q, i, src, nearest):
    """The same decision from an exact nearest-neighbour engine: nearest(q) -> the (d2, lowest index) argmin over the finite source points
    with the contract's d2, or -1.  A pair is mutual iff that argmin is i; queries the engine has no answer for (no finite d2), and pairs
    whose own d2 is not finite, go through the brute force."""
    q = np.asarray(q, f32).reshape(-1, 3); i = np.asarray(i, np.int64)
    j = np.asarray(nearest(q), np.int64)
    out = j == i
    di = d2_f32(q, np.asarray(src, f32)[i])
    odd = (j < 0) | ~np.isfinite(di)
    if odd.any():
        out[odd] = mutual(q[odd], i[odd], src)
    return out


def reciprocal(recs, pose, src, tgt, orig=None, nearest=None):
    """recs: the matcher's records of an iteration's queries (idx < 0: unmatched); orig: the original source index of every query (default:
    its position); src / tgt: the full-resolution clouds.  Returns the filtered records ({-1, 0} where a judged pair is not mutual), the
    stats record and the judged / mutual masks."""
    recs = np.asarray(recs)
    orig = np.arange(len(recs), dtype=np.int64) if orig is None else np.asarray(orig, np.int64)
    judged = recs["idx"] >= 0
    q = to_source_frame(pose, np.asarray(tgt, f32)[recs["idx"][judged]])
    keep = mutual(q, orig[judged], src) if nearest is None else mutual_by_nearest(q, orig[judged], src, nearest)
    out = np.array(recs, dtype=MATCH_DTYPE)
    mut = np.zeros(len(recs), bool); mut[judged] = keep
    drop = judged & ~mut
    out["idx"][drop] = -1; out["weight"][drop] = 0.0
    return dict(recs=out, stats=dict(n_matched=int(judged.sum()), n_mutual=int(keep.sum())), judged=judged, mutual=mut)


def mutual_fp64(pose, src, tgt, idx):
    """The plain mutual test in the target's frame, fp64: pair (i, idx[i]) is mutual iff source i is the nearest transformed source point to
    target idx[i].  For well-separated points only (no ties, no rounding-sized margins)."""
    T = np.asarray(pose, np.float64); s = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]
    t = np.asarray(tgt, np.float64)
    out = np.zeros(len(idx), bool)
    for i, j in enumerate(idx):
        if j >= 0:
            out[i] = int(np.argmin(((s - t[j]) ** 2).sum(1))) == i
    return out


def match_brute(p, tgt, max_distance):
    """The library's matcher on transformed points p: the (fp32 d2, lowest index) argmin over the finite targets, kept when d2 <= max_distance."""
    tgt = np.asarray(tgt, f32)
    D = d2_f32(np.asarray(p, f32)[:, None, :], tgt[None, :, :])
    D = np.where(np.isfinite(tgt).all(1)[None, :], D, np.inf)
    D = np.where(np.isnan(D), np.inf, D)
    j = np.argmin(D, 1)                                      # (first minimum: the lowest index)
    d = D[np.arange(len(p)), j]
    recs = np.zeros(len(p), MATCH_DTYPE)
    ok = d <= f32(max_distance)
    recs["idx"] = np.where(ok, j, -1); recs["weight"] = np.where(ok, 1.0, 0.0)
    return recs


def icp(src, tgt, tgt_nrm, max_distance, n_iterations, use_reciprocal, pose=None):
    """Point-to-plane ICP with the brute-force matcher, constant weights, no rejection, the restatement's reciprocal filter when asked, and the
    point-to-plane sums / solve / composition of the other restatements.  Returns the final pose and the kept fraction per iteration."""
    import gicp_restatement as G
    import robust_restatement as R
    pose = np.eye(4, dtype=f32) if pose is None else np.asarray(pose, f32)
    kept = []
    for _ in range(n_iterations):
        p = G.transform(pose, src)
        recs = match_brute(p, tgt, max_distance)
        if use_reciprocal:
            r = reciprocal(recs, pose, src, tgt)
            kept.append(r["stats"]["n_mutual"] / max(r["stats"]["n_matched"], 1))
            recs = r["recs"]
        s, _ = R.sums(1, p, tgt, recs, tgt_nrm=tgt_nrm)
        pose = G.compose(G.solve(s), pose)
    return pose, kept
