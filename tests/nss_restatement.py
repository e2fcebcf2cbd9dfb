"""Numpy restatement of normal-space sampling (params.selection = ICP_SELECT_NORMAL_SPACE) as include/icp_hip.h states it: the bucket of
a source point, the water-filled quotas, the draw of one iteration, the lists of a whole run.  Written from the contract alone, fp32
where the contract says fp32, so that the device's buckets and index lists can be compared with it exactly."""
import numpy as np

NONE = 0xFFFF
M32 = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    h = h & M32
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def select_hash(seed, iteration, index):
    """icp_select_hash, vectorised over `index` (uint32 arithmetic carried in uint64)."""
    index = np.asarray(index, dtype=np.uint64) & M32
    inner = _fmix32(np.uint64((int(seed) + int(iteration) * 0x7F4A7C15 + 0x165667B1) & 0xFFFFFFFF))
    return _fmix32((index * np.uint64(0x9E3779B9) + inner) & M32).astype(np.uint32)


def buckets(pts, nrm, grid):
    """uint16 bucket of every point (NONE: no bucket), every operation in fp32."""
    p = np.asarray(pts, np.float32); n = np.asarray(nrm, np.float32)
    g = np.float32(grid)
    with np.errstate(all="ignore"):
        a = np.abs(n)
        m = np.maximum(a[:, 0], np.maximum(a[:, 1], a[:, 2]))
        ok = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1) & (m != 0)
        axis = np.where(a[:, 0] == m, 0, np.where(a[:, 1] == m, 1, 2))
        rows = np.arange(len(n))
        na = n[rows, axis]
        u = np.where(axis == 0, n[:, 1], n[:, 0]) / m
        v = np.where(axis == 2, n[:, 1], n[:, 2]) / m
        half = np.float32(0.5) * g

        def cell(t):
            c = np.floor((t + np.float32(1.0)) * half)
            return np.minimum(grid - 1, np.where(np.isfinite(c), c, 0).astype(np.int64))
        face = 2 * axis + (na < 0)
        b = face * grid * grid + cell(v) * grid + cell(u)
    return np.where(ok, b, NONE).astype(np.uint16)


def base_set(pts, nrm, factor):
    """The base set of a decimation factor (RANDOM_SAMPLING's): every point for factor 0, else every factor-th point that is finite in
    point and normal (PointCloud::getCoarseResolution)."""
    n = len(pts)
    if factor == 0:
        return np.arange(n, dtype=np.int64)
    idx = np.arange(0, n, factor, dtype=np.int64)
    ok = np.isfinite(np.asarray(pts, np.float32)[idx]).all(axis=1) & np.isfinite(np.asarray(nrm, np.float32)[idx]).all(axis=1)
    return idx[ok]


def sample_size(proba, m):
    v = float(np.float32(proba)) * float(m)
    if m <= 0 or not v > 0.0:
        return 0
    return m if v >= m else int(np.ceil(v))


def quotas(cnt, M, seed, iteration):
    """(q, c): the quota of every bucket and the water-filling cap."""
    cnt = np.asarray(cnt, np.int64)
    if M <= 0:
        return np.zeros_like(cnt), 0
    c = 1
    while np.minimum(cnt, c).sum() < M:
        c += 1
    q = np.minimum(cnt, c)
    E = int(q.sum() - M)
    capped = np.nonzero(cnt >= c)[0]
    keys = select_hash(seed, iteration, np.uint64(0x80000000) | capped.astype(np.uint64))
    q[capped[np.argsort(keys, kind="stable")[:E]]] -= 1
    return q, c


def draw(bkt, base, proba, seed, iteration, n_buckets):
    """The index list of one draw: increasing original indices."""
    base = np.asarray(base, np.int64)
    cand = base[bkt[base] != NONE]
    b = bkt[cand].astype(np.int64)
    cnt = np.bincount(b, minlength=n_buckets)
    q, _ = quotas(cnt, sample_size(proba, len(cand)), seed, iteration)
    h = select_hash(seed, iteration, cand)
    out = []
    for k in np.nonzero(q)[0]:
        seg = cand[b == k]
        out.append(seg[np.argsort(h[b == k], kind="stable")[:q[k]]])
    return np.sort(np.concatenate(out)).astype(np.int32) if out else np.zeros(0, np.int32)


def run_lists(pts, nrm, factors, proba, seed, grid=5, resample=True):
    """The index list of every iteration of a run with the decimation schedule `factors` (icp_schedule)."""
    bkt = buckets(pts, nrm, grid)
    lists, first = [], {}
    for i, f in enumerate(factors):
        if not resample and f in first:
            lists.append(lists[first[f]])
            continue
        first.setdefault(f, i)
        lists.append(draw(bkt, base_set(pts, nrm, f), proba, seed, i, 6 * grid * grid))
    return lists
