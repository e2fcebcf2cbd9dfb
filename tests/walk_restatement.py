"""NumPy float32 restatements of the two steps of the shared BVH walk (icp-variants_amd/csrc/dev_bvh.hpp), vectorised over many
leaves / nodes, and the generators of the cases the tests run them on.  No GPU needed.

  leaf_update_sequential : the definition -- the strict-< scan over the 8 slots of a leaf in slot order (leaf_update_sequential in
                           dev_bvh.hpp, followed by the others_insert calls of leaf_eval).
  leaf_update_closed     : what leaf_eval does instead where no tie is involved, and its tie predicate (`rare`): where it is set the
                           device runs the scan.
  quad_bounds            : ((e0^2 + e1^2) + e2^2), e = max(max(lo - p, p - hi), 0), of the four children of a 4-wide node.

All arithmetic is IEEE float32 without contraction, in the order the device uses, so results compare bitwise."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
CATEGORIES = ("continuous", "grid2", "grid4", "seed_inside", "tie_lower_elsewhere", "tie_higher_elsewhere", "unseeded", "padded", "huge")


def leaf_distances(C, P):
    """C [n, 3, 8] leaf coordinates, P [n, 3] queries -> [n, 8] squared distances, ((e0^2 + e1^2) + e2^2)."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = (P[:, :, None] - C).astype(F)
        sq = (e * e).astype(F)
        return ((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)


def _others_insert(x, xl, b2, l2, b3, on):
    """others_insert of dev_bvh.hpp for the rows where `on` is set (in place)."""
    better = x < b2
    same = xl == l2
    nb3 = np.where(same, b3, np.minimum(b3, np.where(better, b2, x)))
    nl2 = np.where(better, xl, l2)
    nb2 = np.where(better, x, b2)
    b3[on] = nb3[on]; l2[on] = nl2[on]; b2[on] = nb2[on]


def _finish(x, moved, leaf, prev_best, prev_leaf, b2, l2, b3):
    every = np.ones(len(x), bool)
    _others_insert(x, leaf, b2, l2, b3, every)
    _others_insert(prev_best, prev_leaf, b2, l2, b3, moved)


def _scan(dd, IDX, leaf, best, bi, bpos, on):
    """The sequential scan on the rows `on` (best, bi, bpos updated in place); returns mo, the smallest distance among the leaf's points
    that do not end up as the winner."""
    n = len(dd)
    mo = np.full(n, FLT_MAX, F)
    here = (bpos >> 3) == leaf
    for t in range(8):
        d = dd[:, t]; j = IDX[:, t]
        take = ((d < best) | ((d == best) & (j < bi))) & on
        other = np.where(take, np.where(here, best, FLT_MAX), np.where(j != bi, d, FLT_MAX)).astype(F)
        mo = np.where(on, np.minimum(mo, other), mo).astype(F)
        here = here | take
        best[take] = d[take]; bi[take] = j[take]; bpos[take] = leaf[take] * 8 + t
    return mo


def leaf_update_sequential(C, IDX, P, leaf, best, bi, bpos, b2, l2, b3):
    """-> (best, bi, bpos, b2, l2, b3) after the leaf, by the scan."""
    best, b2, b3 = best.astype(F).copy(), b2.astype(F).copy(), b3.astype(F).copy()
    bi, bpos, l2 = bi.astype(np.int32).copy(), bpos.astype(np.int32).copy(), l2.astype(np.int32).copy()
    dd = leaf_distances(C, P)
    prev_leaf = bpos >> 3; prev_best = best.copy()
    m = np.minimum(dd.min(axis=1), FLT_MAX).astype(F)
    heavy = m <= best
    mo = _scan(dd, IDX, leaf, best, bi, bpos, heavy)
    x = np.where(heavy, mo, m).astype(F)
    moved = heavy & (prev_leaf != leaf) & ((bpos >> 3) == leaf)
    _finish(x, moved, leaf, prev_best, prev_leaf, b2, l2, b3)
    return best, bi, bpos, b2, l2, b3


def leaf_update_closed(C, IDX, P, leaf, best, bi, bpos, b2, l2, b3):
    """-> (best, bi, bpos, b2, l2, b3, rare): the closed form where exactly one slot is at the leaf minimum and it beats the running best
    strictly or is the running best; `rare` marks the rows with a tie, which take the scan."""
    best, b2, b3 = best.astype(F).copy(), b2.astype(F).copy(), b3.astype(F).copy()
    bi, bpos, l2 = bi.astype(np.int32).copy(), bpos.astype(np.int32).copy(), l2.astype(np.int32).copy()
    dd = leaf_distances(C, P)
    prev_leaf = bpos >> 3; prev_best = best.copy()
    srt = np.sort(dd, axis=1)
    m1, m2 = srt[:, 0], srt[:, 1]                        # smallest and second smallest, with multiplicity
    m = np.minimum(m1, FLT_MAX).astype(F)
    heavy = m <= best
    e = dd == m1[:, None]
    ts = ((e[:, 1] | e[:, 3] | e[:, 5] | e[:, 7]) * 1 + (e[:, 2] | e[:, 3] | e[:, 6] | e[:, 7]) * 2 + (e[:, 4] | e[:, 5] | e[:, 6] | e[:, 7]) * 4).astype(np.int32)
    js = np.take_along_axis(IDX, ts[:, None].astype(np.int64), axis=1)[:, 0]
    lt = m < best
    rare = heavy & ~((m2 > m1) & (lt | (js == bi)))
    fast = heavy & ~rare
    x = m.copy()
    x[fast] = np.minimum(m2, FLT_MAX).astype(F)[fast]
    take = fast & lt
    moved = take & (prev_leaf != leaf)
    best[take] = m[take]; bi[take] = js[take]; bpos[take] = (leaf * 8 + ts)[take]
    mo = _scan(dd, IDX, leaf, best, bi, bpos, rare)
    x[rare] = mo[rare]
    moved = moved | (rare & (prev_leaf != leaf) & ((bpos >> 3) == leaf))
    _finish(x, moved, leaf, prev_best, prev_leaf, b2, l2, b3)
    return best, bi, bpos, b2, l2, b3, rare


def quad_bounds(LO, HI, P):
    """LO, HI [n, 3, 4] child boxes, P [n, 3] -> [n, 4] squared lower bounds."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = P[:, :, None]
        e = np.maximum(np.maximum((LO - p).astype(F), (p - HI).astype(F)), F(0)).astype(F)
        sq = (e * e).astype(F)
        return ((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)


def leaf_cases(category, n, seed=0):
    """n leaves of 8 points with a query and the state a walk can arrive with.  Original indices are unique within a leaf (pads: -1) and
    differ from the running best's unless that lives in the leaf, in which case `best` is the distance of its slot -- what every caller of
    leaf_eval guarantees.  -> dict of C, IDX, P, leaf, best, bi, bpos, b2, l2, b3."""
    rng = np.random.default_rng([seed, CATEGORIES.index(category)])
    grid = {"grid2": 2, "grid4": 4}.get(category, 0)
    if grid:
        C = rng.integers(0, grid, (n, 3, 8)).astype(F); P = (rng.integers(0, 2 * grid, (n, 3)) * 0.5).astype(F)
    elif category == "huge":
        C = (rng.uniform(-1, 1, (n, 3, 8)) * 10.0 ** rng.uniform(17, 20, (n, 1, 1))).astype(F); P = (rng.uniform(-1, 1, (n, 3)) * 1e18).astype(F)
    else:
        C = rng.uniform(-1, 1, (n, 3, 8)).astype(F); P = rng.uniform(-1.2, 1.2, (n, 3)).astype(F)
    leaf = rng.integers(0, 1 << 16, n).astype(np.int32)
    # unique indices in an order unrelated to the slots; the odd values are free for a running best that lives elsewhere
    IDX = (2 * (rng.integers(1, 1 << 20, (n, 1)) * 8 + np.argsort(rng.random((n, 8)), axis=1))).astype(np.int32)
    if category == "padded":
        npad = rng.integers(1, 9, n)                      # 1 .. 8 pads at the end of the leaf (8: an empty leaf)
        pad = np.arange(8)[None, :] >= (8 - npad)[:, None]
        C = np.where(pad[:, None, :], F(np.inf), C).astype(F); IDX = np.where(pad, -1, IDX).astype(np.int32)
    dd = leaf_distances(C, P)
    m = np.minimum(dd.min(axis=1), FLT_MAX).astype(F)
    other_leaf = (leaf + 1 + rng.integers(0, 1000, n)).astype(np.int32)
    # a running best from another leaf: a distance around the leaf's own (grids: one of the grid's distances, so that ties are common)
    if grid:
        best = dd[np.arange(n), rng.integers(0, 8, n)].copy()
    else:
        with np.errstate(over="ignore"):
            best = np.minimum(m * rng.choice(np.array([0.5, 0.9, 1.1, 2.0, 100.0], F), n), FLT_MAX).astype(F)
    bi = (2 * rng.integers(0, 1 << 23, n) + 1).astype(np.int32)
    bpos = (other_leaf * 8 + rng.integers(0, 8, n)).astype(np.int32)
    if category in ("seed_inside", "grid2", "grid4", "padded", "huge"):
        # the running best lives in this leaf (all rows of seed_inside, a third of the rows of the others; never a pad)
        s = rng.integers(0, 8, n)
        inside = (IDX[np.arange(n), s] >= 0) & ((rng.random(n) < 1 / 3) | (category == "seed_inside")) & np.isfinite(dd[np.arange(n), s])
        best = np.where(inside, dd[np.arange(n), s], best).astype(F)
        bi = np.where(inside, IDX[np.arange(n), s], bi).astype(np.int32); bpos = np.where(inside, leaf * 8 + s, bpos).astype(np.int32)
    if category in ("tie_lower_elsewhere", "tie_higher_elsewhere"):
        js = IDX[np.arange(n), dd.argmin(axis=1)]
        best = m.copy(); bi = (js + (-1 if category == "tie_lower_elsewhere" else 1)).astype(np.int32)
    if category == "unseeded":
        best = np.full(n, FLT_MAX, F); bi = np.full(n, -1, np.int32); bpos = np.full(n, -1, np.int32)
    # the runner-up record: empty, or an entry of this leaf, of the running best's leaf or of a third one
    kind = rng.integers(0, 4, n)
    with np.errstate(over="ignore"):
        b2 = np.where(kind == 0, FLT_MAX, np.minimum(best * rng.choice(np.array([1.0, 1.5, 4.0], F), n), FLT_MAX)).astype(F)
        b3 = np.where(kind == 0, FLT_MAX, np.minimum(b2 * rng.choice(np.array([1.0, 2.0], F), n), FLT_MAX)).astype(F)
    l2 = np.select([kind == 0, kind == 1, kind == 2], [-1, leaf, bpos >> 3], other_leaf + 7).astype(np.int32)
    return dict(C=C, IDX=IDX, P=P, leaf=leaf, best=best, bi=bi, bpos=bpos, b2=b2, l2=l2, b3=b3)


def node_cases(n, empty_lo, empty_hi, seed=0):
    """n 4-wide nodes with a query each: the query inside the box, on a face, outside; degenerate boxes (lo == hi); empty children encoded
    as (empty_lo, empty_hi) on every axis; coordinates whose squares overflow.  -> LO, HI [n, 3, 4], P [n, 3]."""
    rng = np.random.default_rng([seed, 99])
    a = rng.uniform(-1, 1, (n, 3, 4)).astype(F); b = rng.uniform(-1, 1, (n, 3, 4)).astype(F)
    LO, HI = np.minimum(a, b), np.maximum(a, b)
    P = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    kind = rng.integers(0, 6, n)
    inside = kind == 1                                     # inside child 0's box
    t = rng.random((n, 3)).astype(F)
    P = np.where(inside[:, None], (LO[:, :, 0] + (HI[:, :, 0] - LO[:, :, 0]) * t).astype(F), P)
    P = np.clip(P, np.where(inside[:, None], LO[:, :, 0], -np.inf), np.where(inside[:, None], HI[:, :, 0], np.inf)).astype(F)
    face = kind == 2                                       # on a face of child 1's box: one coordinate exactly lo or hi
    ax = rng.integers(0, 3, n); side = rng.integers(0, 2, n)
    onface = np.where(side == 0, LO[np.arange(n), ax, 1], HI[np.arange(n), ax, 1])
    P[np.arange(n)[face], ax[face]] = onface[face]
    degen = kind == 3                                      # points as boxes
    HI = np.where(degen[:, None, None], LO, HI)
    onpoint = degen & (rng.random(n) < 0.5)
    P = np.where(onpoint[:, None], LO[:, :, 2], P)
    huge = kind == 4
    P = np.where(huge[:, None], P * F(1e19), P).astype(F)
    empty = (kind == 5)[:, None] & (rng.random((n, 4)) < 0.5)     # some children empty
    LO = np.where(empty[:, None, :], F(empty_lo), LO).astype(F); HI = np.where(empty[:, None, :], F(empty_hi), HI).astype(F)
    return LO, HI, P.astype(F)
