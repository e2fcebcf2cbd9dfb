"""Crafted clouds for the two neighbourhood kernels behind GICP and colored ICP (k_gicp_normals<K>, k_color_gradients<K>): exact distance
ties, sizes around K / the block / the tree levels, repeats, degenerate shapes, non-finite holes, bad normals, scale extremes and
neighbourhoods placed at the determinant threshold.  numpy only, no device; fixed seeds.  Test infrastructure only.

  CASES                    name -> (points (n, 3) fp32, normals (n, 3) fp32, rgba (n, 4) uint8), at most 4 100 points each
  FAMILY                   name -> the family the case belongs to (the rows of DESIGN.md's table of worst errors)
  KS                       the K instantiations
  reference(name, k)       the restatements on a case, computed once and shared: neighbours, GICP normals, eigenvalues, covariances,
                           gradients, det / threshold, and the gradients solved without the threshold
  brute_neighbours(...)    the plain O(n^2) neighbour lists the shortcut of gicp_restatement.neighbours is checked against
  linear_gradient(nrm)     the closed-form gradient of the linear-intensity case
  ladder_window(k)         the det / threshold interval in which the threshold case's crafted points must lie
"""
import functools
import os
import re
import numpy as np

import colored_restatement as CR
import gicp_restatement as G

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (5, 10, 20)
TILTED = (0.25, -0.5, 2.0)
LINEAR = (3, 5, 10)                    # R + G + B = 3 x + 5 y + 10 on the plane lattice
BAND = (1e-2, 1e4)                     # det / threshold: inside, the fp64 adjugate and numpy's determinant may disagree visibly
BAND_CAP = 0.02


def block_threads():
    """BVH_THREADS, read from the device source: the sizes below follow the kernels' block."""
    src = open(os.path.join(ROOT, "icp-variants_amd", "csrc", "dev_bvh.hpp")).read()
    return int(re.search(r"#define ICP_BVH_THREADS (\d+)", src).group(1))


BLOCK = block_threads()
SIZES = sorted({3, 4, 255, 256, 257, 4097, BLOCK - 1, BLOCK, BLOCK + 1} | {k + d for k in KS for d in (-1, 0, 1)})


def _unit_normals(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _colours(rng, n):
    c = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    c[:, 3] = 255
    return c


def _split_sum(s):
    """uint8 colours with R + G + B = s (0 <= s <= 765)."""
    s = np.asarray(s, np.int64)
    r = np.minimum(s, 255); g = np.minimum(s - r, 255); b = s - r - g
    return np.stack([r, g, b, np.full_like(s, 255)], 1).astype(np.uint8)


def linear_gradient(nrm):
    """The gradient of I = (3 x + 5 y + 10) / 765 on a plane z = const seen from a tangent plane of normal n: the d with n . d = 0 and
    v . d = v . g for every in-plane v, d = g - (g . n / n_z) z."""
    g = np.array([LINEAR[0], LINEAR[1], 0.0]) / 765.0
    n = np.asarray(nrm, np.float64)
    out = np.tile(g, (len(n), 1))
    out[:, 2] = -(n @ g) / n[:, 2]
    return out


def ladder_window(k):
    """With c = m - 1 the weight of the constraint row, det / threshold is proportional to c^-4 while c^2 dominates the trace.  A kernel
    that used m for c lowers it by (m / (m - 1))^4: a point above 2 (where the zero pattern is asserted) and below that factor (where the
    wrong kernel falls to the threshold or below) tells the two apart.  (lo, hi) with a tenth of the interval kept clear at either end."""
    f = (k / (k - 1.0)) ** 4
    return (2.0 + 0.1 * (f - 2.0), f - 0.1 * (f - 2.0)) if f > 2.0 else None


def _ladder(rng, n_clusters=12, k=5):
    """n_clusters isolated groups of exactly k points, each scaled until the det / threshold of its first point sits in ladder_window(k)."""
    lo, hi = ladder_window(k)
    want = 0.5 * (lo + hi)
    pts, nrm, col = [], [], []
    for c in range(n_clusters):
        centre = np.array([50.0 + 10.0 * c, -40.0, 25.0])
        off = rng.normal(0, 1, (k, 3)); off[0] = 0
        n = _unit_normals(rng, k); rgba = _colours(rng, k)
        s = 2e-3
        for _ in range(60):
            p = (centre + s * off).astype(f32)
            m = CR.gradients(p, n, rgba, k)[1][0]
            if lo < m < hi:
                break
            s *= (want / m) ** 0.25
        pts.append(p); nrm.append(n); col.append(rgba)
    return np.concatenate(pts), np.concatenate(nrm), np.concatenate(col)


def _build():
    cases, family = {}, {}

    def add(fam, name, pts, nrm, rgba):
        pts = np.ascontiguousarray(pts, f32); nrm = np.ascontiguousarray(nrm, f32); rgba = np.ascontiguousarray(rgba, np.uint8)
        assert pts.shape == nrm.shape == (len(pts), 3) and rgba.shape == (len(pts), 4) and 0 < len(pts) <= 4100, name
        cases[name] = (pts, nrm, rgba); family[name] = fam

    # lattices: exact fp32 ties in nearly every neighbourhood
    rng = np.random.default_rng(1201)
    g = np.arange(40, dtype=f32)
    plane = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((40, 40), 3, f32)], -1).reshape(-1, 3)
    h = np.arange(14, dtype=f32)
    block = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    pc = _colours(rng, len(plane))
    add("lattice", "plane", plane, np.tile(f32([0, 0, 1]), (len(plane), 1)), pc)
    add("lattice", "plane tilted", plane, np.tile(f32(TILTED), (len(plane), 1)), pc)
    bn, bc = _unit_normals(rng, len(block)), _colours(rng, len(block))
    add("lattice", "block", block, bn, bc)
    perm = rng.permutation(len(block))
    add("lattice", "block shuffled", block[perm], bn[perm], bc[perm])

    # sizes around K, the block and the tree levels
    for n in SIZES:
        rng = np.random.default_rng(2400 + n)
        add("sizes", "uniform %d" % n, rng.uniform(-1, 1, (n, 3)), _unit_normals(rng, n), _colours(rng, n))

    # repeats and degenerate shapes
    rng = np.random.default_rng(3105)
    base = rng.normal(0, 1, (700, 3)).astype(f32)
    add("repeats", "pairs", base[rng.permutation(np.repeat(np.arange(700), 2))], _unit_normals(rng, 1400), _colours(rng, 1400))
    add("repeats", "one point", np.tile(f32([[0.5, -1.25, 2.0]]), (600, 1)), _unit_normals(rng, 600), _colours(rng, 600))
    t = rng.uniform(0, 10, (500, 1)).astype(f32)
    add("repeats", "line", t * f32([[0.6, 0.0, 0.8]]) + f32([[1, 2, 3]]), _unit_normals(rng, 500), _colours(rng, 500))
    holes = rng.normal(0, 1, (3000, 3)).astype(f32)
    holes[rng.choice(3000, 300, replace=False)] = np.nan
    holes[rng.choice(3000, 100, replace=False), rng.integers(0, 3, 100)] = np.inf
    holes[rng.choice(3000, 50, replace=False), 2] = -np.inf
    add("holes", "holes", holes, _unit_normals(rng, 3000), _colours(rng, 3000))
    two = np.full((300, 3), np.nan, f32); two[10] = [1, 2, 3]; two[200] = [1, 2, 3.5]
    add("holes", "two finite", two, _unit_normals(rng, 300), _colours(rng, 300))
    three = np.full((300, 3), np.nan, f32); three[[7, 150, 299]] = [[1, 2, 3], [1, 2, 3.5], [1.5, 2, 3]]
    add("holes", "three finite", three, _unit_normals(rng, 300), _colours(rng, 300))
    for n in (1, 2, 3, 1000):
        add("holes", "all NaN %d" % n, np.full((n, 3), np.nan, f32), _unit_normals(rng, n), _colours(rng, n))

    # the normals and colours the gradient kernel reads by original index
    rng = np.random.default_rng(4207)
    n = 1000
    nrm = _unit_normals(rng, n)
    rows = rng.permutation(n)[:25].reshape(5, 5)
    nrm[rows[0]] = 0.0
    nrm[rows[1]] = np.nan; nrm[rows[1][:2], 1:] = 0.5                   # NaN in one component or in all three
    nrm[rows[2], rng.integers(0, 3, 5)] = [np.inf, -np.inf, np.inf, -np.inf, np.inf]
    nrm[rows[3]] *= f32(1e-3)
    nrm[rows[4]] *= f32(1e3)
    add("normals and colours", "bad normals", rng.normal(0, 1, (n, 3)), nrm, _colours(rng, n))
    add("normals and colours", "one colour", rng.uniform(-1, 1, (500, 3)), _unit_normals(rng, 500), np.tile(np.uint8([[90, 17, 200, 255]]), (500, 1)))
    lin_n = np.where((np.arange(len(plane)) % 2 == 0)[:, None], f32([[0, 0, 1]]), f32([TILTED]))
    add("normals and colours", "linear intensity", plane, lin_n, _split_sum(LINEAR[0] * plane[:, 0] + LINEAR[1] * plane[:, 1] + LINEAR[2]))

    # scale
    rng = np.random.default_rng(5309)
    tight = (rng.integers(0, 6, (40, 3)) * f32(1e-3))[:, None, :] + rng.normal(0, 1e-4, (40, 25, 3))
    wide = (rng.integers(-3, 4, (40, 3)) * f32(1e2))[:, None, :] + rng.normal(0, 1.0, (40, 25, 3))
    mixed = np.concatenate([tight.reshape(-1, 3), wide.reshape(-1, 3)]).astype(f32)
    perm = rng.permutation(2000)
    tight_mask = perm < 1000
    add("scale", "mixed scales", mixed[perm], _unit_normals(rng, 2000), _colours(rng, 2000))
    add("scale", "offset 1e4", (rng.normal(0, 1, (2000, 3)) + 1e4), _unit_normals(rng, 2000), _colours(rng, 2000))

    # the determinant threshold: a few isolated groups of exactly 5 points placed just above it, inside a well-conditioned cloud
    rng = np.random.default_rng(6411)
    lp, ln, lc = _ladder(rng)
    body = rng.uniform(-1, 1, (3940, 3))
    pts = np.concatenate([body, lp]); nrm = np.concatenate([_unit_normals(rng, 3940), ln]); col = np.concatenate([_colours(rng, 3940), lc])
    is_ladder = np.arange(len(pts)) >= 3940
    perm = rng.permutation(len(pts))
    add("threshold", "threshold ladder", pts[perm], nrm[perm], col[perm])
    return cases, family, dict(tight=tight_mask, ladder=is_ladder[perm])


CASES, FAMILY, MARKS = _build()          # MARKS: the tight-cluster points of "mixed scales", the crafted groups of "threshold ladder"
NAMES = list(CASES)


def brute_neighbours(pts, kmax, highest_index_wins=False):
    """Plain O(n^2): for every finite point the min(kmax, finite) smallest (fp32 (dx dx + dy dy) + dz dz, index) pairs over the finite
    points, by lexsort -- (indices, distances), -1 / NaN rows for non-finite points.  highest_index_wins: ties broken the wrong way."""
    pts = np.ascontiguousarray(pts, f32)
    n = len(pts)
    fin = np.nonzero(np.isfinite(pts).all(1))[0]
    kk = min(kmax, len(fin))
    ids = np.full((n, kk), -1, np.int64); d2s = np.full((n, kk), np.nan, f32)
    if kk == 0:
        return ids, d2s
    F = pts[fin]
    key = -fin if highest_index_wins else fin
    for a in range(0, len(fin), 256):
        d = F[a:a + 256, None, :] - F[None, :, :]
        d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)
        o = np.lexsort((np.broadcast_to(key, d2.shape), d2), axis=1)[:, :kk]
        ids[fin[a:a + 256]] = fin[o]; d2s[fin[a:a + 256]] = np.take_along_axis(d2, o, 1)
    return ids, d2s


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """The restatements on a case, once: dict(nb, nrm, ev, cov, grad, margin, solved).  Callers leave the arrays unchanged."""
    pts, nrm, rgba = CASES[name]
    nb = G.neighbours(pts, k)
    gn, ev, cov = G.normals(pts, k, nb=nb, cov=True)
    grad, margin, solved = CR.gradients(pts, nrm, rgba, k, nb=nb, full=True)
    out = dict(nb=nb, nrm=gn, ev=ev, cov=cov, grad=grad, margin=margin, solved=solved)
    for v in out.values():
        v.setflags(write=False)
    return out


def in_band(margin):
    with np.errstate(invalid="ignore"):
        return (margin > BAND[0]) & (margin < BAND[1])
