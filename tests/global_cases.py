"""Input clouds of the global-registration edge tests (tests/test_gpu_global.py on the device, tests/test_global_host.py on the host, which
proves with the restatement alone what the device tests rely on).  Test infrastructure only; needs no GPU.

  unit_normals(n, seed)      n random unit vectors
  lattices()                 the 40 x 40 integer plane and the shuffled 14^3 integer block: exact fp32 distance ties in every neighbour list
  uniform_cloud(n, seed)     n uniform random points with random unit normals (the sizes around K, the block and a tree level)
  SIZES(k)                   those sizes
  deep_scan()                one 40 800-point laser scan with its analytic normals: a deeper tree than the bunny's
  coincident_cloud()         25 copies of one point among 200 others: more coincident points than any K
  line_cloud()               60 points on the x axis: every triple is collinear, RANSAC has REPEATED and DEGENERATE hypotheses only
  ribbon_cloud()             60 points a hair off the x axis: triples on both sides of the collinearity threshold, none near it
  EDGE_CASES, sub_clouds()   n points of the bunny source against the whole target: M = n correspondences without the mutual test
  collinearity(p)            (cc, 1e-6 aa bb) of triples in ransac_collinear's names and order, fp64
"""
import functools

import numpy as np

f32 = np.float32


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(f32)


@functools.lru_cache(maxsize=None)
def lattices():
    """dict name -> (points, normals): tests/test_gpu_normals.py::test_exact_ties_on_lattices' plane and shuffled block."""
    g = np.arange(40, dtype=f32)
    plane = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((40, 40), 3, f32)], -1).reshape(-1, 3)
    h = np.arange(14, dtype=f32)
    block = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    block = block[np.random.default_rng(5).permutation(len(block))]
    return {"plane": (plane, unit_normals(len(plane), 11)), "block": (block, unit_normals(len(block), 11))}


def SIZES(k):
    return sorted({1, 2, k - 1, k, k + 1, 255, 256, 257, 4097})


def uniform_cloud(n, seed):
    p = np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(f32)
    return p, unit_normals(n, seed + 1)


@functools.lru_cache(maxsize=None)
def deep_scan():
    from icp_amd import synth
    p, nrm, _ = synth.laser_scan(synth.scan_pose(0), 3, n_tilt=120, n_beam=340)
    return np.ascontiguousarray(p, f32), np.ascontiguousarray(nrm, f32)


DEEP_ROWS = 2000


def deep_rows(n):
    return np.sort(np.random.default_rng(17).choice(n, DEEP_ROWS, replace=False))


COPIES, COPY_AT = 25, 37


def coincident_cloud():
    """(points, normals, indices of the copies): 200 scattered points and 25 copies of point COPY_AT spread among them."""
    p, nrm = uniform_cloud(225, 23)
    where = np.sort(np.random.default_rng(29).choice(np.setdiff1d(np.arange(225), [COPY_AT]), COPIES - 1, replace=False))
    p[where] = p[COPY_AT]
    return p, nrm, np.sort(np.append(where, COPY_AT))


def _strip(offset, seed):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 1.0, 60))
    off = offset * rng.uniform(-1.0, 1.0, (60, 2))
    p = np.stack([x, off[:, 0], off[:, 1]], axis=1).astype(f32)
    tilt = rng.uniform(-0.5, 0.5, 60); a = rng.uniform(0.0, 2 * np.pi, 60)
    nrm = np.stack([tilt, np.cos(a), np.sin(a)], axis=1)
    return p, (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(f32)


LINE_H, LINE_SEED = 512, 0


def line_cloud():
    """60 points at sorted uniform x in [0, 1], y = z = 0, normals (tilt, cos a, sin a) normalised; source and target alike."""
    return _strip(0.0, 3)


RIBBON_WIDTH, RIBBON_CLOUD_SEED, RIBBON_H, RIBBON_SEED = 1e-4, 4, 512, 0
RIBBON_BAND = 1e-9          # every hypothesis: |cc - thr| > RIBBON_BAND thr, thr = 1e-6 aa bb (a few fp64 roundings are 1e-15)


def ribbon_cloud():
    """The line cloud with y and z offsets uniform in +-RIBBON_WIDTH: three points 0.1 apart with such offsets make an angle of the
    order of 1e-3 rad, the collinearity threshold, so the draws fall on both sides of it."""
    return _strip(RIBBON_WIDTH, RIBBON_CLOUD_SEED)


def collinearity(p):
    """p (H, 3, 3) fp64 triples -> (cc, thr): |e1 x e2|^2 and 1e-6 |e1|^2 |e2|^2 as ransac_collinear computes them."""
    a = p[:, 1] - p[:, 0]; b = p[:, 2] - p[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)

    def dot(u, v):
        return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    return dot(c, c), 1e-6 * (dot(a, a) * dot(b, b))


SUB_SIZES = (3, 4, 64, 255, 256, 257, 513)      # M of the RANSAC edge cases: the smallest that registers, the 256-thread score stride
SUB_K = 10
H_EDGES = (1, 63, 64, 65, 65536)                # at M = 64: around the 64-thread fit block, the smallest and the largest allowed
# (n, start, H): source points start .. start + n - 1.  The correspondences of the first 3 or 4 source points share a target point, so every
# triple of theirs is DEGENERATE or REPEATED; the sub-clouds from point 2 (M = 3) and point 1 (M = 4) have a triangle that is fitted.
EDGE_CASES = [(n, 0, 512) for n in SUB_SIZES if n != 64] + [(64, 0, H) for H in H_EDGES] + [(3, 2, 512), (4, 1, 512)]
EDGE_SIMILARITIES = (0.9, 0.0)                  # 0.9: hardly a triple of such pairs passes the edge test; 0: every triangle is fitted

N_BEST_H, N_BEST_K = 200, 10                    # on the bunny: between 65 and 255 valid hypotheses (tests/test_global_host.py)


def sub_clouds(bunny, n, start=0):
    return bunny["src_pts"][start:start + n], bunny["src_nrm"][start:start + n], bunny["tgt_pts"], bunny["tgt_nrm"]


def edge_seed(n, start, H):
    return n + H + 1000 * start
