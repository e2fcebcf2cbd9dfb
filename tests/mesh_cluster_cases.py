"""The inputs the vertex-clustering tests share (tests/test_mesh_cluster_host.py, tests/test_gpu_mesh_cluster.py), the smallest at which the
kernels can go wrong.  Every case is a dict(vertices, triangles, cell_size, origin, normals, colors) -- normals and colors may be None --,
computed once and read-only.  No device code."""
import functools
import numpy as np

f32 = np.float32
U32_MAX = 0xFFFFFFFF


def _case(vertices, triangles, cell_size=1.0, origin=(0.0, 0.0, 0.0), normals=None, colors=None):
    c = dict(vertices=np.ascontiguousarray(vertices, f32).reshape(-1, 3), triangles=np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3),
             cell_size=float(cell_size), origin=tuple(float(x) for x in origin),
             normals=None if normals is None else np.ascontiguousarray(normals, f32).reshape(-1, 3),
             colors=None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def args(case, normals=True, colors=True):
    """(vertices, triangles, cell_size) and the keywords of Context.mesh_cluster / the restatement's cluster."""
    return (case["vertices"], case["triangles"], case["cell_size"]), dict(origin=case["origin"], normals=case["normals"] if normals else None,
                                                                          colors=case["colors"] if colors else None)


def attributes(rng, n, nan_share=0.0, uncoloured_share=0.0):
    """Random unit normals (a share with one NaN component) and colours (a share with alpha 0)."""
    nr = rng.normal(size=(n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(f32)
    bad = rng.random(n) < nan_share
    nr[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
    col = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    col[:, 3] = np.where(rng.random(n) < uncoloured_share, 0, rng.integers(1, 256, n)).astype(np.uint8)
    return nr, col


# three cells along a corner, two vertices in each: 0, 3 in A; 1, 4 in B; 2, 5 in C
_SIX = [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.5, 0.5), (0.25, 0.75, 0.5), (1.25, 0.25, 0.75), (0.75, 1.75, 0.25)]


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> case, the small crafted ones."""
    c = {}
    c["empty"] = _case(np.zeros((0, 3)), np.zeros((0, 3)))
    c["vertices without triangles"] = _case(_SIX, np.zeros((0, 3)))
    c["triangles without vertices"] = _case(np.zeros((0, 3)), [(0, 1, 2), (U32_MAX, 0, 0)])
    c["one triangle over three cells"] = _case(_SIX[:3], [(0, 1, 2)])
    c["one triangle inside one cell"] = _case([(0.1, 0.2, 0.3), (0.9, 0.1, 0.5), (0.5, 0.9, 0.7)], [(0, 1, 2)])
    c["same triple in two rotations"] = _case(_SIX, [(1, 2, 0), (3, 4, 5), (5, 3, 4)])
    c["opposite orientations"] = _case(_SIX, [(0, 1, 2), (3, 5, 4), (2, 1, 0)])
    # vertices 0 and 1 share cell X, whose only triangle degenerates: X is absent and the ranks of the later clusters shift
    c["a cluster whose triangles all degenerate"] = _case([(7.5, 7.5, 7.5), (7.25, 7.75, 7.5)] + _SIX, [(0, 1, 2), (0, 0, 4), (2, 3, 4), (5, 6, 7)])
    on_faces = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 2, 2), (-1, 0, 3), (1, 1, 0), (3, 0, -2)]
    c["vertices exactly on cell faces"] = _case(on_faces, [(0, 1, 2), (0, 2, 3), (4, 5, 6), (1, 6, 7), (3, 4, 7)])
    c["vertices on the faces of 0.1 cells"] = _case(np.array(on_faces) * f32(0.1), [(0, 1, 2), (0, 2, 3), (4, 5, 6), (1, 6, 7), (3, 4, 7)], cell_size=0.1)
    # floor, not truncation: -0.5 lies in cell -1; -1e-10 lies in cell -1 with g - f rounding up to 1
    neg = [(-0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (-1e-10, 0.25, -1e-10), (-1.0, -2.5, -0.75), (0.75, 0.25, -3.0), (-0.25, 0.5, 0.75)]
    c["negative coordinates"] = _case(neg, [(0, 1, 2), (3, 4, 5), (1, 3, 5), (6, 1, 2), (0, 4, 2)])
    rng = np.random.default_rng(9)
    p = rng.uniform(-2, 2, (40, 3))
    c["a non-zero origin"] = _case(p, rng.integers(0, 40, (80, 3)), cell_size=0.37, origin=(0.3, -1.7, 2.05))
    lo, hi = -float(1 << 20), float(1 << 20) - 0.5
    edge = [(lo, 0.5, 0.5), (hi, 0.5, 0.5), (0.5, lo, hi), (0.5, 0.5, 0.5), (lo, lo, lo), (hi, hi, hi)]
    c["cells at -2^20 and 2^20 - 1"] = _case(edge, [(0, 1, 2), (3, 4, 5), (0, 3, 5), (1, 2, 4)])
    out = edge + [(lo - 1.0, 0.5, 0.5), (0.5, float(1 << 20), 0.5), (np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (1.5, 0.5, 0.5)]
    c["outside the range, NaN and inf"] = _case(out, [(0, 1, 2), (6, 0, 1), (0, 7, 1), (8, 3, 5), (9, 3, 5), (3, 10, 5), (3, 5, 11), (11, 3, 5)])
    c["indices beyond the vertices"] = _case(_SIX, [(0, 1, 2), (6, 1, 2), (0, U32_MAX, 2), (0, 1, U32_MAX - 1), (3, 4, 5), (1 << 31, 4, 5)])
    # attributes: opposite normals that sum to zero (cell A), a NaN normal beside a good one (cell B), a cluster without a coloured member (cell C)
    nr = [(0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, -1), (np.nan, 0, 0), (0, 0.6, 0.8)]
    col = [(10, 20, 30, 255), (200, 100, 0, 1), (1, 2, 3, 0), (11, 21, 31, 7), (0, 0, 255, 0), (9, 9, 9, 0)]
    c["normals that cancel, a NaN normal, uncoloured members"] = _case(_SIX, [(0, 1, 2), (3, 4, 5)], normals=nr, colors=col)
    return c


@functools.lru_cache(maxsize=None)
def one_cell():
    """4096 vertices in ONE cell, tied to two other cells by a few triangles: same-address adds, 64-bit sums, Q by integer division."""
    rng = np.random.default_rng(4096)
    v = np.concatenate([rng.uniform(0.0, 1.0, (4096, 3)) * 0.25 + (3 * 0.25, -2 * 0.25, 1 * 0.25), [(0.1, 0.1, 0.1), (-0.6, 0.3, 0.9)]])
    t = [(i, 4096, 4097) for i in (4095, 7, 7, 2048)] + [(4097, 5, 4096), (4096, 9, 4097), (0, 1, 2)]
    nr, col = attributes(rng, len(v), nan_share=0.01, uncoloured_share=0.3)
    return _case(v, t, cell_size=0.25, normals=nr, colors=col)


@functools.lru_cache(maxsize=None)
def distinct_cells(V=5000):
    """V vertices in V distinct cells: the cell table is half full, so there are probe chains in both tables."""
    rng = np.random.default_rng(V)
    i = np.arange(V)
    v = (np.stack([i % 50, (i // 50) % 50, i // 2500], 1) - 25 + rng.uniform(0.01, 0.99, (V, 3))) * 0.5
    t = rng.integers(0, V, (2 * V, 3))
    t[1::7] = t[0:-1:7][:len(t[1::7]), [1, 2, 0]]                      # duplicates in another rotation
    nr, col = attributes(rng, V)
    return _case(v, t, cell_size=0.5, normals=nr, colors=col)


RANDOM_SIZES = (63, 64, 65, 255, 256, 257, 1025, 1024 * 256 + 1)


@functools.lru_cache(maxsize=None)
def random_mesh(V):
    """V random vertices in about V / 8 cells (at least 27) and 2 V random triangles, a tenth of them copies of others in another rotation;
    a few invalid vertices and indices; normals (2 % with a NaN component) and colours (a fifth uncoloured)."""
    rng = np.random.default_rng(V)
    side = max(3, int(round((V / 8.0) ** (1.0 / 3.0))))
    cs = 0.5
    v = rng.uniform(-side * cs / 2, side * cs / 2, (V, 3)).astype(f32)
    v[rng.integers(0, V, max(1, V // 200))] = np.nan
    t = rng.integers(0, V, (2 * V, 3)).astype(np.int64)
    src = rng.integers(0, 2 * V, 2 * V // 10)
    t[rng.integers(0, 2 * V, len(src))] = t[src][:, [2, 0, 1]]
    t[rng.integers(0, 2 * V, max(1, V // 100)), rng.integers(0, 3, max(1, V // 100))] = V + rng.integers(0, 5, max(1, V // 100))
    nr, col = attributes(rng, V, nan_share=0.02, uncoloured_share=0.2)
    return _case(v, t, cell_size=cs, origin=(0.05, -0.1, 0.15), normals=nr, colors=col)
