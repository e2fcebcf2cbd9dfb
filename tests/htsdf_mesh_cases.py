"""The shapes the hashed-mesh tests share (tests/test_htsdf_mesh_host.py, tests/test_gpu_htsdf_mesh.py), the smallest at which the kernels
can go wrong: 1/8 m voxels and a dyadic origin (o + (float)g s is exact, so the dense volume over the blocks' bounding box holds the same
positions bit for bit), analytic spheres F = clip((|p - c| - r) / truncation, -1, 1) with weight 1.  Every case is (coords (B, 3) int32 in
key order, tsdf (B, 8, 8, 8), weight (B, 8, 8, 8)); the arrays are computed once and are read-only.  No device code."""
import functools
import numpy as np

import htsdf_cases as HC
import htsdf_mesh_restatement as HM
import htsdf_restatement as HR

f32 = np.float32
OPTS = dict(origin=(0.5, -0.25, 1.0), voxel_size=0.125, truncation=0.5, max_weight=64.0, min_depth=0.3, max_depth=8.0)
TRUNC_VOXELS = 4.0                                               # truncation / voxel_size
EDGE_BLOCK = ((1 << 20) - 1, 0, -(1 << 20))                      # case F: a corner of the storable range


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def sphere_blocks(coords, centre, radius):
    """The analytic sphere (centre and radius in voxel coordinates) sampled on the blocks `coords`, sorted into key order."""
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    coords = coords[HM.sort_blocks(coords)]
    l = np.arange(8, dtype=np.float64)
    t = np.empty((len(coords), 8, 8, 8), f32)
    for e, b in enumerate(coords.astype(np.int64)):
        z, y, x = np.meshgrid(b[2] * 8 + l, b[1] * 8 + l, b[0] * 8 + l, indexing="ij")
        dist = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
        t[e] = np.clip((dist - radius) / TRUNC_VOXELS, -1.0, 1.0).astype(f32)
    return coords, t, np.ones_like(t)


@functools.lru_cache(maxsize=None)
def case_a():
    """One block, the sphere closed inside its cells 0 .. 6: no neighbour at all."""
    return _frozen(*sphere_blocks([(0, 0, 0)], (3.3, 3.6, 3.4), 2.2))


B_CENTRE, B_RADIUS = (0.3, -0.4, 0.2), 5.3


@functools.lru_cache(maxsize=None)
def case_b():
    """2 x 2 x 2 blocks around the origin of the voxel grid: the surface crosses the three block planes, their edges and the shared corner."""
    return _frozen(*sphere_blocks(HC.box_coords((-1, -1, -1), (2, 2, 2)), B_CENTRE, B_RADIUS))


@functools.lru_cache(maxsize=None)
def case_c(missing):
    """B without the block `missing` ((0, 0, 0) or (-1, -1, -1)): an open mesh, the cells that touch the missing block invalid."""
    coords = [tuple(b) for b in HC.box_coords((-1, -1, -1), (2, 2, 2)) if tuple(b) != tuple(missing)]
    return _frozen(*sphere_blocks(coords, B_CENTRE, B_RADIUS))


@functools.lru_cache(maxsize=None)
def case_d():
    """3 x 3 x 3 blocks, a sphere, and crafted values: 2 % of the weights 0, the others drawn from {1, 2}, five NaN and three inf values of
    F, twenty voxels exactly 0.  Run at min_weight 0 and 1.5."""
    coords, t, w = sphere_blocks(HC.box_coords((-1, -1, -1), (3, 3, 3)), (4.3, 3.6, 4.4), 9.3)
    rng = np.random.default_rng(0xD)
    w = rng.choice(np.array([1, 2], f32), w.shape).astype(f32)
    w[rng.random(w.shape) < 0.02] = 0
    near = np.argwhere(np.abs(t) < 0.5)                          # crafted values where they meet the surface
    pick = near[rng.choice(len(near), 28, replace=False)]
    vals = [np.nan] * 5 + [np.inf, -np.inf, np.inf] + [0.0] * 20
    for (e, z, y, x), v in zip(pick, vals):
        t[e, z, y, x] = v
    return _frozen(coords, t, w)


@functools.lru_cache(maxsize=None)
def case_e():
    """11 x 10 x 10 = 1100 blocks (4.5 MB): more than 1024 entries per count table, so the scan of the tables carries."""
    return _frozen(*sphere_blocks(HC.box_coords((-5, -5, -5), (11, 10, 10)), (3.3, -0.4, 0.2), 30.0))


@functools.lru_cache(maxsize=None)
def case_f():
    """The single block at a corner of the storable range; the neighbours beyond it do not exist.  |g| < 2^24: (float)g is exact."""
    b = np.array(EDGE_BLOCK, np.int64)
    return _frozen(*sphere_blocks([EDGE_BLOCK], tuple(b * 8 + np.array([3.3, 3.6, 3.4])), 2.2))


@functools.lru_cache(maxsize=None)
def case_h_host(which="NEG"):
    """htsdf_cases.frames() at POSES fused into NEG (or STRADDLE) by the restatement of the hashed volume: (options, coords, tsdf, weight)."""
    opts = getattr(HC, which)
    vol = HR.HVolume(**opts)
    _, cam = HC.camera()
    for d, P in zip(HC.frames(), HC.POSES):
        HR.integrate(vol, d, cam, P)
    return (opts,) + _frozen(*vol.sorted_blocks())


def dense_of(coords, tsdf, weight, opts=OPTS):
    """The dense volume over the bounding box of the blocks: (options for Context.tsdf_create / tsdf_restatement.Volume, tsdf, weight)."""
    from icp_amd import binding
    lo_b = coords.min(0); n_b = coords.max(0) + 1 - lo_b
    d_opts = HC.dense_options(opts, tuple(int(v) for v in lo_b), tuple(int(v) for v in n_b))
    T, W = binding.tsdf_blocks_to_dense(coords, tsdf, weight, lo_b.astype(np.int64) * 8, d_opts["dims"])
    return d_opts, T, W
