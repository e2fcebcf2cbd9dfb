"""The shapes the coloured hashed view tests share (tests/test_htsdf_color_view_host.py, tests/test_gpu_htsdf_color_view.py):
htsdf_raycast_cases' volumes and poses (RC), each with a colour pool.  P, NEG and STRADDLE are fused from htsdf_cases' frames with crafted
colour frames through htsdf_color_restatement.integrate_color (the geometry is RC's, asserted).  The spheres A - D and F get an analytic
colour -- non-integer channel values that vary along all three axes and leave 0 .. 255 on both sides, so the clamp is exercised -- with Wc
zeroed on a sparse deterministic pattern and on one whole block of B.  G is this file's own: 2 x 2 x 2 blocks around the grid origin with
a sphere whose surface passes through the middle of the cell (-1, -1, -1), seen along the diagonal, so that hits fall into cells spanning
2, 4 and 8 blocks (B's sphere encloses the grid origin: no ray ends in its eight-block cell).  Every case is (name, options, coords, tsdf, weight, rgb,
cweight, poses); the arrays are computed once and are read-only.  No device code."""
import functools
import numpy as np

import htsdf_cases as HC
import htsdf_color_restatement as HCR
import htsdf_color_view_restatement as VR
import htsdf_mesh_cases as MC
import htsdf_raycast_cases as RC
import htsdf_restatement as HR

f32 = np.float32
SIZES = RC.SIZES
ZERO_BLOCK = (0, -1, -1)                                         # the block of B (and of C) whose Wc is all 0
G_CENTRE, G_RADIUS = (5.0, 5.0, 5.0), float(np.sqrt(3 * 5.5 ** 2))      # the surface passes through the middle of cell (-1, -1, -1)


def color_frames():
    """One colour frame (h*w, 4) u8 per frame of htsdf_cases.frames(): random bytes, a black and a white patch, the fourth byte junk."""
    rng = np.random.default_rng(0xC0107)
    out = []
    for k in range(3):
        c = rng.integers(0, 256, (HC.H, HC.W, 4), dtype=np.uint8)
        c[5:12, 8:20, :3] = 0; c[30:40, 40:60, :3] = 255
        out.append(c.reshape(-1, 4))
    return out


@functools.lru_cache(maxsize=None)
def fused(which):
    """htsdf_cases' three frames with color_frames() fused into BOX ("P"), NEG or STRADDLE by the restatement of the coloured hashed volume:
    (options, coords, tsdf, weight, rgb, cweight)."""
    opts = HC.BOX if which == "P" else getattr(HC, which)
    vol = HCR.add_color(HR.HVolume(**opts))
    _, cam = HC.camera()
    for d, c, P in zip(HC.frames(), color_frames(), HC.POSES):
        HCR.integrate_color(vol, d, c, cam, P)
    return (opts,) + MC._frozen(*vol.sorted_blocks(), *HCR.sorted_colors(vol))


def analytic_colors(coords, zero_block=None):
    """rgb (B, 8, 8, 8, 3) and cweight (B, 8, 8, 8) of the blocks `coords`: per voxel, with g its coordinate relative to the first block's
    first voxel, R = 300.7 - 13.3 gx + 2.9 gy + 1.7 gz, G = -40.2 + 3.1 gx + 11.9 gy - 2.3 gz, B = 128.4 - 5.7 gx + 4.3 gy + 9.1 gz;
    Wc = 1 + (gx + gy + gz) % 3, and 0 where (gx + 2 gy + 3 gz) % 11 == 0 and on every voxel of `zero_block`."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    lo = coords.min(0) * 8
    l = np.arange(8, dtype=np.int64)
    rgb = np.empty((len(coords), 8, 8, 8, 3), f32); wc = np.empty((len(coords), 8, 8, 8), f32)
    for e, b in enumerate(coords):
        z, y, x = np.meshgrid(b[2] * 8 + l - lo[2], b[1] * 8 + l - lo[1], b[0] * 8 + l - lo[0], indexing="ij")
        rgb[e, ..., 0] = 300.7 - 13.3 * x + 2.9 * y + 1.7 * z
        rgb[e, ..., 1] = -40.2 + 3.1 * x + 11.9 * y - 2.3 * z
        rgb[e, ..., 2] = 128.4 - 5.7 * x + 4.3 * y + 9.1 * z
        wc[e] = 1 + (x + y + z) % 3
        wc[e][(x + 2 * y + 3 * z) % 11 == 0] = 0
        if zero_block is not None and tuple(int(v) for v in b) == tuple(zero_block):
            wc[e] = 0
    return MC._frozen(rgb, wc)


@functools.lru_cache(maxsize=None)
def case_g():
    return MC._frozen(*MC.sphere_blocks(HC.box_coords((-1, -1, -1), (2, 2, 2)), G_CENTRE, G_RADIUS))


def _g_views():
    eye = (-9.0, -8.0, -10.0)
    return [RC.look_at(eye, (0.0, 0.0, 0.0)), RC.look_at((-7.0, -7.5, -6.5), (-0.5, -0.5, -0.5)), RC.look_at((-12.0, 2.0, 1.0), (-2.0, 2.5, 1.5))]


@functools.lru_cache(maxsize=None)
def all_cases():
    """[(name, options, coords, tsdf, weight, rgb, cweight, [poses])]: RC.all_cases() with colours, then G."""
    out = []
    for name, opts, c, t, w, poses in RC.all_cases():
        if name in ("P", "NEG", "STRADDLE"):
            o2, c2, t2, w2, rgb, wc = fused(name)
            assert np.array_equal(c2, c) and np.array_equal(t2.view(np.uint32), t.view(np.uint32)) and np.array_equal(w2.view(np.uint32), w.view(np.uint32))
        else:
            rgb, wc = analytic_colors(c, ZERO_BLOCK if name[0] in "BC" else None)
        out.append((name, opts, c, t, w, rgb, wc, poses))
    c, t, w = case_g()
    out.append(("G", MC.OPTS, c, t, w) + analytic_colors(c) + (_g_views(),))
    return out


def shifted(case, by=2):
    """RC.shifted for a coloured case."""
    name, opts, c, t, w, rgb, wc, poses = case
    n2, o2, c2, t2, w2, p2 = RC.shifted((name, opts, c, t, w, poses), by)
    return (n2, o2, c2, t2, w2, rgb, wc, p2)


@functools.lru_cache(maxsize=None)
def dense_equality_cases():
    """RC.dense_equality_cases() with colours, and G shifted: P as it is, A - D and G moved to non-negative coordinates."""
    cs = all_cases()
    return [cs[0]] + [shifted(c) for c in cs if c[0][0] in "ABCDG"]


def dense_lo0(case):
    """RC.dense_lo0 with the colour arrays: (options, tsdf, weight, rgb (nz, ny, nx, 3), cweight (nz, ny, nx))."""
    from icp_amd import binding
    name, opts, c, t, w, rgb, wc, _ = case
    d_opts, T, W = RC.dense_lo0(opts, c, t, w)
    RGB, WC = binding.tsdf_block_colors_to_dense(c, rgb, wc, np.zeros(3, np.int64), d_opts["dims"])
    return d_opts, T, W, RGB, WC


def dense_of(case):
    """MC.dense_of with the colour arrays, over the bounding box of the blocks."""
    from icp_amd import binding
    name, opts, c, t, w, rgb, wc, _ = case
    d_opts, T, W = MC.dense_of(c, t, w, opts)
    RGB, WC = binding.tsdf_block_colors_to_dense(c, rgb, wc, c.min(0).astype(np.int64) * 8, d_opts["dims"])
    return d_opts, T, W, RGB, WC


def blocks_of(case, **over):
    name, opts, c, t, w, rgb, wc, _ = case
    return VR.ColorBlocks(c, t, w, rgb, wc, **dict(opts, **over))


@functools.lru_cache(maxsize=None)
def restated(case_index, size_index, pose_index, which="all"):
    """The restatement's coloured ray-cast of one (case, camera size, pose), computed once and shared:
    (depth, vertices, normals, rgba, hits, coloured hits, path, trace)."""
    case = {"all": all_cases, "dense": dense_equality_cases}[which]()[case_index]
    w, h = SIZES[size_index]
    tr = {}
    out = VR.raycast_color(blocks_of(case), RC.camera(w, h)[1], case[7][pose_index], trace=tr)
    for a in out[:4] + (out[6],):
        a.setflags(write=False)
    return out + (tr,)


MESH_CASES = ("P", "NEG", "A", "B", "C without (0, 0, 0)", "D", "F", "G")      # the cases meshed with colours
MIN_WEIGHTS = (0.0, 1.5)


@functools.lru_cache(maxsize=None)
def restated_mesh(case_index, min_weight):
    """The restatement's coloured mesh of one case: (vertices, normals, triangles, colours, stats)."""
    st = {}
    out = VR.mesh(blocks_of(all_cases()[case_index]), min_weight, st)
    for a in out:
        a.setflags(write=False)
    return out + (st,)
