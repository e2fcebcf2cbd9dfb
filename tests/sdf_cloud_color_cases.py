"""Inputs of the tests of a coloured laser scan aligned to the coloured TSDF volume with the photometric term: numpy
only, no device.  Built on tests/sdf_cloud_cases.py (K: the model, the special points, the plane volumes, SIZES, FOLD_BLOCKS) with colours on
top; tests/test_sdf_cloud_color_host.py shows on the restatement that they reach what they are named for, tests/test_gpu_sdf_cloud_color.py
runs them on the device.

  colored_model()   K.model() with sdf_color_restatement.smooth_colors, dense, and the same voxels and colours cut into blocks
  wall_colors()     the bytes of that smooth field at a cloud's points (the cloud in the world frame: its true pose is the identity), so
                    that the photometric row pulls where the geometric one does; the fourth byte is random, it is not read
  special()         K.special()'s points with colours, and what the colour row can get wrong: a valid point whose cell has exactly one
                    corner with Wc == 0, one whose cell holds an inf, a black and a white point, two twins that differ in the fourth byte
                    alone; special_model() is the volume crafted for them
  plane_*           K.plane_hashed() and K.plane_dense() with a colour per voxel, and the dense box that covers the eight blocks"""
import copy
import functools
import os
import re
import numpy as np

import htsdf_color_restatement as HC
import htsdf_restatement as HR
import sdf_cloud_cases as K
import sdf_cloud_color_restatement as R
import sdf_cloud_restatement as SC
import sdf_color_restatement as PC
import tsdf_cloud_color_cases as CK

f32, f64 = np.float32, np.float64
START, EYE, FOLD_BLOCKS = K.START, K.EYE, K.FOLD_BLOCKS
WEIGHT = 0.1


def points_per_block():
    """256 x SCC_POINTS_PER_LANE, read from the device source: the coloured kernels have a constant of their own, and the sizes follow it."""
    src = open(os.path.join(K.ROOT, "icp-variants_amd", "csrc", "dev_sdf_cloud_color.hpp")).read()
    return 256 * int(re.search(r"constexpr int SCC_POINTS_PER_LANE = (\d+);", src).group(1))


PER_BLOCK = points_per_block()
SIZES = sorted({1, 63, 64, 65, 255, 256, 257, 3000, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1, 2 * PER_BLOCK - 1, 2 * PER_BLOCK, 2 * PER_BLOCK + 1})
assert FOLD_BLOCKS[-1] * PER_BLOCK <= FOLD_BLOCKS[-1] * K.PER_BLOCK      # (K.fold_cloud() is long enough for the largest fold)


def smooth_bytes(w):
    """sdf_color_restatement.smooth_colors' three sinusoids at world points (n, 3): (n, 3) fp64 byte values, unrounded."""
    x, y, z = w[:, 0].astype(f64), w[:, 1].astype(f64), w[:, 2].astype(f64)
    r = 128 + 60 * np.sin(2 * np.pi * (x + 0.3 * y) / 1.7) + 0 * z
    g = 120 + 50 * np.cos(2 * np.pi * (y - 0.2 * x + 0.1 * z) / 1.5)
    b = 110 + 40 * np.sin(2 * np.pi * (0.6 * x + 0.5 * y + 0.3 * z) / 2.1 + 1.0)
    return np.stack([r, g, b], 1)


def wall_colors(pts, seed=0):
    """rgba (n, 4) uint8 of points given in the world frame; a non-finite point gets zero bytes; the fourth byte is random."""
    p = np.nan_to_num(np.asarray(pts, f64), nan=0.0, posinf=0.0, neginf=0.0)
    rgb = np.clip(np.rint(smooth_bytes(p)), 0, 255).astype(np.uint8)
    a = np.random.default_rng(1000 + seed).integers(0, 256, (len(p), 1), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a], 1))


def with_blocks_colored(dense):
    """K.as_hashed of a coloured dense volume, the blocks' colours cut from its colour array."""
    hv = HC.add_color(K.as_hashed(dense))
    for (bx, by, bz) in hv.blocks:
        sl = (slice(8 * bz, 8 * bz + 8), slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
        hv.colors[(bx, by, bz)] = [dense.rgb[sl].copy(), dense.wc[sl].copy()]
    return hv


@functools.lru_cache(maxsize=None)
def colored_model(hashed=False, free_cell=False):
    """K.model() with every voxel coloured by the smooth field (a hashed volume: every voxel of its blocks).  Shared: do not modify."""
    if hashed:
        return with_blocks_colored(colored_model(False, free_cell))
    return PC.smooth_colors(copy.deepcopy(K.model(False, free_cell)))


def cell_of(vol, q):
    """The voxel index (x, y, z) of the lowest corner of the cell of world point q (fp32, the contract's floor)."""
    return tuple(int(np.floor((f32(q[a]) - vol.o[a]) / vol.s)) for a in range(3))


@functools.lru_cache(maxsize=None)
def special():
    """(points (n, 3) fp32 in the scan frame, rgba (n, 4), index of each special point by name, crafted: the voxels special_model() changes).
    Posed at START.  The colour specials are copies of valid wall points of K.special()'s cloud, so each has a twin with a plain colour."""
    pts, names = K.special()
    names = dict(names)
    vol = colored_model(False, True)
    world = pts.astype(f64) @ START[:3, :3].astype(f64).T + START[:3, 3].astype(f64)
    rgba = wall_colors(world, seed=7)
    t = SC.point_terms(vol, pts, START)
    valid = np.nonzero(t["valid"])[0]
    cells = [cell_of(vol, t["q"][i]) for i in valid]
    # five valid points whose cells share no corner: three voxels apart on some axis
    chosen = []
    for i, c in zip(valid, cells):
        if all(max(abs(c[a] - d[a]) for a in range(3)) >= 3 for _, d in chosen):
            chosen.append((int(i), c))
        if len(chosen) == 5:
            break
    assert len(chosen) == 5, len(chosen)
    pts = [p for p in pts]; rgba = [c for c in rgba]

    def add(name, src, color):
        names[name] = len(pts); pts.append(pts[src].copy()); rgba.append(np.array(color, np.uint8))
    plain = [int(v) for v in rgba[chosen[2][0]][:3]]
    add("wc_zero", chosen[0][0], rgba[chosen[0][0]]); add("s_inf", chosen[1][0], rgba[chosen[1][0]])
    add("alpha_00", chosen[2][0], plain + [0x00]); add("alpha_ff", chosen[2][0], plain + [0xFF])
    add("black", chosen[3][0], [0, 0, 0, 77]); add("white", chosen[4][0], [255, 255, 255, 3])
    crafted = dict(wc_zero=tuple(chosen[0][1]), s_inf=tuple(d + 1 for d in chosen[1][1]))
    # the points that are considered and not valid keep the colours given above: a colour on a point without a valid cell counts for nothing
    return np.array(pts).astype(f32), np.ascontiguousarray(np.array(rgba, np.uint8)), names, crafted


@functools.lru_cache(maxsize=None)
def special_model(hashed=False):
    """colored_model(free_cell=True) with one corner's Wc set to 0 and one corner's red set to inf.  Shared: do not modify."""
    if hashed:
        return with_blocks_colored(special_model(False))
    vol = copy.deepcopy(colored_model(False, True))
    crafted = special()[3]
    i, j, k = crafted["wc_zero"]; vol.wc[k, j, i] = 0.0
    i, j, k = crafted["s_inf"]; vol.rgb[k, j, i, 0] = np.inf
    return vol


# ---- the plane volumes with a colour per voxel: a smooth function of the GLOBAL voxel index, so the hashed blocks and the covering box agree
def plane_rgb(i, j, k):
    s = 0.1
    return np.stack([128 + 60 * np.sin(2 * np.pi * (i + 0.3 * j) * s / 1.7), 120 + 50 * np.cos(2 * np.pi * (j - 0.2 * i + 0.1 * k) * s / 1.5),
                     110 + 40 * np.sin(2 * np.pi * (0.6 * i + 0.5 * j + 0.3 * k) * s / 2.1 + 1.0)], -1).astype(f32)


@functools.lru_cache(maxsize=None)
def plane_dense():
    vol = copy.deepcopy(K.plane_dense())
    nx, ny, nz = K.PLANE_DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol.rgb = plane_rgb(i, j, k); vol.wc = np.ones((nz, ny, nx), f32)
    return vol


@functools.lru_cache(maxsize=None)
def plane_hashed():
    hv = HC.add_color(copy.deepcopy(K.plane_hashed()))
    loc = np.arange(8)
    for (bx, by, bz) in hv.blocks:
        k, j, i = np.meshgrid(8 * bz + loc, 8 * by + loc, 8 * bx + loc, indexing="ij")
        hv.colors[(bx, by, bz)] = [plane_rgb(i, j, k), np.ones((8, 8, 8), f32)]
    return hv


@functools.lru_cache(maxsize=None)
def plane_cover():
    """The dense box of 16^3 voxels that covers plane_hashed()'s eight blocks, voxel for voxel: its origin is global voxel (-8, -8, -8)."""
    hv = plane_hashed()
    o = tuple(float(hv.o[a] + f32(-8) * hv.s) for a in range(3))
    vol = SC.Volume((16, 16, 16), **dict(K.PLANE_OPTS, origin=o))
    coords, t, w = hv.sorted_blocks()
    rgb, wc = HC.sorted_colors(hv)
    lo = np.array([-8, -8, -8])
    vol.tsdf[:], vol.weight[:] = HR.blocks_to_dense(coords, t, w, lo, (16, 16, 16))
    vol.wc = HR.blocks_to_dense(coords, wc, wc, lo, (16, 16, 16))[0]
    vol.rgb = np.stack([HR.blocks_to_dense(coords, rgb[..., ch], wc, lo, (16, 16, 16))[0] for ch in range(3)], -1)
    return vol


@functools.lru_cache(maxsize=None)
def fold_colors():
    return wall_colors(K.fold_cloud(), seed=17)


@functools.lru_cache(maxsize=None)
def fold_reference(blocks):
    n = blocks * PER_BLOCK
    return R.system(colored_model(), K.fold_cloud()[:n], fold_colors()[:n], START, weight=WEIGHT)


def track_scans():
    """tsdf_cloud_color_cases.track_scans: four scans of one wall whose colour is a function of the world point, and their true poses."""
    return CK.track_scans()
