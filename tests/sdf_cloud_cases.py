"""Inputs of the tests of a laser scan aligned to the TSDF volume: numpy only, no device.  tests/test_sdf_cloud_host.py
shows on the restatement that they reach what they are named for; tests/test_gpu_sdf_cloud.py runs them on the device.

  model()        four wall scans (tsdf_cloud_cases.cloud) fused by tsdf_cloud_restatement into a dense box whose extents are multiples of 8,
                 and the same voxels cut into blocks: the dense and the hashed volume hold the same field
  special()      about 300 points at START against model() with a crafted all-free-space cell: a NaN, an inf, an unobserved cell, |F| == 1
                 exactly, one point outside the box on each face
  plane_*        small crafted volumes whose every voxel is observed (a tilted plane's distance): the last cell of each face of a dense box,
                 and cells that straddle blocks -1 / 0 of a hashed volume on each axis
  SIZES          1, 63 .. 257, 3000 and one point either side of one block's and of two blocks' points; FOLD_BLOCKS for k_sdf_solve's fold"""
import functools
import os
import re
import numpy as np

import sdf_cloud_restatement as SC
import tsdf_cloud_restatement as CR
from support import pose_of
from tsdf_cloud_cases import cloud

f32 = np.float32
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OPTS = dict(origin=(-3.95, -2.35, 0.65), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=6.0)
DIMS = (80, 48, 32)
EYE = np.eye(4, dtype=f32)
MODEL_POSES = [EYE, pose_of((0.02, -0.03, 0.01), (0.03, -0.02, 0.01)), pose_of((-0.03, 0.02, -0.02), (-0.02, 0.03, -0.02)), pose_of((0.01, 0.04, 0.02), (0.01, 0.01, 0.03))]
START = pose_of((0.012, -0.009, 0.007), (0.03, -0.02, 0.025))      # a few centimetres and a hundredth of a radian from the answer (EYE)
FREE_CELL = (2, 2, 2)                                # special(): the crafted cell whose eight corners all read exactly 1


def points_per_block():
    """256 x SC_POINTS_PER_LANE, read from the device source: the sizes below follow the kernel's constant."""
    src = open(os.path.join(ROOT, "icp-variants_amd", "csrc", "dev_sdf_cloud.hpp")).read()
    return 256 * int(re.search(r"constexpr int SC_POINTS_PER_LANE = (\d+);", src).group(1))


PER_BLOCK = points_per_block()
SIZES = sorted({1, 63, 64, 65, 255, 256, 257, 3000, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1, 2 * PER_BLOCK - 1, 2 * PER_BLOCK, 2 * PER_BLOCK + 1})
FOLD_BLOCKS = (1, 64, 65, 256, 257, 513)


def as_hashed(dense):
    """The dense volume's observed voxels as an HVolume with the same origin: every 8 x 8 x 8 block that holds a weight."""
    hv = SC.HVolume(origin=tuple(float(x) for x in dense.o), voxel_size=float(dense.s), truncation=float(dense.trunc), max_weight=float(dense.max_w),
                    max_depth=float(dense.max_d))
    nx, ny, nz = dense.dims
    assert nx % 8 == 0 and ny % 8 == 0 and nz % 8 == 0
    for bz in range(nz // 8):
        for by in range(ny // 8):
            for bx in range(nx // 8):
                sl = (slice(8 * bz, 8 * bz + 8), slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
                if (dense.weight[sl] > 0).any():
                    hv.blocks[(bx, by, bz)] = [dense.tsdf[sl].copy(), dense.weight[sl].copy()]
    return hv


@functools.lru_cache(maxsize=None)
def model(hashed=False, free_cell=False):
    """The shared model.  free_cell: with the eight corners of FREE_CELL set to (1, weight 1).  Shared: do not modify."""
    if hashed:
        return as_hashed(model(False, free_cell))
    vol = SC.Volume(DIMS, **OPTS)
    for k, T in enumerate(MODEL_POSES):
        info = CR.integrate(vol, cloud(3000, seed=90 + k), T)
        assert info["n_outside"] == 0, info
    # the box's outermost layer stays unobserved, so the hashed copy (whose cells may read neighbouring blocks) sees the same validity
    w = vol.weight
    assert not (w[0].any() or w[-1].any() or w[:, 0].any() or w[:, -1].any() or w[:, :, 0].any() or w[:, :, -1].any())
    if free_cell:
        i, j, k = FREE_CELL
        assert not vol.weight[k - 1:k + 3, j - 1:j + 3, i - 1:i + 3].any()
        vol.tsdf[k:k + 2, j:j + 2, i:i + 2] = 1.0; vol.weight[k:k + 2, j:j + 2, i:i + 2] = 1.0
    return vol


def voxel_point(vol, idx, frac=(0.4, 0.3, 0.6)):
    """The world point at fractions `frac` inside the cell whose lowest corner is voxel `idx`."""
    return np.array([float(vol.o[a]) + (idx[a] + frac[a]) * float(vol.s) for a in range(3)], np.float64)


def special():
    """(points (n, 3) fp32 in the scan frame, index of each special point by name).  Posed at START against model(free_cell=True)."""
    vol = model(False, True)
    inv = np.linalg.inv(START.astype(np.float64))
    to_scan = lambda w: (inv[:3, :3] @ w + inv[:3, 3])
    pts = [p for p in cloud(290, seed=7).astype(np.float64)]
    names = {}

    def add(name, p):
        names[name] = len(pts); pts.append(np.asarray(p, np.float64))
    add("nan", (np.nan, 0.0, 2.0)); add("inf", (0.1, np.inf, 2.0)); add("minus_inf", (0.1, 0.2, -np.inf))
    add("unobserved", to_scan(voxel_point(vol, (40, 24, 1))))
    add("free", to_scan(voxel_point(vol, FREE_CELL)))
    nx, ny, nz = DIMS
    for a, n in enumerate(DIMS):
        lo = [40, 24, 16]; hi = [40, 24, 16]
        lo[a] = -2; hi[a] = n + 1
        add("below_" + "xyz"[a], to_scan(voxel_point(vol, lo))); add("above_" + "xyz"[a], to_scan(voxel_point(vol, hi)))
    return np.array(pts).astype(f32), names


def plane_field(gx, gy, gz, s, trunc):
    """F of a tilted plane through the grid, in units of the truncation, kept inside (-0.9, 0.9)."""
    d = (0.5 * gx + 0.3 * gy + 0.8 * gz) * s * 0.25
    return np.clip(d / trunc, -0.9, 0.9).astype(f32)


PLANE_OPTS = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=6.0)
PLANE_DIMS = (10, 9, 8)


@functools.lru_cache(maxsize=None)
def plane_dense():
    """A dense box whose every voxel is observed.  Shared: do not modify."""
    vol = SC.Volume(PLANE_DIMS, **PLANE_OPTS)
    nx, ny, nz = PLANE_DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol.tsdf[:] = plane_field(i - 5.0, j - 4.0, k - 4.0, 0.1, 0.3); vol.weight[:] = 1.0
    return vol


@functools.lru_cache(maxsize=None)
def plane_hashed():
    """The eight blocks (-1 .. 0)^3, every voxel observed.  Shared: do not modify."""
    hv = SC.HVolume(**PLANE_OPTS)
    loc = np.arange(8)
    for bz in (-1, 0):
        for by in (-1, 0):
            for bx in (-1, 0):
                k, j, i = np.meshgrid(8 * bz + loc, 8 * by + loc, 8 * bx + loc, indexing="ij")
                hv.blocks[(bx, by, bz)] = [plane_field(i.astype(f32), j.astype(f32), k.astype(f32), 0.1, 0.3), np.ones((8, 8, 8), f32)]
    return hv


def cell_points(vol, cells, per_cell=12, seed=0):
    """per_cell random points inside each of the cells (lowest corner's voxel index), world frame, fp32."""
    r = np.random.default_rng(seed)
    out = []
    for c in cells:
        for _ in range(per_cell):
            out.append(voxel_point(vol, c, r.uniform(0.05, 0.95, 3)))
    return np.array(out).astype(f32)


def face_cells():
    """(the first and the last cell of each axis of PLANE_DIMS, the cells one step outside them)."""
    nx, ny, nz = PLANE_DIMS
    inside, outside = [], []
    for a, n in enumerate(PLANE_DIMS):
        for v, w in ((0, -1), (n - 2, n - 1)):
            c = [4, 3, 3]; c[a] = v; inside.append(tuple(c))
            c = [4, 3, 3]; c[a] = w; outside.append(tuple(c))
    return inside, outside


def straddle_cells():
    """Cells with index -1 on one axis (corners in blocks -1 and 0), on two, on all three; and index 7 .. -9 outside the eight blocks."""
    inside = [(-1, 3, -4), (2, -1, 3), (-3, 2, -1), (-1, -1, 4), (-1, -1, -1), (6, 6, 6), (-8, -8, -8)]
    outside = [(7, 0, 0), (0, -9, 0), (-1, -1, 7)]
    return inside, outside


@functools.lru_cache(maxsize=None)
def fold_cloud():
    """FOLD_BLOCKS[-1] blocks of wall points; a prefix of b * PER_BLOCK points runs b blocks.  Shared: do not modify."""
    return cloud(FOLD_BLOCKS[-1] * PER_BLOCK, seed=17)


@functools.lru_cache(maxsize=None)
def fold_reference(blocks):
    return SC.system(model(), fold_cloud()[:blocks * PER_BLOCK], START)


# ---- the three small scans of the loop tests: the wall seen from three poses a few centimetres apart, in the sensor frame
TRACK_POSES = [EYE, pose_of((0.01, -0.012, 0.006), (0.03, -0.02, 0.015)), pose_of((0.02, -0.02, 0.012), (0.06, -0.035, 0.03))]
TRACK_DIMS = dict(dims=DIMS, **OPTS)


def track_scans(n=2500):
    """Three scans of ONE wall (the same world surface, different samples of it), each in its own sensor frame."""
    out = []
    for k, T in enumerate(TRACK_POSES):
        w = cloud(n, seed=30 + k).astype(np.float64)
        inv = np.linalg.inv(T.astype(np.float64))
        out.append((w @ inv[:3, :3].T + inv[:3, 3]).astype(f32))
    return out
