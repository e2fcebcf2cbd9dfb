"""The shapes the hashed TSDF tests share (tests/test_htsdf_host.py, tests/test_gpu_htsdf.py): volumes, frames and poses, at the smallest
sizes at which the kernels can go wrong.  No device code."""
import numpy as np

import tsdf_restatement as TS
from icp_amd.synth import make_pose, tum_K, wavy_depth

f32 = np.float32
MINF = f32(-np.inf)
W, H = 64, 48

# 10 cm voxels (blocks of 0.8 m); the origin sits inside the scene, so the frames below reach blocks on both sides of 0 on every axis
STRADDLE = dict(origin=(0.25, 0.15, 1.3), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=2.4)
# 10 cm voxels again, the origin below and in front of everything the frames reach: all blocks at non-negative coordinates, inside BOX_DIMS
BOX = dict(origin=(-1.8, -1.8, -0.5), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=2.4)
BOX_DIMS = (48, 48, 48)
# 1/16 m voxels and an origin that is a multiple of it: o + (float)g s is exact, so a dense box whose origin is shifted by whole voxels
# holds the same positions bit for bit.  NEG_LO: the box's first block (negative on every axis), NEG_BLOCKS its extent in blocks.
NEG = dict(origin=(0.5, 0.25, 1.5), voxel_size=0.0625, truncation=0.25, max_weight=64.0, min_depth=0.3, max_depth=2.4)
NEG_LO, NEG_BLOCKS = (-5, -5, -3), (8, 8, 6)

TILTED = make_pose((0.12, -0.2, 0.07), (0.1, -0.05, 0.02)).astype(f32)
POSES = [np.eye(4, dtype=f32), TILTED, make_pose((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05)).astype(f32)]


def camera(w=W, h=H):
    from icp_amd import binding
    return binding.depth_camera(tum_K(w), w, h), TS.Camera(tum_K(w), w, h)


def crafted_frame(w=W, h=H):
    """wavy_depth with every kind of depth the contract names: MINF, NaN, +inf, 0, a negative depth, a depth beyond max_depth (2.4), a hole."""
    d = wavy_depth(w, h)
    d[0, :6] = [MINF, np.nan, np.inf, 0.0, -1.0, 2.5]
    d[h // 3:h // 3 + 4, w // 2:w // 2 + 4] = MINF
    return d


def frames():
    """Three 64 x 48 frames for POSES."""
    return [crafted_frame(), wavy_depth(W, H, 1.4), wavy_depth(W, H, 1.6)]


def box_coords(lo, n):
    """Every block of the box of n = (nx, ny, nz) blocks whose first block is lo, (B, 3) int32."""
    z, y, x = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    return (np.stack([x, y, z], -1).reshape(-1, 3) + np.asarray(lo)).astype(np.int32)


def dense_options(opts, lo_blocks, n_blocks):
    """The dense volume that covers the box of blocks: the same options, origin shifted by whole voxels (rounded once per axis)."""
    o = np.asarray(opts["origin"], f32); s = f32(opts["voxel_size"])
    origin = tuple(float(f32(o[a] + f32(8 * lo_blocks[a]) * s)) for a in range(3))
    return dict(opts, origin=origin, dims=tuple(8 * n for n in n_blocks))
