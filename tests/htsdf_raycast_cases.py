"""The shapes the hashed ray-cast tests share (tests/test_htsdf_raycast_host.py, tests/test_gpu_htsdf_raycast.py), the smallest at which
the kernel can go wrong.  Volumes: htsdf_cases' fused frames (P: non-negative blocks only; NEG and STRADDLE on both sides of 0) and
htsdf_mesh_cases' analytic spheres on 1/8 m voxels (A one block; B 2 x 2 x 2 blocks around the grid origin; C: B with one block missing;
D 3 x 3 x 3 blocks with zero weights, NaN, inf and exact-zero values; F the single block at a corner of the storable range).  Every case
is (name, options, coords, tsdf, weight, poses): the arrays are computed once and are read-only, the poses were chosen on the CPU so that
the restatement's trace holds every class the host test asserts.  No device code."""
import functools
import numpy as np

import htsdf_cases as HC
import htsdf_mesh_cases as MC
import htsdf_raycast_restatement as RR
import htsdf_restatement as HR
import tsdf_restatement as TS
from icp_amd.synth import make_pose, tum_K

f32 = np.float32
SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (64, 48)]          # one ray; a partial tile; tile-exact; one over on both axes; several blocks
S = 0.125                                                        # the spheres' voxel size: a block is exactly 1 m


def camera(w, h):
    """(the library's camera, the restatements' camera) of w x h pixels at the TUM intrinsics scaled to the width."""
    from icp_amd import binding
    return binding.depth_camera(tum_K(w), w, h), TS.Camera(tum_K(w), w, h)


def pose(angles, position):
    return make_pose(angles, position).astype(f32)


def world(voxel):
    """The world position of a point given in voxel coordinates of the spheres' grid."""
    return np.asarray(MC.OPTS["origin"], np.float64) + np.asarray(voxel, np.float64) * S


def _toward(voxel, distance, angles=(0.0, 0.0, 0.0), back=(0.0, 0.0, 1.0)):
    """A camera looking along +z (turned by `angles`) from `distance` metres in front of `voxel` along -back."""
    return pose(angles, world(voxel) - distance * np.asarray(back, np.float64))


def look_at(eye, target):
    """A camera at `eye` whose +z axis points at `target` (both in voxel coordinates of the spheres' grid)."""
    e, t = world(eye), world(target)
    z = (t - e) / np.linalg.norm(t - e)
    x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, e
    return T.astype(f32)


D_OPTS = dict(MC.OPTS, ray_step=0.0625)                          # half a voxel: the march meets the few crafted voxels of D


@functools.lru_cache(maxsize=None)
def case_p():
    """htsdf_cases' three frames fused into BOX by the restatement of the hashed volume: every block at non-negative coordinates."""
    vol = HR.HVolume(**HC.BOX)
    _, cam = HC.camera()
    for d, P in zip(HC.frames(), HC.POSES):
        HR.integrate(vol, d, cam, P)
    c, t, w = MC._frozen(*vol.sorted_blocks())
    assert c.min() >= 0
    return c, t, w


def cases():
    """[(name, options, coords, tsdf, weight, [poses])]."""
    out = [("P", HC.BOX) + case_p() + ([HC.TILTED, HC.POSES[2], pose((0.0, 0.5, 0.0), (0.3, 0.0, -0.4))],)]
    for which in ("NEG", "STRADDLE"):
        opts, c, t, w = MC.case_h_host(which)
        out.append((which, opts, c, t, w, [HC.TILTED, pose((0.05, 0.4, -0.1), (-0.2, 0.1, -0.3))]))
    # A: from outside (the march enters the block, meets the sphere) and from inside it (the first valid sample is negative)
    out.append(("A", MC.OPTS) + MC.case_a() + ([_toward((3.3, 3.6, 3.4), 0.9, (0.05, -0.04, 0.02)), _toward((3.3, 3.6, 3.4), 0.3)],))
    # B, C: from outside along a diagonal, so that the rays cross the three block planes and their edges in the shell between the blocks'
    # hull and the sphere; and from 0.3 m in front of the cell (-1, -1, -1), the one cell whose corners lie in all eight blocks
    corner = (-0.48, -0.48, -0.48)
    views = [look_at((-10.0, -9.0, -11.0), MC.B_CENTRE), _toward(corner, 0.3), look_at((11.0, 1.0, -0.48), MC.B_CENTRE),
             _toward((-0.48, 6.6, -0.48), 0.3), _toward((6.6, -0.48, -0.48), 0.3)]
    out.append(("B", MC.OPTS) + MC.case_b() + (views,))
    for missing in ((0, 0, 0), (-1, -1, -1)):
        out.append(("C without %s" % (missing,), MC.OPTS) + MC.case_c(missing) + (views,))
    out.append(("D", D_OPTS) + MC.case_d() + ([look_at((-11.0, -6.0, -12.0), (4.3, 3.6, 4.4)), pose((0.0, 3.0, 0.2), world((6.0, 5.0, 20.0))), _toward((4.3, 3.6, 4.4), 0.3),
                                               pose((-0.9, 0.3, 0.0), world((2.0, -10.0, -6.0)))],))
    return out


def case_f():
    """The block at a corner of the storable range, the camera beside it: rays along -z and +x leave -2^23 .. 2^23 - 2 (invalid, no cast)."""
    b = np.array(MC.EDGE_BLOCK, np.float64) * 8
    views = [pose((0.0, 0.0, 0.0), world(b + (3.5, 3.5, -6.0))), pose((0.0, 1.2, 0.0), world(b + (-4.0, 3.5, 3.5))), pose((0.0, 3.14, 0.0), world(b + (3.5, 3.5, 12.0)))]
    return ("F", MC.OPTS) + MC.case_f() + (views,)


def shifted(case, by=2):
    """A case moved by `by` blocks on every axis (a block of the spheres' grid is exactly 1 m: the poses move with it), every block at
    non-negative coordinates: what the dense equality is stated on."""
    name, opts, c, t, w, poses = case
    assert abs(opts["voxel_size"] - S) < 1e-12
    moved = []
    for P in poses:
        Q = P.copy(); Q[:3, 3] = (P[:3, 3].astype(np.float64) + by).astype(f32)
        moved.append(Q)
    c2 = (c + by).astype(np.int32)
    assert c2.min() >= 0
    return (name + " shifted", opts, c2, t, w, moved)


def dense_lo0(opts, coords, t, w):
    """The dense volume of the equivalence: the same origin and voxel size, the blocks written from voxel (0, 0, 0) on, dims covering every
    block.  Returns (options for Context.tsdf_create / tsdf_restatement.Volume, tsdf, weight)."""
    dims = tuple(int(v) for v in (coords.max(0).astype(np.int64) + 1) * 8)
    T, W = HR.blocks_to_dense(coords, t, w, (0, 0, 0), dims)
    keep = ("origin", "voxel_size", "truncation", "max_weight", "min_depth", "max_depth", "ray_step")
    return dict({k: opts[k] for k in keep if k in opts}, dims=dims), T, W


def dense_equality_cases():
    """P as it is, A - D shifted to non-negative coordinates."""
    cs = cases()
    return [cs[0]] + [shifted(c) for c in cs if c[0][0] in "ABCD"]


def blocks_of(case, **over):
    name, opts, c, t, w, _ = case
    return RR.Blocks(c, t, w, **dict(opts, **over))


@functools.lru_cache(maxsize=None)
def restated(case_index, size_index, pose_index, which="all"):
    """The restatement's ray-cast of one (case, camera size, pose), computed once and shared: (depth, vertices, normals, hits, trace)."""
    cs = {"all": all_cases, "dense": dense_equality_cases}[which]()
    case = cs[case_index]
    w, h = SIZES[size_index]
    tr = {}
    d, v, n, hits = RR.raycast(blocks_of(case), camera(w, h)[1], case[5][pose_index], trace=tr)
    for a in (d, v, n):
        a.setflags(write=False)
    return d, v, n, hits, tr


@functools.lru_cache(maxsize=None)
def all_cases():
    return cases() + [case_f()]
