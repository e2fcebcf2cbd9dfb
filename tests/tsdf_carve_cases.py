"""Inputs of the carving cloud fuse (icp_set_tsdf_carve_options): numpy only, no device.
tests/test_tsdf_carve_host.py shows on the restatement that every case reaches the edge it is named for; tests/test_gpu_tsdf_carve.py
runs them on the device.  CASES maps a name to a dict:
  why       what the case is for
  opts      the volume's options; dims: the dense box, or None (hashed); capacity: the hashed volume's first block capacity
  alloc     hashed: block coordinates allocated (icp_tsdf_allocate_blocks) before the first step, or None
  carve     dict(distance, min_range)
  steps     [(cloud, pose, sensor origin or None, "source" | "target")], fused in turn into one volume
  copies    1, or how often the device's cloud repeats every point of the steps' clouds (the restatement fuses ONE copy: see replay)
  expect    figures counted BY HAND for the last step: any of n_carved, n_steps, n_samples, n_outside, n_blocks, n_updated"""
import functools
import numpy as np

import htsdf_restatement as HR
import tsdf_carve_restatement as CV
import tsdf_cloud_restatement as CR
import tsdf_cloud_cases as CC
from tsdf_cloud_cases import cloud, OPTS, DYADIC, TILTED, EYE, FLAT, translated

f32 = np.float32
INF = float("inf")
E = (0.05, -0.02, 0.1)


def block_box(lo, hi):
    """Every block coordinate of the box lo .. hi (inclusive), (n, 3) int32."""
    ax = [np.arange(lo[a], hi[a] + 1) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


def case(why, opts, steps, carve, dims=None, alloc=None, capacity=64, copies=1, **expect):
    steps = [(np.ascontiguousarray(s[0], f32), np.asarray(s[1], f32), s[2] if len(s) > 2 else None, s[3] if len(s) > 3 else "source") for s in steps]
    return dict(why=why, opts=opts, dims=dims, alloc=alloc, capacity=capacity, carve=dict(carve), steps=steps, copies=copies, expect=expect)


ALL_THE_WAY = dict(distance=INF, min_range=0.0)
# the wall under OPTS from TILTED: the sensor sits in block (-1, -1, -2), the wall in voxels z = -1 .. 15.  WALL_BLOCKS covers the middle of
# the space between them and leaves the sides out: rays cross resident and missing blocks in turn.
WALL_BLOCKS = block_box((-2, -2, -2), (1, 1, 0))
INSIDE = (dict(OPTS, origin=(-1.8, -1.8, -0.5)), (36, 36, 36))        # a box with the sensor in it; the wall leaves through its sides
OUTSIDE = (dict(OPTS, origin=(-1.2, -1.2, 0.6)), (24, 24, 20))        # the sensor 0.5 m in front of the box: every ray enters mid-walk

CASES = {}
for _n in (1, 63, 64, 65, 257, 3000):
    _cap = 1 << 10 if _n == 3000 else 64
    CASES["n%d/hashed" % _n] = case("%d points, blocks between sensor and wall resident in part" % _n, OPTS, [(cloud(_n), TILTED)], ALL_THE_WAY, alloc=WALL_BLOCKS, capacity=_cap)
    CASES["n%d/dense" % _n] = case("%d points, the sensor inside the box" % _n, INSIDE[0], [(cloud(_n), TILTED)], ALL_THE_WAY, dims=INSIDE[1])
CASES["target_with_origin/hashed"] = case("the target, a sensor origin under a tilted pose, min_range 0.5, then the source onto W = 1", OPTS,
                                          [(cloud(300, seed=5), TILTED, E, "target"), (cloud(257, seed=6), TILTED, E, "source")], dict(distance=INF, min_range=0.5), alloc=WALL_BLOCKS)
CASES["target_with_origin/dense"] = case("the same into the box", INSIDE[0], [(cloud(300, seed=5), TILTED, E, "target"), (cloud(257, seed=6), TILTED, E, "source")],
                                         dict(distance=INF, min_range=0.5), dims=INSIDE[1])
CASES["hostile_points/hashed"] = case("a NaN, an inf, a point at the sensor centre, one nearer than the truncation, one beyond max_depth", OPTS,
                                      [(np.concatenate([np.array([[np.nan, 0, 1], [0, np.inf, 1], E, [0.05, 0.0, 0.2], [0, 0, 7.5]], f32), cloud(70, seed=8)]), TILTED, E)], ALL_THE_WAY,
                                      alloc=WALL_BLOCKS)

# ---- the dyadic ray: DYADIC's grid (voxel 1/4 m, truncation 3 voxels, max_depth 6 m: J = 24 all the way), rays along +x, +y and -z from
# the voxel centre (0, 0, 0) to points 8 voxels (2 m) away.  r - truncation = 5 voxels: the carve samples sit ON the voxel centres 4, 3,
# 2, 1 and at t = 0 (m = -5, skipped: not > min_range), the band on 5 .. 11 (M = 6).  By hand, per ray: 4 carved, 7 samples.
AXES = np.array([[2.0, 0, 0], [0, 2.0, 0], [0, 0, -2.0]], f32)
AXES_BLOCKS = np.array([[0, 0, 0], [0, 0, -1]], np.int32)          # voxels 0 .. 7 of every ray (the band's blocks come with the touch)
DYADIC_BOX = (dict(DYADIC, origin=(-0.5, -0.5, -3.0)), (24, 16, 16))        # the sensor on voxel (2, 2, 12)
for _name, _carve, _count, _j, _why in (
        ("all_the_way", ALL_THE_WAY, 4, 24, "t = 1, 3/4, 1/2, 1/4 carved, t = 0 not"),
        ("min_range_on_a_sample", dict(distance=INF, min_range=0.5), 2, 24, "min_range == t_m exactly at m = -3: that sample is skipped"),
        ("distance_not_a_multiple", dict(distance=0.6, min_range=0.0), 3, 3, "distance 0.6 m at 0.25 m voxels: J = ceil(2.4) = 3"),
        ("starts_mid_ray", dict(distance=0.5, min_range=0.0), 2, 2, "distance shorter than r - truncation: the walk starts 2 voxels before the band")):
    CASES["dyadic/%s/hashed" % _name] = case(_why, DYADIC, [(AXES, EYE)], _carve, alloc=AXES_BLOCKS, n_carved=3 * _count, n_steps=_j, n_samples=21, n_outside=0, n_updated=3 * (7 + _count))
    CASES["dyadic/%s/dense" % _name] = case(_why, DYADIC_BOX[0], [(AXES, EYE)], _carve, dims=DYADIC_BOX[1], n_carved=3 * _count, n_steps=_j, n_samples=21, n_outside=0,
                                            n_updated=3 * (7 + _count))
# r = 2 voxels < truncation: r - truncation < 0, every m < 0 sample has t < 0; the band's own samples at t = 1/4 .. 5/4: 5 per ray
NEAR = (AXES * f32(0.25)).astype(f32)
CASES["dyadic/nearer_than_truncation/hashed"] = case("r < truncation: no carve sample", DYADIC, [(NEAR, EYE)], ALL_THE_WAY, alloc=AXES_BLOCKS, n_carved=0, n_steps=24, n_samples=15)
CASES["dyadic/nearer_than_truncation/dense"] = case("r < truncation: no carve sample", DYADIC_BOX[0], [(NEAR, EYE)], ALL_THE_WAY, dims=DYADIC_BOX[1], n_carved=0, n_steps=24, n_samples=15)


# ---- the join: along the space diagonal a step of one voxel moves every axis by 0.577 voxels, so two neighbouring samples share a voxel
# whenever all three stay on one side of their ties.  JOIN_SAME is the first range on a ladder whose m = -1 and m = 0 samples do.
def join_voxels(p):
    """(voxel of the sample at m = -1, voxel at m = 0) of the ray from FLAT's origin to p."""
    vol = HR.HVolume(**FLAT)
    c, u, r, _ = CR.rays(vol, np.asarray([p], f32), EYE)
    out = []
    for m in (-1, 0):
        t = np.fmin((r - vol.trunc) + f32(m) * vol.s, r + vol.trunc)
        out.append(tuple(int(np.floor(((c[a] + t * u[:, a]) - vol.o[a]) / vol.s + f32(0.5))[0]) for a in range(3)))
    return out


JOIN_LADDER = [np.array([x, x, x], f32) for x in np.arange(0.60, 0.80, 0.005)]
JOIN_SAME = next(p for p in JOIN_LADDER if join_voxels(p)[0] == join_voxels(p)[1])
JOIN_APART = np.array([1.0, 0.0, 0.0], f32)          # along an axis every sample has a voxel of its own
JOIN_BLOCKS = block_box((0, 0, 0), (0, 0, 0))
CASES["join/same_voxel"] = case("the m = -1 and m = 0 samples share a voxel: the band's first sample is skipped and not counted", FLAT, [(JOIN_SAME[None], EYE)], ALL_THE_WAY, alloc=JOIN_BLOCKS)
CASES["join/apart"] = case("the m = -1 and m = 0 samples lie in neighbouring voxels", FLAT, [(JOIN_APART[None], EYE)], ALL_THE_WAY, alloc=JOIN_BLOCKS, n_samples=7, n_carved=6)

# ---- hashed residency.  +x from the origin to x = 5 m under FLAT (voxel 0.1, truncation 0.3): the band on voxels 47 .. 53 (blocks 5 and
# 6, touched), the carve samples on voxels 46 .. 1 (min_range 0.05 keeps the sample at t ~ 0 out of the count).  Blocks 0, 2 and 4 are
# resident, 1 and 3 missing: carved are voxels 1 .. 7, 16 .. 23, 32 .. 39 and, in the touched block 5, 40 .. 46: 7 + 8 + 8 + 7 = 30.
ALTERNATE = np.array([[0, 0, 0], [2, 0, 0], [4, 0, 0]], np.int32)
CASES["residency/alternate"] = case("blocks alternately resident and missing along the ray; carving allocates none", FLAT, [(np.array([[5.0, 0, 0]], f32), EYE)],
                                    dict(distance=INF, min_range=0.05), alloc=ALTERNATE, n_carved=30, n_blocks=5, n_samples=7)
for _k, _d in ((1, (-1, 0, 0)), (2, (-1, -1, 0)), (3, (-1, -1, -1))):
    _c = np.array([0.45 if x else 0.05 for x in _d], f32)                       # the sensor in block 0 on the axes the ray moves along
    _u = np.array(_d, np.float64) / np.sqrt(_k)
    CASES["residency/across_zero_%d" % _k] = case("a ray across block 0 / -1 on %d axes, all eight blocks around the origin resident" % _k, FLAT,
                                                  [((_u * 1.5)[None].astype(f32), translated(*_c))], ALL_THE_WAY, alloc=block_box((-1, -1, -1), (0, 0, 0)))
CASES["residency/beyond_the_range"] = case("a pose near voxel 2 10^7: no sample is storable, carve samples do nothing and count nothing", OPTS,
                                           [(cloud(100, seed=7), CC.translated(2.0e6, -0.05, 0.02, rot=TILTED[:3, :3]))], ALL_THE_WAY, alloc=WALL_BLOCKS, n_carved=0, n_samples=0, n_updated=0,
                                           n_blocks=len(WALL_BLOCKS))
CASES["residency/straddle"] = case("a fan across the last storable voxel on +x: carve samples on the storable side", FLAT, [CC.RANGE_STRADDLE["x_plus"][1][0][2:4]], ALL_THE_WAY,
                                   alloc=block_box(((1 << 20) - 2, -1, -1), ((1 << 20) - 2, 0, 0)))          # (the sensor's own block, 2^20 - 3, is missing)

# ---- the dense box
CASES["box/sensor_outside"] = case("the sensor 0.5 m in front of the box: every ray enters it mid-walk", OUTSIDE[0], [(cloud(500, seed=12), TILTED)], ALL_THE_WAY, dims=OUTSIDE[1])
CASES["box/corner"] = case("DENSE_FACES' ray along the diagonal that leaves through the corner voxel, from two voxels further back", DYADIC,
                           [(np.array([[1.375, 1.125, 0.875]], f32), EYE, (-0.375, -0.625, -0.875))], ALL_THE_WAY, dims=CC.FACE_DIMS)
for _d in ((63, 3, 15), (65, 5, 17)):
    _o, _dims, _pts, _pose, _e, _ = CC.DENSE_SHAPES[CC.shape_name(_d)][1][0]
    CASES["box/%s" % CC.shape_name(_d)] = case("a box on one side of the fold's 64 x 4 x 16 tile, identity then a quarter turn", _o, [(_pts[:1200], EYE, _e), (_pts[:1200], CC.QUARTER_Y, _e)],
                                               ALL_THE_WAY, dims=_dims)

# ---- exact ones and the mixed voxel, on the dyadic grid.  HIT ends 2 m along +x: its band is voxels 5 .. 11.  PASS ends 4 m along +x
# (band 13 .. 19): it carves voxels 1 .. 12.  Voxels 1 .. 4: N = 2, S = 65536 (both pass, f = 1).  Voxel 5 (x = 1.25 m): HIT gives
# sdf = 0.75, f = 1, k = 32768; PASS gives 32768: S = 65536.  Voxel 8, on HIT's point: k = 0 and 32768, fbar = 1/2.  Voxel 11: HIT gives
# sdf = -0.75, f = -1, k = -32768; PASS 32768: S = 0.
HIT, PASS = [2.0, 0, 0], [4.0, 0, 0]
CASES["exact_ones"] = case("voxels carved from W = 0 read D == 1.0f, W == 1", DYADIC_BOX[0], [(np.array([PASS], f32), EYE)], ALL_THE_WAY, dims=DYADIC_BOX[1], n_carved=12, n_updated=19)
CASES["mixed_voxel"] = case("one ray hits a voxel, another passes through it: the integer average", DYADIC_BOX[0], [(np.array([HIT, PASS], f32), EYE)], ALL_THE_WAY, dims=DYADIC_BOX[1],
                            n_carved=4 + 12, n_updated=19)

# ---- lanes and combining.  A and B lie in different blocks; with WALL_BLOCKS resident both rays carve, and every copy of a point
# observes the same voxels: the wave combining meets runs of 64, runs cut by lane 0, alternating and single lanes.
PILE = case("2^17 + 1 copies of one point, 1 m carved: every carved voxel has N = 131073 and fbar == 1", OPTS, [(CC.PILE_POINT, EYE)],
            dict(distance=1.0, min_range=0.0), alloc=block_box((-1, -1, -2), (0, 0, 0)), copies=CC.PILE_N)
CASES["lanes/pile/hashed"] = PILE
CASES["lanes/pile/dense"] = case(PILE["why"], CC.PILE_BOX[0], [(CC.PILE_POINT, EYE)], dict(distance=1.0, min_range=0.0), dims=CC.PILE_BOX[1], copies=CC.PILE_N)
for _n, (_why, _p) in CC.LANE_CLOUDS.items():
    CASES["lanes/%s/hashed" % _n] = case(_why, OPTS, [(_p, EYE)], ALL_THE_WAY, alloc=block_box((-3, -2, -2), (1, 1, 1)))
    CASES["lanes/%s/dense" % _n] = case(_why, dict(OPTS, origin=(-2.4, -1.2, -0.3)), [(_p, EYE)], ALL_THE_WAY, dims=(40, 30, 56))


def new_volume(c):
    vol = CC.new_volume(c["opts"], c["dims"])
    if c["alloc"] is not None:
        vol.allocate(c["alloc"])
    return vol


COUNTED_PER_RAY = ("n_points", "n_rays", "n_samples", "n_outside", "n_carved")


def device_cloud(c, pts):
    """The cloud the device is given: every point `copies` times."""
    return np.repeat(pts, c["copies"], 0) if c["copies"] > 1 else pts


def replay(c, carve=None, after=None):
    """The case's steps fused by the restatement into a fresh volume under `carve` (None: the case's own).  -> (infos, stats, vol)
    A case with copies = n > 1 stands for a cloud that repeats every point n times: every voxel's S and N are n times those of one
    copy -- integers, exact -- and fbar = (float)((double)(n S) / ((double)(n N) 32768)) is the correctly rounded quotient of the same
    rational number as for one copy, so the folded volume is that of ONE copy bit for bit and only the per-ray counts scale.  The
    restatement therefore fuses one copy (tests/test_tsdf_carve_host.py checks the argument literally on a thousand copies)."""
    cv = c["carve"] if carve is None else carve
    vol = new_volume(c)
    infos, stats = [], []
    for k, (pts, pose, origin, _) in enumerate(c["steps"]):
        info, st = CV.integrate(vol, pts, pose, origin, **cv)
        for d in (info, st):
            for key in d:
                if key in COUNTED_PER_RAY:
                    d[key] *= c["copies"]
        infos.append(info); stats.append(st)
        if after:
            after(k, vol)
    return infos, stats, vol


@functools.lru_cache(maxsize=None)
def reference(name):
    """replay() of CASES[name], computed once; nobody writes into what it returns."""
    return replay(CASES[name])
