"""Inputs of the laser-scan fuse (icp_tsdf_integrate_cloud) at the edges of its shapes, ranges and accumulators: numpy
only, no device.  tests/test_tsdf_cloud_cases_host.py shows on the restatement that every case reaches what it is named for;
tests/test_gpu_tsdf_cloud_shapes.py runs them on the device.  A table maps a name to (reason, steps); a step is (options, dims or None
(hashed), cloud, pose, sensor origin or None, block capacity), and the steps of a case are fused in turn into one volume.

  DENSE_SHAPES    non-cubic boxes around the fold's 64 x 4 x 16 tile, axes of length 2; two poses, so the second fold starts from W = 1
  DENSE_FACES     dyadic rays in the planes where floorf(x + 0.5f) decides between the face layer and outside; an edge, a corner
  RANGE_STRADDLE  fans of short rays across the last storable voxel of the hashed volume, +- x and +- z
  PILE_UP         2^17 + 1 copies of one point (S beyond 32 bits, of both signs); four piles among a wall, shuffled
  SATURATION      max_weight 1.0 and 2.5, four fuses
  LANES           point orders made for the touch's rule about the lane to the left, at block capacity 64 and 1
  BAND            a band narrower than a voxel (M = 1) and one of 20 steps"""
import functools
import numpy as np

import htsdf_restatement as HR
import tsdf_cloud_restatement as CR
from support import pose_of

f32 = np.float32
OPTS = dict(origin=(0.25, 0.15, 1.3), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=6.0)
DYADIC = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.25, truncation=0.75, max_weight=64.0, min_depth=0.3, max_depth=6.0)
TILTED = pose_of((0.12, -0.2, 0.07), (0.1, -0.05, 0.02))
EYE = np.eye(4, dtype=f32)


def cloud(n, seed=3):
    """n points of a wavy wall 1 .. 3 m in front of the sensor, in the sensor frame."""
    r = np.random.default_rng(seed)
    a, b = r.uniform(-0.9, 0.9, n), r.uniform(-0.6, 0.6, n)
    z = 2.0 + 0.8 * np.sin(3 * a) * np.cos(2 * b)
    return np.stack([np.tan(a) * z, np.tan(b) * z, z], 1).astype(f32)


def translated(x=0.0, y=0.0, z=0.0, rot=None):
    T = np.eye(4, dtype=f32)
    if rot is not None:
        T[:3, :3] = np.asarray(rot, f32)
    T[:3, 3] = (x, y, z)
    return T


def new_volume(opts, dims):
    return HR.HVolume(**opts) if dims is None else CR.DVolume(dims, **opts)


def replay(case, after=None):
    """The case's steps fused by the restatement into a fresh volume; after(k, vol, info) is called behind every step.  -> (infos, vol)"""
    steps = case[1]
    vol = new_volume(steps[0][0], steps[0][1])
    infos = []
    for k, (_, _, pts, pose, origin, _) in enumerate(steps):
        infos.append(CR.integrate(vol, pts, pose, origin))
        if after:
            after(k, vol, infos[-1])
    return infos, vol


@functools.lru_cache(maxsize=None)
def reference(table, name):
    """replay() of TABLES[table][name], computed once; nobody writes into what it returns."""
    return replay(TABLES[table][name])


def sample_voxels(opts, pts, pose, origin=None):
    """(valid (M + 1, n) bool, g (M + 1, n, 3) float64): the nearest voxel of every sample of every ray, before any range test -- the
    contract's t_m and g_a once more, for the host conditions that ask where a single ray's samples fall."""
    vol = HR.HVolume(**opts)
    c, u, r, usable = CR.rays(vol, pts, pose, origin)
    valid, g = [], []
    with np.errstate(all="ignore"):
        for m in range(CR.n_steps(vol) + 1):
            t = np.fmin((r - vol.trunc) + f32(m) * vol.s, r + vol.trunc)
            valid.append(usable & (t > 0))
            g.append(np.stack([np.floor(((c[a] + t * u[:, a]) - vol.o[a]) / vol.s + f32(0.5)) for a in range(3)], 1).astype(np.float64))
    return np.array(valid), np.array(g)


# ---- DENSE_SHAPES: voxel 0.1, truncation 0.3, the box centred on the wall's middle (0, 0, 2)
# (icp_tsdf_options: every extent >= 2.  The thinnest boxes there are stand where an axis of length 1 would; REFUSED is asked for and refused.)
SHAPES = [(2, 2, 2), (2, 40, 33), (40, 2, 33), (40, 33, 2), (63, 3, 15), (64, 4, 16), (65, 5, 17), (129, 2, 31)]
REFUSED = [(1, 1, 1), (1, 40, 33), (40, 1, 33), (40, 33, 1)]
WALL = cloud(3000)
# 90 degrees about y (x' = z, z' = -x), then moved so that the wall, now around x' = 2, is around the box's middle again
QUARTER_Y = translated(-2.0, 0.0, 2.0, rot=[[0, 0, 1], [0, 1, 0], [-1, 0, 0]])
SENSOR_E = (0.05, -0.02, 0.1)
AS_TARGET = "65x5x17"                                # this case: a sensor origin, and the cloud as the target


def shape_name(d):
    return "%dx%dx%d" % d


def _shape_case(d):
    nx, ny, nz = d
    opts = dict(OPTS, origin=(-0.05 * nx, -0.05 * ny, 2.0 - 0.05 * nz))
    e = SENSOR_E if shape_name(d) == AS_TARGET else None
    return ("box %s: identity, then a quarter turn about y onto W = 1" % (d,), [(opts, d, WALL, EYE, e, 0), (opts, d, WALL, QUARTER_Y, e, 0)])


DENSE_SHAPES = {shape_name(d): _shape_case(d) for d in SHAPES}

# ---- DENSE_FACES: DYADIC's grid (voxel 1/4 m, origin 0, truncation 3 voxels, M = 6) on a 6 x 5 x 4 box.  In voxel units a sample's
# index is floorf(v + 0.5f).  A case is ONE call: the sensor centre c sits in the plane under test (pose EYE, sensor origin = c), its
# four rays run along +- the two other axes to points 4 voxels (1 m) away, so every sample keeps c's coordinate on the tested axis
# exactly (u is an axis, t u_a = 0) and the samples lie 1 .. 7 voxels from c along the ray, on integers.
# By hand, axis x, c = (v, 2, 1) voxels: +y reaches y = 3 .. 9 (3, 4 inside the 5 rows), -y 1 .. -5 (1, 0), +z 2 .. 8 (2, 3), -z 0 .. -6
# (0): 7 samples in range and 21 outside when v rounds into the box, 0 and 28 when it does not.  sdf = 1 m - 1/4 m per voxel walked,
# never below -3/4 m: all 7 are observed, k = 32768 for the first of every ray.  Axis y, c = (2, v, 1): +-x gives 3, 4, 5 and 1, 0, +-z
# as before: 8 / 20.  Axis z, c = (2, 2, v): +-x 3, 4, 5 and 1, 0, +-y 3, 4 and 1, 0: 9 / 19.
FACE_DIMS = (6, 5, 4)
FACE_MID = (2.0, 2.0, 1.0)
EPS = 2.0 ** -10
FACE_COUNTS = {0: 7, 1: 8, 2: 9}                     # n_samples == n_updated of an inside case, by the tested axis


def _face_case(axis, v):
    c = np.array(FACE_MID, np.float64); c[axis] = v
    pts = []
    for a in range(3):
        if a != axis:
            for sign in (4.0, -4.0):
                p = c.copy(); p[a] += sign
                pts.append(p * 0.25)
    return [(DYADIC, FACE_DIMS, np.array(pts, f32), EYE, tuple(float(x) for x in c * 0.25), 0)]


DENSE_FACES = {}
FACE_PAIRS = []                                      # (axis, layer index, name of the inside case, name of its twin outside)
for _a, _n in enumerate(FACE_DIMS):
    for _side, _in, _out, _layer in (("lo", -0.5, -0.5 - EPS, 0), ("hi", _n - 0.5 - EPS, _n - 0.5, _n - 1)):
        _names = ["%s_%s_%s" % ("xyz"[_a], _side, w) for w in ("in", "out")]
        DENSE_FACES[_names[0]] = ("axis %s at %r voxels: rounds to index %d, the face layer" % ("xyz"[_a], _in, _layer), _face_case(_a, _in))
        DENSE_FACES[_names[1]] = ("axis %s at %r voxels: rounds to %d, outside" % ("xyz"[_a], _out, -1 if _side == "lo" else _n), _face_case(_a, _out))
        FACE_PAIRS.append((_a, _layer, _names[0], _names[1]))
# along +x from (1, -1/2, -1/2): y and z both on the tie that rounds to 0; x = 2 .. 8, of which 2 .. 5 lie in the box: 4 in, 3 out
DENSE_FACES["edge"] = ("a ray along the box edge y = z = 0, both on the tie", [(DYADIC, FACE_DIMS, np.array([[1.25, -0.125, -0.125]], f32), EYE, (0.25, -0.125, -0.125), 0)])
# along +x from (-2, 2, 1) to (2, 2, 1): x = -1 .. 5, all but the first in the box; the last sample's voxel is exactly the truncation
# behind the point (sdf = 1 - 7/4 = -3/4, which is not < -3/4): observed, f = -1, k = -32768
DENSE_FACES["band_end"] = ("the last sample's sdf equals -truncation exactly: observed", [(DYADIC, FACE_DIMS, np.array([[0.5, 0.5, 0.25]], f32), EYE, (-0.5, 0.5, 0.25), 0)])
# along the diagonal to the box's outer corner (5.5, 4.5, 3.5): not dyadic (no diagonal has a dyadic unit vector), the restatement decides
DENSE_FACES["corner"] = ("a ray along the diagonal that leaves through the corner voxel (5, 4, 3)",
                         [(DYADIC, FACE_DIMS, np.array([[1.375, 1.125, 0.875]], f32), EYE, (0.125, -0.125, -0.375), 0)])

# ---- RANGE_STRADDLE: hashed, voxel 0.1, origin 0: the storable voxels end at 2^23 - 1 (838 860.7 m) and -2^23 (-838 860.8 m)
FLAT = dict(OPTS, origin=(0.0, 0.0, 0.0))
EDGE_AT = 838859.0


def _fan(axis, sign):
    """21 points 1.5 .. 2.5 m ahead along sign * axis, a few centimetres to the side."""
    k = np.arange(21)
    p = np.zeros((21, 3))
    p[:, axis] = sign * (1.5 + 0.05 * k)
    p[:, (axis + 1) % 3] = 0.03 * (k % 5 - 2)
    p[:, (axis + 2) % 3] = 0.02 * (k % 3 - 1)
    return p.astype(f32)


RANGE_STRADDLE = {}
for _a in (0, 2):
    for _s, _sn in ((1.0, "plus"), (-1.0, "minus")):
        _t = [0.0, 0.0, 0.0]; _t[_a] = _s * EDGE_AT
        RANGE_STRADDLE["%s_%s" % ("xyz"[_a], _sn)] = ("a fan across the last storable voxel on %s%s" % ("+" if _s > 0 else "-", "xyz"[_a]),
                                                      [(FLAT, None, _fan(_a, _s), translated(*_t), None, 64)])

# ---- PILE_UP: hashed under OPTS, and in a box that holds the piles and cuts the wall
PILE_POINT = np.array([[0.3, 0.2, 1.5]], f32)
PILE_N = (1 << 17) + 1
PILE_BOX = (dict(OPTS, origin=(-1.0, -0.8, 0.9)), (21, 17, 19))


def _mixed():
    four = np.array([[0.3, 0.2, 1.5], [0.3, 0.2, 1.6], [-0.4, 0.1, 2.0], [0.0, 0.0, 2.5]], f32)
    pts = np.concatenate([np.repeat(four, 16384, 0), cloud(2000, seed=51)])
    return pts[np.random.default_rng(52).permutation(len(pts))]


PILE_UP = {}
for _kind, (_o, _d) in (("hashed", (OPTS, None)), ("dense", PILE_BOX)):
    PILE_UP["one_point/" + _kind] = ("2^17 + 1 copies of one point: N = 131073, S beyond 2^32 and below 0", [(_o, _d, np.repeat(PILE_POINT, PILE_N, 0), EYE, None, 64)])
    PILE_UP["four_piles_in_a_wall/" + _kind] = ("four points x 16384 copies among 2000 wall points, shuffled", [(_o, _d, _mixed(), EYE, None, 256)])

# ---- SATURATION: four fuses, the clouds alternating, the pose shifted a little each time
SAT_BOX = (-1.8, -1.8, -0.5), (44, 40, 36)
SAT_WEIGHTS = {1.0: [1.0, 1.0, 1.0, 1.0], 2.5: [1.0, 2.0, 2.5, 2.5]}
SATURATION = {}
for _mw in SAT_WEIGHTS:
    for _kind in ("hashed", "dense"):
        _o = dict(OPTS, max_weight=_mw) if _kind == "hashed" else dict(OPTS, max_weight=_mw, origin=SAT_BOX[0])
        _d = None if _kind == "hashed" else SAT_BOX[1]
        SATURATION["max_weight_%s/%s" % (_mw, _kind)] = ("max_weight %s: the cap is reached and held" % _mw, [
            (_o, _d, cloud(800, seed=61 + (k & 1)), pose_of((0.0, 0.01 * k, 0.0), (0.01 * k, 0.0, -0.005 * k)), None, 256) for k in range(4)])

# ---- LANES: hashed, orders of points made for k_htsdf_touch_cloud's rule (a lane skips the touch when the lane to its left holds the
# same block key); A and B lie in different blocks, RUN_A and RUN_B behind the wall where nothing else reaches
A, B = (0.3, 0.2, 1.5), (-1.4, 0.9, 2.6)
RUN_A, RUN_B, LONE = (0.5, 0.5, 5.0), (-1.0, 0.3, 4.5), (-2.0, 1.0, 4.0)
NANS = (np.nan, np.nan, np.nan)


def _runs():
    p = cloud(300, seed=71)
    p[60:71] = RUN_A; p[250:263] = RUN_B
    return p


def _last_wave_of_one():
    p = cloud(193, seed=72)
    p[192] = LONE
    return p


LANE_CLOUDS = {
    "same_256": ("256 copies of one point: every lane's left neighbour holds its key", np.array([A] * 256, f32)),
    "abab": ("A B A B ... for 192 points: no lane's left neighbour holds its key", np.array([A, B] * 96, f32)),
    "nan_between": ("A A NaN A A: the lane behind the NaN has an empty left neighbour", np.array([A, A, NANS, A, A], f32)),
    "runs": ("equal points at 60 .. 70 (across a wave's first lane) and 250 .. 262 (across a work-group's)", _runs()),
    "last_wave_of_one": ("193 points: the last wave holds one point, in blocks of its own", _last_wave_of_one()),
}
LANES = {"%s/capacity_%d" % (n, cap): (why, [(OPTS, None, p, EYE, None, cap)]) for n, (why, p) in LANE_CLOUDS.items() for cap in (64, 1)}

# ---- BAND: M = ceil(2 truncation / s) = 1 and 20 at voxel 0.1
BAND_BOX = (-2.2, -1.8, 0.0), (44, 36, 40)
BAND_STEPS = {0.04: 1, 1.0: 20}
BAND = {}
for _tr in BAND_STEPS:
    for _kind in ("hashed", "dense"):
        _o = dict(OPTS, truncation=_tr) if _kind == "hashed" else dict(OPTS, truncation=_tr, origin=BAND_BOX[0])
        BAND["truncation_%s/%s" % (_tr, _kind)] = ("truncation %s at voxel 0.1: M = %d" % (_tr, BAND_STEPS[_tr]),
                                                   [(_o, None if _kind == "hashed" else BAND_BOX[1], cloud(300, seed=81), TILTED, None, 64)])

TABLES = dict(DENSE_SHAPES=DENSE_SHAPES, DENSE_FACES=DENSE_FACES, RANGE_STRADDLE=RANGE_STRADDLE, PILE_UP=PILE_UP, SATURATION=SATURATION, LANES=LANES, BAND=BAND)
ALL = [(t, n) for t, cases in TABLES.items() for n in cases]
