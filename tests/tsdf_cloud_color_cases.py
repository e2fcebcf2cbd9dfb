"""Inputs of the coloured laser-scan fuse (icp_tsdf_integrate_cloud_color): numpy only, no device.
tests/test_tsdf_cloud_color_host.py shows on the restatement that every case reaches what it is named for;
tests/test_gpu_tsdf_cloud_color.py runs them on the device.  CASES maps a name to a dict:
  why       what the case is for
  opts      the volume's options; dims: the dense box, or None (hashed); capacity: the hashed volume's first block capacity
  steps     fused in turn into one coloured volume: ("fuse", cloud, rgba, pose, sensor origin or None) or ("evict", centre, radius)
Volumes of a few thousand voxels, or a few dozen blocks; clouds of at most a few hundred points."""
import functools
import numpy as np

import htsdf_color_restatement as HC
import htsdf_evict_restatement as ER
import tsdf_cloud_color_restatement as KR
import tsdf_cloud_cases as CC
from tsdf_cloud_cases import cloud, OPTS, DYADIC, TILTED, EYE

f32 = np.float32


def colours(n, seed, alpha=255):
    """n rgba rows: random rgb bytes; alpha a constant, or None for random bytes."""
    r = np.random.default_rng(seed)
    c = r.integers(0, 256, (n, 4), dtype=np.uint8)
    if alpha is not None:
        c[:, 3] = alpha
    return c


def fuse(pts, rgba, pose=EYE, origin=None):
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3); rgba = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
    assert len(pts) == len(rgba)
    return ("fuse", pts, rgba, np.asarray(pose, f32), origin)


def case(why, opts, steps, dims=None, capacity=64):
    return dict(why=why, opts=opts, dims=dims, capacity=capacity, steps=list(steps))


# ---- the dyadic grid (voxel 1/4 m, truncation 3 voxels, M = 6): the sensor on a voxel centre, rays along +x.  A point p voxels away has
# its band samples at p - 3 .. p + 3 voxels; on a voxel centre v the distance is sdf = (p - v) / 4 m.
#   p = 8     samples ON the voxels 5 .. 11, sdf = 3/4 .. -3/4 m: all seven updated, all seven coloured (neither test is strict).
#   p = 8.4   samples at 5.4 .. 11.4: voxels 5 .. 11; voxel 5 has sdf = 0.85 m > truncation: updated (f = 1) and NOT coloured.
#   p = 7.6   samples at 4.6 .. 10.6: voxels 5 .. 11; voxel 11 has sdf = -0.85 m < -truncation: neither updated nor coloured.
DBOX = (dict(DYADIC, origin=(-0.5, -0.5, -3.0)), (24, 16, 16))       # 6144 voxels; the sensor (the world's origin) on voxel (2, 2, 12)
ROW = (12, 2)                                        # [z, y] of the +x rays' voxels in the dense box, x = 2 + v
ON, PAST, SHORT = [2.0, 0.0, 0.0], [2.1, 0.0, 0.0], [1.9, 0.0, 0.0]
OBLIQUE = [1.5, 1.5, -1.5]                           # along the space diagonal a step moves every axis by 0.58 voxels: voxels repeat
RED = [200, 17, 5, 255]
STORAGES = (("hashed", DYADIC, None), ("dense",) + DBOX)
WALL = dict(hashed=(OPTS, None), dense=(dict(OPTS, origin=(-1.8, -1.8, -0.5)), (36, 36, 36)))      # the sensor inside the box; the wall leaves through its sides
OUTSIDE = (dict(OPTS, origin=(-1.2, -1.2, 0.6)), (24, 24, 20))      # the sensor 0.5 m in front of the box
SIZES = (1, 255, 256, 257, 513)
HOSTILE = np.concatenate([np.array([[np.nan, 0, 1], [0, np.inf, 1], [-np.inf, 0, 2], [0.05, -0.02, 0.1], [0, 0, 7.5], [3.0, 3.0, 6.5]], f32), cloud(70, seed=8)])

CASES = {}
for _kind, _o, _d in STORAGES:
    CASES["one_point/" + _kind] = case("one ray: seven voxels, each the point's bytes exactly with Wc == 1", _o, [fuse([ON], [RED])], _d)
    CASES["two_rays_0_and_255/" + _kind] = case("two rays through the same voxels with bytes 0 and 255: the mean is 127.5", _o,
                                                [fuse([ON, ON], [[0, 255, 0, 9], [255, 0, 255, 200]])], _d)
    CASES["three_rays_thirds/" + _kind] = case("three rays whose mean (1/3, 2/3, 254 2/3) is not representable", _o,
                                               [fuse([ON, ON, ON], [[1, 0, 255, 1], [0, 1, 255, 2], [0, 1, 254, 3]])], _d)
    CASES["beyond_truncation/" + _kind] = case("the first band sample's voxel has sdf > truncation: updated, not coloured", _o, [fuse([PAST], [RED])], _d)
    CASES["behind_truncation/" + _kind] = case("the last band sample's voxel has sdf < -truncation: neither updated nor coloured", _o, [fuse([SHORT], [RED])], _d)
    CASES["oblique/" + _kind] = case("an oblique ray whose consecutive samples repeat voxels", _o, [fuse([OBLIQUE], [RED])], _d)
for _kind, (_o, _d) in WALL.items():
    for _n in SIZES:
        CASES["n%d/%s" % (_n, _kind)] = case("%d wall points under a tilted pose" % _n, _o, [fuse(cloud(_n), colours(_n, 100 + _n), TILTED)], _d)
    CASES["alpha_varies/" + _kind] = case("n257 with random alpha bytes: the same colours", _o, [fuse(cloud(257), np.concatenate([colours(257, 357)[:, :3], colours(257, 9, None)[:, 3:]], 1), TILTED)], _d)
    _perm = np.random.default_rng(11).permutation(257)
    CASES["shuffled/" + _kind] = case("n257 in another order: the same colours", _o, [fuse(cloud(257)[_perm], colours(257, 357)[_perm], TILTED)], _d)
    CASES["hostile_points/" + _kind] = case("NaN and inf points, one at the sensor centre, two beyond max_depth, among wall points", _o,
                                            [fuse(HOSTILE, colours(len(HOSTILE), 21), TILTED, (0.05, -0.02, 0.1))], _d)
    CASES["twice/" + _kind] = case("the same scan fused twice: Wc 1 -> 2", _o, [fuse(cloud(200, seed=4), colours(200, 31), TILTED)] * 2, _d)
    CASES["thrice_clamped/" + _kind] = case("three times with max_weight 2: Wc 1, 2, 2", dict(_o, max_weight=2.0), [fuse(cloud(200, seed=4), colours(200, 31), TILTED)] * 3, _d)
    CASES["two_scans/" + _kind] = case("two different scans, one after the other: the second starts from accumulators the first fold zeroed", _o,
                                       [fuse(cloud(200, seed=4), colours(200, 31), TILTED), fuse(cloud(220, seed=5), colours(220, 32), CC.pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05)))], _d)
CASES["leaving_the_box/dense"] = case("the sensor in front of the box: rays enter it mid-band and leave through its sides", OUTSIDE[0],
                                      [fuse(cloud(300, seed=12), colours(300, 41), TILTED)], OUTSIDE[1])
CASES["negative_blocks/hashed"] = case("a wall behind the origin: every block has a negative coordinate", OPTS,
                                       [fuse(cloud(150, seed=13), colours(150, 42), CC.translated(-3.0, -2.5, -4.0))])
for _cap in (1, 2):
    CASES["grows_inside/capacity_%d" % _cap] = case("block capacity %d and a scan of dozens of blocks: pool and colour pool grow inside the coloured call" % _cap, OPTS,
                                                    [fuse(cloud(300, seed=14), colours(300, 43), TILTED)], capacity=_cap)
CASES["accumulators_remade/hashed"] = case("a one-ray fuse at capacity 4, then a scan that grows the pool: the accumulators are re-made", DYADIC,
                                           [fuse([ON], [RED]), fuse(cloud(300, seed=15), colours(300, 44), TILTED)], capacity=4)
CASES["evict_between/hashed"] = case("an evict between two coloured fuses: the pool is compacted under the accumulators", OPTS,
                                     [fuse(cloud(300, seed=16), colours(300, 45), TILTED), ("evict", (0.0, 0.0, 2.0), 1.2),
                                      fuse(cloud(300, seed=17), colours(300, 46), CC.pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05)))])

# (n257 is cloud(257) with colours(257, 100 + 257): the twins above carry the same rgb bytes)
SAME_COLOURS = [("alpha_varies/" + k, "n257/" + k) for k in WALL] + [("shuffled/" + k, "n257/" + k) for k in WALL]
CARVED = ["one_point/hashed", "one_point/dense", "oblique/dense", "n257/hashed", "n257/dense", "n513/hashed", "hostile_points/dense", "leaving_the_box/dense",
          "twice/hashed", "thrice_clamped/dense", "grows_inside/capacity_1"]
CARVES = (dict(distance=0.5, min_range=0.0), dict(distance=float("inf"), min_range=0.0))


def new_volume(c):
    return KR.add_color(CC.new_volume(c["opts"], c["dims"]))


def replay(c, carve=None, after=None):
    """The case's steps applied by the restatement to a fresh coloured volume under `carve` (None: off).
    -> (per fuse step (info, carve stats, n_colored), vol); after(k, vol, uncoloured twin) is called behind every step, the twin a volume
    that went through the same steps with tsdf_carve_restatement's uncoloured fuse."""
    cv = dict(distance=0.0, min_range=0.0) if carve is None else carve
    vol, twin = new_volume(c), CC.new_volume(c["opts"], c["dims"])
    out = []
    for k, st in enumerate(c["steps"]):
        if st[0] == "evict":
            n, _ = ER.evict(vol, st[1], st[2]); ER.evict(twin, st[1], st[2])
            HC.drop_colors(vol)
            assert n > 0 and vol.blocks
        else:
            _, pts, rgba, pose, origin = st
            out.append(KR.integrate(vol, pts, rgba, pose, origin, **cv))
            KR.CV.integrate(twin, pts, pose, origin, **cv)
        if after:
            after(k, vol, twin)
    return out, vol


@functools.lru_cache(maxsize=None)
def reference(name):
    """replay() of CASES[name] without carving, computed once; nobody writes into what it returns."""
    return replay(CASES[name])


# ---- the tracking loop: four small scans of one wall, each in its own sensor frame, in the box of sdf_cloud_cases
def track_scans(n=1500):
    """(scans, colours, poses): the wall's colour is a function of the world point, so the scans agree where they overlap.  (With 600
    points a scan the first model is too sparse: 20 valid points against min_valid 64, and every alignment fails.)"""
    import sdf_cloud_cases as SK
    poses = SK.TRACK_POSES + [CC.pose_of((0.03, -0.028, 0.018), (0.09, -0.05, 0.045))]
    scans, cols = [], []
    for k, T in enumerate(poses):
        w = cloud(n, seed=30 + k).astype(np.float64)
        inv = np.linalg.inv(T.astype(np.float64))
        scans.append((w @ inv[:3, :3].T + inv[:3, 3]).astype(f32))
        rgb = np.clip(128 + 100 * np.sin(3.0 * w + np.array([0.0, 1.0, 2.0])), 0, 255).astype(np.uint8)
        cols.append(np.concatenate([rgb, np.full((n, 1), 255, np.uint8)], 1))
    return scans, cols, poses
