"""Inputs whose SHAPE is chosen against the tiles of the TSDF kernels (tests/test_gpu_tsdf_shapes.py on the device,
tests/test_tsdf_shape_cases_host.py on the host).  Test infrastructure only; needs the restatements, no GPU.

The tiles.  k_tsdf_integrate[_color] tiles the VOLUME: 64 x 4 threads, 16 voxels along z per thread.  The mesh passes walk the volume as
runs of 64 consecutive voxels, 4 runs per wave, 1024 voxels per block, and find a vertex index from the mask bytes of a 64-byte line.
k_tsdf_raycast[_color] tiles the FRAME: 16 x 16 pixels per block, 8 x 8 per wave.  The model target pads its planes to a multiple of 64
and block (0, 0) of the SoA ray-cast writes the padding.

  VOLUMES              the volume shapes: see the table below for the tile each one is about
  integrate_case       options, crafted start, marked voxels and the three steps of the integrate test at one shape (or at a slice of BIG)
  integrate_reference  the restatement's volume and counts after every step
  RAY_SIZES, RAY_POSES the frame sizes and poses of the ray-cast test; ray_volume the fused volume, ray_reference the restatement's output
  TARGET_FRAMES        the frames whose pixel count is no multiple of 64; target_source, stale_cloud, track_frames
  mesh_volume          an analytic field with colours at every shape of VOLUMES
  case_volume          all 256 corner-sign cases of a cell, one cell each, in three layouts

  (2, 2, 2)      the smallest volume icp_tsdf_options_check accepts: one cell, less than one run, one thread row of the integrate tile
  (64, 4, 16)    exactly one integrate tile; 64 runs, each one row: the neighbour at l + nx is the same lane of the next run
  (65, 5, 17)    one over on every axis: a second block along x, y and z that holds one voxel layer
  (128, 8, 32)   exactly 2 x 2 x 2 integrate tiles; every row is two runs
  (2, 3, 40)     nx = 2: 32 rows in one run, three z chunks the last of which is half full
  (128, 2, 2)    two voxels on y and z, rows of two runs; 512 voxels: half a mesh block
  (64, 16, 3)    every row one run, three layers: 3072 voxels, exactly three mesh blocks
  (2, 2, 130)    four voxels per layer: 16 layers in a run, nine z chunks, the last with two layers
  (32, 32, 2)    a plane of exactly 1024 voxels: one mesh block per layer, the neighbour at l + plane is the same thread of the next block

Placement of the integrate volumes.  The camera of the 40 x 30 frame sees x in [-0.9, 0.9] at a depth of 1.5 m.  Every volume spans the
depth of the frames' surface (1.0 .. 2.5 m) or sits inside its band, and all but (2, 2, 2) reach beyond the image on one axis or behind
the surface by more than the truncation, so each step updates some voxels and not all: test_tsdf_shape_cases_host.py asserts it."""
import functools

import numpy as np

import tsdf_color_restatement as TC
import tsdf_mesh_restatement as TM
import tsdf_restatement as TS
from icp_amd.synth import camera_sequence, tum_K, wavy_depth
from support import pose_of

f32, f64 = np.float32, np.float64
MINF = f32(-np.inf)
W, H = 40, 30
EYE = np.eye(4, dtype=f32)

VOLUMES = [(2, 2, 2), (64, 4, 16), (65, 5, 17), (128, 8, 32), (2, 3, 40), (128, 2, 2), (64, 16, 3), (2, 2, 130), (32, 32, 2)]
BIG = (128, 8, 32)
SLICES = [(64, 4, 16), (65, 5, 17), (2, 2, 2)]                       # volumes that must equal [:nz, :ny, :nx] of BIG's


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def camera_matrix():
    return tum_K(W)


def rcam_of(width, height):
    """The 40 x 30 camera's fx, fy, cx, cy with another width and height: a smaller frame is a crop from pixel (0, 0)."""
    return TS.Camera(camera_matrix(), width, height)


# ---- 1. integrate

# dims -> (voxel size, origin)
PLACEMENT = {(2, 2, 2): (0.05, (0.02, -0.04, 1.52)),
             (64, 4, 16): (0.04, (-1.3, -0.07, 1.2)),
             (65, 5, 17): (0.04, (-1.3, -0.09, 1.2)),
             (128, 8, 32): (0.02, (-0.7, -0.09, 1.6)),
             (2, 3, 40): (0.05, (0.1, -0.06, 0.6)),
             (128, 2, 2): (0.02, (-1.3, 0.01, 1.6)),
             (64, 16, 3): (0.04, (-1.3, -0.3, 1.55)),
             (2, 2, 130): (0.02, (-0.15, 0.1, 0.2)),
             (32, 32, 2): (0.05, (-0.8, -0.8, 1.6))}
INT_COMMON = dict(truncation=0.1, max_weight=2.0, min_depth=0.3, max_depth=2.4)
INT_POSES = (EYE, pose_of((0.1, -0.25, 0.05), (0.3, -0.1, 0.2)))      # test_gpu_tsdf.py's two poses


@functools.lru_cache(maxsize=None)
def integrate_frames():
    """The two depth frames of test_integrate_matches_restatement_bit_for_bit (every kind of depth the contract names) and a seeded colour
    frame for each.  Returns the three steps (depth, rgbx, pose): two frames at two poses, and the first once more."""
    d1 = wavy_depth(W, H)
    d1[0, :6] = [MINF, np.nan, np.inf, 0.0, -1.0, 2.5]                # 2.5 > max_depth
    d1[10:14, 20:24] = MINF
    d2 = wavy_depth(W, H, base=1.4); d2[5, 5] = np.nan
    rng = np.random.default_rng(40)
    c1, c2 = (rng.integers(0, 256, (W * H, 4), dtype=np.uint8) for _ in range(2))
    _frozen(d1, d2, c1, c2)
    return ((d1, c1, INT_POSES[0]), (d2, c2, INT_POSES[1]), (d1, c1, INT_POSES[0]))


def integrate_options(dims, place=None):
    s, origin = PLACEMENT[dims if place is None else place]
    return dict(INT_COMMON, dims=dims, origin=origin, voxel_size=s)


@functools.lru_cache(maxsize=None)
def _full_start(dims):
    """(tsdf, weight, rgb, wc, marked) of a whole volume at its own placement: arbitrary values, weights in {0, 1, 1.5}, and NaNs with a
    payload in a third of the voxels that no step writes."""
    opts = integrate_options(dims)
    vol = TS.Volume(**opts)
    shape = vol.tsdf.shape
    rng = np.random.default_rng(dims[0] * 10007 + dims[1] * 101 + dims[2])
    t0 = rng.uniform(-1, 1, shape).astype(f32); w0 = rng.choice(np.array([0, 1, 1.5], f32), shape)
    c0 = rng.uniform(0, 255, shape + (3,)).astype(f32); wc0 = rng.choice(np.array([0, 1, 1.5], f32), shape)
    written = np.zeros(shape, bool)
    for depth, _, pose in integrate_frames():
        written |= TC.integrate_masks(vol, depth, rcam_of(W, H), pose)[0]
    marked = ~written & (np.arange(written.size).reshape(shape) % 3 == 0)
    t0.view(np.uint32)[marked] = 0x7FC12345; w0.view(np.uint32)[marked] = 0xFFC54321
    c0.view(np.uint32)[marked] = 0x7FC0BEEF; wc0.view(np.uint32)[marked] = 0xFFC0FACE
    return _frozen(t0, w0, c0, wc0, marked)


@functools.lru_cache(maxsize=None)
def integrate_case(dims, of=None):
    """dict(opts, start (tsdf, weight, rgb, wc), marked, steps).  of = BIG: the volume `dims` with BIG's origin and voxel size, starting
    from the slice [:nz, :ny, :nx] of BIG's start."""
    nx, ny, nz = dims
    arrays = _full_start(dims if of is None else of)
    if of is not None:
        arrays = _frozen(*[np.ascontiguousarray(a[:nz, :ny, :nx]) for a in arrays])
    return dict(opts=integrate_options(dims, of), start=arrays[:4], marked=arrays[4], steps=integrate_frames())


def started_volume(case):
    vol = TC.add_color(TS.Volume(**case["opts"]))
    vol.tsdf, vol.weight, vol.rgb, vol.wc = (a.copy() for a in case["start"])
    return vol


@functools.lru_cache(maxsize=None)
def integrate_reference(dims, of=None):
    """The restatement after every step: [(updated, coloured, tsdf, weight, rgb, wc)].  TC.integrate_color writes tsdf and weight as
    TS.integrate does (the host test asserts it), so the plain device call is held against the same arrays."""
    case = integrate_case(dims, of)
    vol = started_volume(case)
    out = []
    for depth, rgbx, pose in case["steps"]:
        n, ncol = TC.integrate_color(vol, depth, rgbx, rcam_of(W, H), pose)
        out.append((n, ncol) + _frozen(vol.tsdf.copy(), vol.weight.copy(), vol.rgb.copy(), vol.wc.copy()))
    return out


# ---- 2. ray-cast

RAY_OPTS = dict(dims=(48, 40, 56), origin=(-1.9, -1.6, -0.4), voxel_size=0.08, truncation=0.32, max_weight=64.0, min_depth=0.3, max_depth=4.0)   # test_gpu_tsdf.RAY_OPTS
RAY_SIZES = [(1, 1), (8, 8), (16, 16), (17, 17), (32, 16), (64, 1), (1, 30), (33, 15), (40, 30)]
# The first two are test_gpu_tsdf.py's.  From both, column 0 of the image looks past what the two fused frames observed and (1, 30) has no
# hit, with this volume wherever it is put; the third pose turns the camera so that column 0 and pixel (0, 0) see the surface.
RAY_POSES = {"inside": EYE, "outside looking in": pose_of((0, 0, 0), (0.0, 0.0, -1.6)), "inside, turned": pose_of((-0.1, 0.3, 0), (0.0, 0.0, 0.0))}
ONE_PIXEL = {"inside": "hole", "outside looking in": "hole", "inside, turned": "hit"}      # what pixel (0, 0) is; asserted in the host test


@functools.lru_cache(maxsize=None)
def ray_frames():
    """The two frames test_gpu_tsdf.py and test_gpu_tsdf_color.py fuse their ray-cast volume from: (depth, rgbx, pose) each."""
    rng = np.random.default_rng(8)
    d1 = wavy_depth(W, H, base=1.6); d1[8:11, 30:34] = MINF
    c1 = rng.integers(0, 256, (W * H, 4), dtype=np.uint8)
    d2 = wavy_depth(W, H, base=1.55)
    c2 = rng.integers(0, 256, (W * H, 4), dtype=np.uint8)
    _frozen(d1, d2, c1, c2)
    return ((d1, c1, EYE), (d2, c2, pose_of((0.02, 0.12, -0.03), (-0.2, 0.05, 0.1))))


@functools.lru_cache(maxsize=None)
def ray_volume():
    """The volume of RAY_OPTS fused from ray_frames() by the restatement, with the colour array; two slabs of Wc = 0 cut the visible
    surface, as test_gpu_tsdf_color.raycast_case has them.  The device test fuses the same frames and asserts the same bits."""
    vol = TC.add_color(TS.Volume(**RAY_OPTS))
    for depth, rgbx, pose in ray_frames():
        TC.integrate_color(vol, depth, rgbx, rcam_of(W, H), pose)
    vol.fused_wc = _frozen(vol.wc.copy())
    vol.wc[:, :, 18:23] = 0; vol.wc[:, 14:17, :] = 0
    _frozen(vol.tsdf, vol.weight, vol.rgb, vol.wc)
    return vol


@functools.lru_cache(maxsize=None)
def ray_reference(size, pose_name):
    """TC.raycast_color of ray_volume() at one frame size: (depth (h, w), vertices, normals, rgba, hits, coloured hits, path).  Its first
    three arrays and its hit count are TS.raycast's."""
    out = TC.raycast_color(ray_volume(), rcam_of(*size), RAY_POSES[pose_name])
    _frozen(*[a for a in out if isinstance(a, np.ndarray)])
    return out


def crop(size, depth, vert, nrm, rgba=None):
    """[:h, :w] of the 40 x 30 output arrays, in the layout of a w x h output."""
    w, h = size
    out = [np.ascontiguousarray(depth[:h, :w]), np.ascontiguousarray(vert.reshape(H, W, 3)[:h, :w].reshape(-1, 3)),
           np.ascontiguousarray(nrm.reshape(H, W, 3)[:h, :w].reshape(-1, 3))]
    if rgba is not None:
        out.append(np.ascontiguousarray(rgba.reshape(H, W, 4)[:h, :w].reshape(-1, 4)))
    return out


# ---- 3. the model target with padding

TARGET_FRAMES = [(40, 30), (17, 17), (33, 15)]                       # n = 1200, 289, 495: 16, 31 and 17 padded entries
SOURCE_POSE = pose_of((0.01, 0.06, 0.0), (-0.1, 0.02, 0.05))         # "inside, between the poses" of test_gpu_tsdf.py
STALE_POINTS = 4096
TARGET_PARAMS = dict(n_iterations=10, max_distance=0.1, seed=0)
TRACK_MAX_DISTANCE = 1.0
ROOM_OPTS = dict(dims=(71, 35, 89), origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)    # test_gpu_tsdf.ROOM_OPTS


def padded(n):
    return (n + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def target_reference(size, color):
    """(vertices, normals, rgba, hits) of the target the model gives at the identity: TS.raycast's, or TC.colored_target's."""
    if color:
        v, n, rgba, hits = TC.colored_target(ray_volume(), rcam_of(*size), EYE)
        return _frozen(v, n, rgba) + (hits,)
    _, v, n, hits = TS.raycast(ray_volume(), rcam_of(*size), EYE)
    return _frozen(v, n) + (None, hits)


@functools.lru_cache(maxsize=None)
def target_source(size, color):
    """(points, normals, rgba) of the source: the model's (coloured) hits seen from SOURCE_POSE in a frame of this size, in that camera's
    frame, so that SOURCE_POSE itself aligns them with the target."""
    v, n, rgba, _ = TC.colored_target(ray_volume(), rcam_of(*size), SOURCE_POSE)
    if not color:
        _, v, n, _ = TS.raycast(ray_volume(), rcam_of(*size), SOURCE_POSE)
    keep = v[:, 2] != MINF
    return _frozen(np.ascontiguousarray(v[keep]), np.ascontiguousarray(n[keep]), np.ascontiguousarray(rgba[keep]))


def stale_cloud(moved):
    """STALE_POINTS points: entry i is point (i // k) mod n_j of moved[j], j = i mod k -- moved: k triples (points, normals, rgba) of n_j
    points each, the source as the matcher will see it at each moment the test asks about.  Every stretch of 16 consecutive entries, so
    every padding, holds copies from every triple."""
    k = len(moved)
    pts = np.empty((STALE_POINTS, 3), f32); nrm = np.empty((STALE_POINTS, 3), f32); rgba = np.empty((STALE_POINTS, 4), np.uint8)
    for j, (p, n, c) in enumerate(moved):
        i = np.arange(j, STALE_POINTS, k)
        pts[i] = p[(i // k) % len(p)]; nrm[i] = n[(i // k) % len(p)]; rgba[i] = c[(i // k) % len(p)]
    return pts, nrm, rgba


@functools.lru_cache(maxsize=None)
def track_frames(size):
    """(K, depth (3, h, w), rgbx (3, w h, 4), gt): three frames of the hand-held camera at 40 x 30 with 1 % holes, cropped from pixel
    (0, 0).  At this resolution neighbouring pixels lie up to half a metre apart in depth, so the source is built with TRACK_MAX_DISTANCE:
    with the default 0.1 the 17 x 17 crop keeps about 50 points, with 1.0 more than 160."""
    w, h = size
    K, depth, rgbx, gt = camera_sequence(3, W, H, hole_frac=0.01)
    depth = np.ascontiguousarray(depth[:, :h, :w])
    rgbx = np.ascontiguousarray(rgbx.reshape(3, H, W, 4)[:, :h, :w].reshape(3, w * h, 4))
    return K, _frozen(depth), _frozen(rgbx), gt


# ---- 4. mesh

MESH_VOXEL = 0.05
PLANE_SHAPES = [(128, 2, 2), (32, 32, 2), (64, 16, 3)]


@functools.lru_cache(maxsize=None)
def mesh_volume(dims):
    """A sphere of 0.8 voxel sizes' radius a little off the volume's centre, written as its signed distance; for PLANE_SHAPES the union
    with the half space behind an oblique plane through the centre, so vertices sit in many runs.  Colours as the mesh colour test has
    them: random channels, Wc in {0, 1, 7}."""
    s = MESH_VOXEL
    origin = (-0.31, 0.17, 0.43)
    centre = np.asarray(origin) + (np.asarray(dims) - 1) / 2.0 * s
    ball = TM.sphere(centre + np.array([0.13, -0.21, 0.17]) * s, 0.8 * s)
    if dims in PLANE_SHAPES:
        nrm = np.array([0.23, 0.61, 0.76]); nrm /= np.linalg.norm(nrm)
        fn = lambda P: np.minimum(ball(P), (P - (centre + 0.31 * s)) @ nrm)
    else:
        fn = ball
    vol = TC.add_color(TM.analytic_volume(fn, dims=dims, s=s, origin=origin))
    rng = np.random.default_rng(dims[0] * 10007 + dims[1] * 101 + dims[2])
    vol.rgb = rng.uniform(0, 255, vol.rgb.shape).astype(f32); vol.wc = rng.choice(np.array([0, 1, 7], f32), vol.wc.shape, p=[0.2, 0.4, 0.4])
    _frozen(vol.tsdf, vol.weight, vol.rgb, vol.wc)
    return vol


# ---- 5. the 256 cases of a cell

LAYOUTS = {"47x47x2": ((47, 47, 2), (0, 1, 2)),                      # dims, (axis of a, axis of b, the axis the two layers lie along)
           "64x47x2": ((64, 47, 2), (0, 1, 2)),                      # every row one run; the voxels beyond i = 46 are unobserved
           "2x47x47": ((2, 47, 47), (1, 2, 0))}                      # the stack turned: the cells lie in the y-z plane
ZERO_CORNERS = {0x00: (3,), 0x01: (6,), 0x17: (3, 5), 0x2C: (0, 4), 0x6A: (0,), 0x96: (0, 3), 0xE8: (0, 1, 2), 0xFE: (0,)}     # cell -> corners: +0.0 (even) / -0.0 (odd)


def case_magnitudes():
    """(256, 8) in [0.1, 0.9]: |F| of corner c of cell m; m and 255 - m share a row, so their vertices coincide."""
    mag = np.random.default_rng(256).uniform(0.1, 0.9, (128, 8)).astype(f32)
    return np.concatenate([mag, mag[::-1]])


@functools.lru_cache(maxsize=None)
def case_volume(layout):
    """Cell m = a + 16 b (a, b = 0..15) has its lowest corner at 3 a on the first plane axis and 3 b on the second, in a volume two layers
    thick, origin 0 and voxel size 1 (a vertex's coordinates name its cell exactly).  Voxels at 2 mod 3 on a plane axis are unobserved, so
    every cell is alone.  Corner c = dx + 2 dy + 4 dz (in the volume's own axes) of cell m is negative iff bit c of m is set; ZERO_CORNERS
    names non-negative corners that are exact zeros of either sign."""
    dims, (ax_a, ax_b, ax_l) = LAYOUTS[layout]
    vol = TC.add_color(TS.Volume(dims, (0.0, 0.0, 0.0), voxel_size=1.0))
    F = np.ones(vol.tsdf.shape, f32); Wt = np.zeros(vol.tsdf.shape, f32)
    mag = case_magnitudes()
    for m in range(256):
        for c in range(8):
            d = (c & 1, (c >> 1) & 1, c >> 2)
            p = [0, 0, 0]
            p[ax_a] = 3 * (m & 15) + d[ax_a]; p[ax_b] = 3 * (m >> 4) + d[ax_b]; p[ax_l] = d[ax_l]
            val = -mag[m, c] if (m >> c) & 1 else mag[m, c]
            if c in ZERO_CORNERS.get(m, ()):
                assert not (m >> c) & 1
                val = f32(-0.0) if c & 1 else f32(0.0)
            F[p[2], p[1], p[0]] = val; Wt[p[2], p[1], p[0]] = 1
    vol.tsdf, vol.weight = F, Wt
    rng = np.random.default_rng(257)
    vol.rgb = rng.uniform(0, 255, vol.rgb.shape).astype(f32); vol.wc = rng.choice(np.array([0, 1, 7], f32), vol.wc.shape, p=[0.2, 0.4, 0.4])
    _frozen(vol.tsdf, vol.weight, vol.rgb, vol.wc)
    return vol


def cell_of_vertices(layout, vert):
    """The cell number m of every vertex of a case volume's mesh, from its coordinates."""
    _, (ax_a, ax_b, _) = LAYOUTS[layout]
    g = np.floor(np.asarray(vert, f64))
    return (g[:, ax_a] // 3 + 16 * (g[:, ax_b] // 3)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def mesh_reference(kind, key):
    """(vertices, normals, triangles, colours) of the restatement for mesh_volume(key) (kind "shape") or case_volume(key) (kind "cases")."""
    vol = mesh_volume(key) if kind == "shape" else case_volume(key)
    return _frozen(*TM.mesh(vol)) + (_frozen(TC.mesh_colors(vol)),)
