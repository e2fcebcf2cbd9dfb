"""Inputs whose BLOCK COUNT is chosen, for the fold of k_sdf_solve / k_sdf_solve_color over the columns of partials[28 or 29][n_blocks] and
counts[2 or 3][n_blocks] (tests/test_gpu_fold_sizes.py on the device, tests/test_fold_cases_host.py on the host).  Test infrastructure
only; needs the restatements, no GPU.

The fold takes, per lane, the blocks lane, lane + 64, lane + 128, lane + 192 in one round trip and advances by 256 (sums), eight blocks per
round trip and 512 (counts): the block counts here sit on both sides of 64, 256 and 512, and at the workload's 1200.

  SDF_CASES          blocks -> (width, height, stride): the frames of direct SDF tracking, 16 x 16 sampled pixels per block
  COLOR_BLOCKS       the SDF cases that are also run with the photometric term (29 sums, 3 counts)
  VG_CASES           blocks -> source points of voxelized GICP, 512 points per block
  sdf_volume(color)  the analytic volume in the restatement's hands, observed everywhere but for ZERO_WEIGHT (and ZERO_COLOR_WEIGHT)
  sdf_case(blocks)   camera matrix, depth frame with its holes, colour frame
  vg_target(), vg_source(blocks)
  premises(case)     from the restatement alone: per block the usable, valid and coloured counts and the share of the cost sum (index 27),
                     next to the bound the device test grants that sum
  check_premises     what must hold for the device test to prove anything: see there

The holes of a frame.  On the sampled grid a pixel (su, sv) with (7 su + 13 sv) mod 31 = 0, 1, 2 or 3 is MINF, NaN, 2.5 m (beyond
max_depth) or 0.3 m behind the surface (usable, but the field is clamped at -1 there: not valid): a lattice that takes 4 of 31 pixels and
leaves no 16 x 16 tile, whole or partial, without a valid one.  So W H > n_depth > n_valid in every frame, and in every block that holds 31
sampled pixels or more.  In the 1200-block frame (OUTLIER_BLOCKS) a pixel where it is 4 or 5 lies 0.1 m behind or in front of the
surface: valid, with a residual of twice the Huber bound 0.05 that the 257- and 1200-block cases are also run with.  At SDF_NEAR the
surface's own residuals stay below 0.041 m, so elsewhere that bound runs the kernel's Huber branch and changes no weight.  The 4100 x 9 strip
cannot carry such pixels: it constrains a rotation about its own axis so weakly (smallest over largest eigenvalue of H 5e-7) that they send
its first step 5 rad away, in the restatement as on the device, and its steps are followed too.

The voxels of weight 0.  A voxel of weight 0 takes the 2 x 2 x 2 cells around it, 10 cm across, out of every frame.  At 640 x 480 a block
sees 4.6 cm of the surface and on the 4100 x 9 strip 6 x 3 mm, so such a voxel next to the surface empties whole blocks of those frames.
ZERO_WEIGHT and ZERO_COLOR_WEIGHT were therefore found by a search on the restatement (candidates next to the surface, one kept only if no
block of any case lost its last valid, or its last coloured, pixel) and are written down here as voxel indices.  Nothing rests on trusting
the search: check_premises asserts its outcome for the inputs as they are."""
import functools

import numpy as np

import sdf_color_restatement as SC
import sdf_restatement as SR
import tsdf_restatement as TS
import vgicp_restatement as VR
from support import pose_of

f32, f64 = np.float32, np.float64
MINF = f32(-np.inf)

VOLUME = dict(dims=(64, 48, 40), origin=(-1.6, -1.2, 0.6), voxel_size=0.05, truncation=0.2, min_depth=0.3, max_depth=2.4)
SDF_NEAR = ((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))            # test_gpu_sdf.NEAR (asserted equal in test_fold_cases_host.py)
SDF_CASES = {6: (40, 30, 1),               # the small neighbour of test_gpu_sdf.py's frame: 3 x 2 blocks
             16: (1280, 16, 5),            # 256 x 4 sampled pixels of a wide frame: the block count follows the sampled grid
             64: (128, 128, 1),            # u = 0 full, nothing else
             65: (208, 80, 1),             # one lane of u = 1
             256: (256, 256, 1),           # one full round
             257: (4100, 9, 1),            # one lane of the second round; partial tiles on both axes
             512: (512, 256, 1),           # two full rounds; one full round of the counts
             513: (420, 300, 1),           # one lane of the counts' second round
             1200: (640, 480, 1)}          # the workload: five rounds, the last with u = 2 partly filled
HUBERS = {257: (0.0, 0.05), 1200: (0.0, 0.05)}                    # elsewhere (0.0,)
COLOR_BLOCKS = (65, 257, 513, 1200)
COLOR_WEIGHT = 0.1
BEHIND, OUTLIER = f32(0.3), f32(0.1)
OUTLIER_BLOCKS = (1200,)

VG_NEAR = ((0.012, -0.009, 0.015), (0.02, -0.015, 0.01))          # test_gpu_vgicp.NEAR
VG_VOXEL, VG_EPS, VG_TARGET_POINTS, VG_BLOCK = 0.1, 1e-3, 20000, 512
VG_CASES = {64: 32768, 65: 32769, 256: 131072, 257: 131073, 512: 262144, 513: 262145}
VG_MIN_POINTS = {257: (1, 3)}                                     # elsewhere (1,)

# (z, y, x) indices into the (40, 48, 64) arrays
ZERO_WEIGHT = ((13, 43, 20), (16, 39, 27), (16, 42, 32), (17, 33, 13), (18, 4, 48), (18, 24, 13), (18, 24, 28), (18, 30, 11), (18, 40, 51), (20, 16, 49),
               (20, 22, 35), (20, 23, 58), (20, 33, 47), (21, 29, 54))
ZERO_COLOR_WEIGHT = ((15, 37, 26), (15, 38, 12), (17, 38, 29), (18, 33, 12), (18, 35, 57), (19, 38, 51), (20, 23, 55), (20, 24, 35), (20, 29, 37))


def hubers(blocks):
    return HUBERS.get(blocks, (0.0,))


def min_points(blocks):
    return VG_MIN_POINTS.get(blocks, (1,))


def sdf_blocks(width, height, stride):
    """ceil(ws / 16) ceil(hs / 16) with ws x hs the sampled grid: what this file claims; the host test holds it against sdf_plan's text."""
    ws, hs = (width + stride - 1) // stride, (height + stride - 1) // stride
    return ((ws + 15) // 16) * ((hs + 15) // 16)


def camera_matrix(width, height):
    """fx = fy = 525 W / 640, the principal point at the image centre (tum_K's cy lies far outside a strip)."""
    fx = 525.0 * width / 640.0
    return np.array([[fx, 0, (width - 1) / 2.0], [0, fx, (height - 1) / 2.0], [0, 0, 1]], f32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def _observed_volume():
    """The field clip((s(x, y) - z) / 0.2, -1, 1), s = 1.5 + 0.12 sin(2.5 x) + 0.1 cos(3 y), weight 1 everywhere: what the frames are cast from."""
    vol = TS.Volume(**VOLUME)
    x = (f64(vol.o[0]) + np.arange(vol.nx) * f64(vol.s))[None, None, :]; y = (f64(vol.o[1]) + np.arange(vol.ny) * f64(vol.s))[None, :, None]
    z = (f64(vol.o[2]) + np.arange(vol.nz) * f64(vol.s))[:, None, None]
    s = 1.5 + 0.12 * np.sin(2.5 * x) + 0.1 * np.cos(3.0 * y)
    vol.tsdf = np.clip((s - z) / f64(vol.trunc), -1.0, 1.0).astype(f32)
    vol.weight = np.ones_like(vol.tsdf)
    _frozen(vol.tsdf, vol.weight)
    return vol


@functools.lru_cache(maxsize=None)
def sdf_volume(color=False):
    """The volume the frames are evaluated against: the observed one with ZERO_WEIGHT; color: SC.smooth_colors with ZERO_COLOR_WEIGHT (the
    way tests/test_gpu_sdf_color.py colours its volume).  Read-only."""
    vol = TS.Volume(**VOLUME)
    vol.tsdf = _observed_volume().tsdf
    w = np.ones_like(vol.tsdf)
    for i in ZERO_WEIGHT:
        w[i] = 0
    vol.weight = _frozen(w)
    if color:
        SC.smooth_colors(vol)
        for i in ZERO_COLOR_WEIGHT:
            vol.wc[i] = 0
        _frozen(vol.rgb, vol.wc)
    return vol


def rendered_colors(vol, depth, rcam, pose):
    """test_gpu_sdf_color.rendered_colors without a shift: the colour frame a camera at `pose` sees of the volume's intensity field."""
    t = SR.pixel_terms(vol, depth, rcam, pose)
    Sv, _, ok = SC.sample_color(vol, t["q"])
    byte = np.clip(np.floor(np.where(ok > 0, Sv, 0).astype(f64) / 3.0 + 0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([byte, byte, byte, np.full(len(byte), 255, np.uint8)], 1))


@functools.lru_cache(maxsize=None)
def sdf_case(blocks):
    """dict(blocks, width, height, stride, K, depth (h, w) with its holes, rgbx (w h, 4): the volume's own colours seen from the identity
    with every seventh pixel a random colour, as tests/test_gpu_sdf_color.py has it).  Read-only."""
    width, height, stride = SDF_CASES[blocks]
    K = camera_matrix(width, height)
    rcam = TS.Camera(K, width, height)
    eye = np.eye(4, dtype=f32)
    cast = TS.raycast(_observed_volume(), rcam, eye)[0]
    rgbx = rendered_colors(sdf_volume(True), cast, rcam, eye)
    rgbx[::7, :3] = np.random.default_rng(blocks).integers(0, 256, (len(rgbx[::7]), 3), dtype=np.uint8)
    depth = cast.copy()
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    on_grid = (u % stride == 0) & (v % stride == 0)
    k = np.where(on_grid, (7 * (u // stride) + 13 * (v // stride)) % 31, -1)
    depth[k == 0] = MINF; depth[k == 1] = np.nan; depth[k == 2] = 2.5
    depth[k == 3] = cast[k == 3] + BEHIND
    if blocks in OUTLIER_BLOCKS:
        depth[k == 4] = cast[k == 4] + OUTLIER; depth[k == 5] = cast[k == 5] - OUTLIER
    return dict(blocks=blocks, width=width, height=height, stride=stride, K=_frozen(K), cast=_frozen(cast), depth=_frozen(depth), rgbx=_frozen(rgbx))


def rcam_of(case):
    return TS.Camera(case["K"], case["width"], case["height"])


def sdf_pose():
    return pose_of(*SDF_NEAR)


def surface(x, y):
    """(z, unit normal) of z = 0.3 sin 2x + 0.2 cos 3y."""
    z = 0.3 * np.sin(2.0 * x) + 0.2 * np.cos(3.0 * y)
    n = np.stack([-0.6 * np.cos(2.0 * x), 0.6 * np.sin(3.0 * y), np.ones_like(x)], 1)
    return z, n / np.linalg.norm(n, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def vg_target():
    """(points, normals, the restatement's grid at VG_VOXEL): 20 000 points on the surface over [-1, 1]^2.  Read-only."""
    r = np.random.default_rng(20000)
    x, y = r.uniform(-1, 1, VG_TARGET_POINTS), r.uniform(-1, 1, VG_TARGET_POINTS)
    z, n = surface(x, y)
    pts, nrm = _frozen(np.stack([x, y, z], 1).astype(f32), n.astype(f32))
    return pts, nrm, VR.grid(pts, nrm, VG_VOXEL)


@functools.lru_cache(maxsize=None)
def vg_source(blocks):
    """(points, normals): VG_CASES[blocks] points of the target's surface; every 97th position NaN, every 89th normal zero; the last point,
    which may be alone in the last block, is valid: it lies in the middle of the surface with its own normal.  Read-only."""
    n = VG_CASES[blocks]
    r = np.random.default_rng(n)
    x, y = r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    x[-1], y[-1] = 0.13, -0.21
    z, nr = surface(x, y)
    pts, nrm = np.stack([x, y, z], 1).astype(f32), nr.astype(f32)
    i = np.arange(n - 1)
    pts[i[i % 97 == 0]] = np.nan
    nrm[i[i % 89 == 5]] = 0
    return _frozen(pts, nrm)


def vg_pose():
    return pose_of(*VG_NEAR)


def _per_block(block, n_blocks, mask, weights=None):
    return np.bincount(block[mask], weights=None if weights is None else weights[mask], minlength=n_blocks)


def sdf_premises(blocks, color=False):
    """From the restatement alone, at SDF_NEAR: dict(n_blocks, counts, usable / valid / colored (per block), share (per block and Huber bound:
    the block's part of the cost sum, index 27), bound (per Huber bound: what the device test grants that sum))."""
    c = sdf_case(blocks)
    vol, rcam, stride = sdf_volume(color), rcam_of(c), c["stride"]
    gx = ((c["width"] + stride - 1) // stride + 15) // 16; gy = ((c["height"] + stride - 1) // stride + 15) // 16
    t = SC.pixel_terms(vol, c["depth"], c["rgbx"], rcam, sdf_pose(), stride) if color else SR.pixel_terms(vol, c["depth"], rcam, sdf_pose(), stride)
    block = (t["v"] // stride // 16) * gx + (t["u"] // stride // 16)
    n_blocks = gx * gy
    m = t["valid"]
    out = dict(n_blocks=n_blocks, usable=_per_block(block, n_blocks, t["usable"]), valid=_per_block(block, n_blocks, m), share={}, bound={})
    out["counts"] = (int(t["usable"].sum()), int(m.sum()))
    n_terms = int(m.sum())
    pho = np.zeros(len(m), f64)
    if color:
        col = t["colored"]
        out["colored"] = _per_block(block, n_blocks, col)
        out["counts"] += (int(col.sum()),)
        n_terms += int(col.sum())
        w2 = f64(f32(COLOR_WEIGHT)) * f64(f32(COLOR_WEIGHT))
        with np.errstate(all="ignore"):
            pho[col] = (w2 * t["r_c"][col]) * t["r_c"][col]
    for h in hubers(blocks):
        with np.errstate(all="ignore"):
            term = np.where(m, (SC._huber(t["r"], h) * t["r"]) * t["r"], 0.0) + pho
        out["share"][h] = _per_block(block, n_blocks, m, term)
        out["bound"][h] = n_terms * 2.0 ** -52 * float(np.abs(term[m]).sum())
    return out


def vg_premises(blocks):
    """sdf_premises for a voxelized GICP case at VG_NEAR: usable = considered, share and bound per min_points."""
    pts, nrm = vg_source(blocks)
    g = vg_target()[2]
    n_blocks = (len(pts) + VG_BLOCK - 1) // VG_BLOCK
    block = np.arange(len(pts)) // VG_BLOCK
    out = dict(n_blocks=n_blocks, share={}, bound={}, valid={}, counts={})
    for mp in min_points(blocks):
        t = VR.point_terms(g, pts, nrm, vg_pose(), VG_EPS, mp)
        term = t["N"] * np.einsum("na,nab,nb->n", t["r"], t["M"], t["r"])
        out["usable"] = np.bincount(block[t["considered"]], minlength=n_blocks)
        out["valid"][mp] = np.bincount(block[t["index"]], minlength=n_blocks)
        out["share"][mp] = np.bincount(block[t["index"]], weights=term, minlength=n_blocks)
        out["bound"][mp] = len(term) * 2.0 ** -52 * float(np.abs(term).sum())
        out["counts"][mp] = (int(t["considered"].sum()), len(term))
        out["last_valid"] = bool(t["valid"][-1])
    return out


CASES = [("sdf", b) for b in SDF_CASES] + [("sdf_color", b) for b in COLOR_BLOCKS] + [("vgicp", b) for b in VG_CASES]


def premises(case):
    """case: one of CASES, (kind, blocks)."""
    kind, blocks = case
    return vg_premises(blocks) if kind == "vgicp" else sdf_premises(blocks, color=kind == "sdf_color")


def check_premises(p, blocks, n_elements, color=False):
    """What makes the device assertions meaningful: the block count is the one claimed; every block has a usable and a valid element (and
    a coloured one), so a block dropped or added twice moves the counts by at least 1; every block's share of the cost sum exceeds the bound
    granted to that sum, so it moves sum 27 by more than the bound.  Returns the smallest share / bound."""
    assert p["n_blocks"] == blocks, (p["n_blocks"], blocks)
    assert len(p["usable"]) == blocks and p["usable"].min() >= 1
    margin = np.inf
    for key, share in p["share"].items():
        valid = p["valid"][key] if isinstance(p["valid"], dict) else p["valid"]
        counts = p["counts"][key] if isinstance(p["counts"], dict) else p["counts"]
        assert len(valid) == blocks and valid.min() >= 1, (blocks, key, int(valid.min()))
        assert n_elements > counts[0] > counts[1], (blocks, key, counts)
        assert p["bound"][key] > 0 and share.min() > p["bound"][key], (blocks, key, float(share.min()), p["bound"][key])
        margin = min(margin, float(share.min()) / p["bound"][key])
    if color:
        assert p["colored"].min() >= 1 and 0 < p["counts"][2] < p["counts"][1], (blocks, p["counts"])
    return margin
