"""Direct SDF tracking with the photometric term on the device (icp_tsdf_sample_color, icp_tsdf_sdf_system_color,
icp_tsdf_align_depth_color, icp_track_depth_sdf_color) against the numpy restatement of the contract (tests/sdf_color_restatement.py):
the intensity sample bit for bit, the 29 sums within what a summation order may change, every step of an alignment from the device's own
previous pose, the stop and the drain, the rank the colour restores, the tracking loop against a composition of public calls, the
refusals, the untouched neighbours, and the outcome on the textured wall."""
import ctypes as C
import functools
import json
import numpy as np
import pytest

import support as S
import sdf_color_restatement as SC
import sdf_restatement as SR
import tsdf_color_restatement as TC
import tsdf_restatement as TS
import tsdf_color_outcome_fixture as CF
import sdf_color_outcome_fixture as CO
from icp_amd.synth import camera_sequence, tum_K, wavy_depth
from support import bits, same_bits, pose_of

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = 1, 4, 8
W, H = 40, 30
SMALL = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=2.4)
ROOM_OPTS = dict(dims=(71, 35, 89), origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
NEAR = ((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))
AWAY = ((0, 3.0, 0), (0.0, 0.0, -1.0))                      # looks away from the model
INT_KEYS = ("n_depth", "n_valid_first", "n_valid_last", "n_color_first", "n_color_last", "iterations", "status")
F64_KEYS = ("cost_first", "cost_last", "cost_color_first", "cost_color_last")


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_record(a, b):
    return set(a) == set(b) and all(a[k] == b[k] for k in INT_KEYS) and all(u64(a[k]) == u64(b[k]) for k in F64_KEYS) and same_bits(a["pose"], b["pose"])


def same_iter(a, b):
    return (a["n_valid"], a["n_color"], a["status"]) == (b["n_valid"], b["n_color"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) \
        and u64(a["cost_color"]) == u64(b["cost_color"]) and same_bits(a["pose"], b["pose"])


def small_model(ctx):
    """The 37 x 21 x 29 volume fused on the device from two wavy_depth frames, with SC.smooth_colors as its colour array, and the same
    volume in the restatement's hands."""
    from icp_amd import binding
    cam, rcam = binding.depth_camera(tum_K(W), W, H), TS.Camera(tum_K(W), W, H)
    ctx.tsdf_create(color=True, **SMALL)
    for _ in range(2):
        ctx.tsdf_integrate(wavy_depth(W, H), cam, np.eye(4, dtype=f32))
    vol = TS.Volume(**SMALL)
    vol.tsdf, vol.weight = ctx.tsdf_volume()
    SC.smooth_colors(vol)
    ctx.tsdf_color_upload(vol.rgb, vol.wc)
    return vol, cam, rcam


def rendered_colors(vol, depth, rcam, pose, shift=(0.0, 0.0, 0.0)):
    """The colour frame a camera at `pose` sees of the volume's intensity field (every channel S / 3, rounded to a byte), the field read
    `shift` metres away from the pixel's own point: the frame whose photometric residual vanishes once the points have moved by `shift`."""
    h, w = depth.shape
    t = SR.pixel_terms(vol, depth, rcam, pose)
    Sv, _, ok = SC.sample_color(vol, t["q"] + np.asarray(shift, f32))
    byte = np.clip(np.floor(np.where(ok > 0, Sv, 0).astype(f64) / 3.0 + 0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([byte, byte, byte, np.full(w * h, 255, np.uint8)], 1))


def scaled_wavy(w, h):
    """wavy_depth(40, 30)'s surface seen through w x h pixels of the same field of view (tum_K scales with the width)."""
    u, v = np.meshgrid((np.arange(w, dtype=np.float64) + 0.5) * W / w - 0.5, (np.arange(h, dtype=np.float64) + 0.5) * H / h - 0.5)
    return (1.5 + 0.3 * np.sin(u * 0.3) + 0.2 * np.cos(v * 0.4) + 0.5 * (u > 0.7 * W)).astype(f32)


def crafted_frame(w=W, h=H):
    """Every kind of depth the contract names: MINF, NaN, +inf, 0, a negative depth, a depth beyond max_depth (2.4), a hole."""
    d = wavy_depth(w, h) if (w, h) == (W, H) else scaled_wavy(w, h)
    d[0, :6] = [MINF, np.nan, np.inf, 0.0, -1.0, 2.5]
    d[h // 3:h // 3 + 3, w // 2:w // 2 + 3] = MINF
    return d


def test_sample_color_matches_restatement_bit_for_bit(gpu_ctx_factory):
    """The crafted 37 x 21 x 29 volume of the geometric sample test on its dyadic grid (origin (-2, -1, -0.5), voxel 0.125) and its 4099
    points -- random ones in and around the volume, on every axis a coordinate exactly on g = 0 and g = n - 2 (valid), on g = n - 1 and just
    below 0 (invalid), far outside, NaN, +inf, -inf.  The colour array: channels beyond 0 .. 255, NaNs with a payload, +-inf, colour weights
    with a payload NaN, and a few hundred voxels with Wc = 0, so that cells with exactly one uncoloured corner occur.  The geometry is left
    cleared (weight 0 everywhere): it plays no part.  S, H and valid bit for bit."""
    opts = dict(dims=(37, 21, 29), origin=(-2.0, -1.0, -0.5), voxel_size=0.125, truncation=0.3)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create(color=True, **opts)
    vol = TC.add_color(TS.Volume(**opts))
    rng = np.random.default_rng(11)
    shape = (29, 21, 37)
    rgb = rng.uniform(-20, 280, shape + (3,)).astype(f32)
    wc = rng.choice(np.array([1, 2.5, 7], f32), shape)
    zero = rng.random(shape) < 0.015
    wc[zero] = 0
    rgb.view(np.uint32)[rng.random(shape + (3,)) < 0.004] = 0x7FC12345
    wc.view(np.uint32)[rng.random(shape) < 0.003] = 0xFFC54321
    rgb[rng.random(shape + (3,)) < 0.001] = np.inf; rgb[rng.random(shape + (3,)) < 0.001] = -np.inf
    rgb[:, :, :2] = np.abs(rgb[:, :, :2]); wc[:, :, :2] = 1                       # the cells on g_x = 0 are valid and finite
    rgb[:, :, 35:] = 100.0; wc[:, :, 35:] = 1                                     # and those on g_x = n - 2
    ctx.tsdf_color_upload(rgb, wc)
    vol.rgb, vol.wc = rgb.copy(), wc.copy()
    n = 4099
    lo = np.array([-2.3, -1.3, -0.8], f32); hi = np.array([2.8, 1.8, 3.3], f32)
    pts = (lo + rng.random((n, 3)).astype(f32) * (hi - lo)).astype(f32)
    inside = np.array([0.3, 0.2, 1.1], f32)
    dims, org, s = (37, 21, 29), np.array(opts["origin"], f32), f32(0.125)
    k = 0
    for a in range(3):
        for g in (0, dims[a] - 2, dims[a] - 1):
            pts[k] = inside; pts[k, a] = org[a] + f32(g) * s
            assert (pts[k, a] - org[a]) / s == f32(g)       # exactly on the plane
            k += 1
        for bad in (np.nextafter(org[a], f32(-10)), f32(1e6), f32(-1e6), np.nan, np.inf, -np.inf):
            pts[k] = inside; pts[k, a] = bad; k += 1
    pts[k] = [np.nan, np.nan, np.nan]; k += 1
    Sd, Hd, ok = ctx.tsdf_sample_color(pts)
    rS, rH, rok = SC.sample_color(vol, pts)
    # cells with exactly one uncoloured corner
    g = np.floor((pts - org) / s); inb = np.isfinite(g).all(1) & (g >= 0).all(1) & (g <= np.array(dims, f32) - 2).all(1)
    i = np.where(inb[:, None], g, 0).astype(int)
    unc = sum((wc[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx] == 0).astype(int) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    one = int((inb & (unc == 1)).sum())
    print("sample_color: %d of %d points valid, %d of them with a NaN field, %d cells with exactly one uncoloured corner, %d voxels with Wc = 0"
          % (rok.sum(), n, np.isnan(rS[rok > 0]).sum(), one, (wc == 0).sum()))
    assert np.array_equal(ok, rok.astype(bool))
    assert same_bits(Sd, rS) and same_bits(Hd, rH)
    for a in range(3):
        assert rok[9 * a + 2] == 0 and not rok[9 * a + 3: 9 * a + 9].any(), a     # g = n - 1 and everything outside: invalid
    assert rok[0] == 1 and rok[1] == 1 and not rok[27]                            # g_x = 0 and g_x = n - 2 were made valid
    assert 200 < (wc == 0).sum() < 600 and one > 50 and 500 < rok.sum() < n - 500 and np.isnan(rS[rok > 0]).sum() > 5
    assert np.isinf(rS[rok > 0]).any() or np.isinf(rH[rok > 0]).any()
    assert (rS[rok == 0] == 0).all() and (rH[rok == 0] == 0).all()
    # no output is mandatory, and no point is no work
    assert ctx.lib.icp_tsdf_sample_color(ctx.h, S.u32(pts).ctypes.data_as(C.c_void_p), C.c_int32(n), None, None, None) == 0
    assert ctx.lib.icp_tsdf_sample_color(ctx.h, None, C.c_int32(0), None, None, None) == 0


SHARES = []


def check_system(ctx, vol, cam, rcam, depth, rgbx, pose, what, stride=1, huber=0.0, color_weight=0.1, color_huber=0.0):
    sums, counts = ctx.tsdf_sdf_system(depth, cam, pose, rgbx=rgbx, stride=stride, huber=huber, color_weight=color_weight, color_huber=color_huber)
    rcounts, rsums, rabs = SC.system(vol, depth, rgbx, rcam, pose, stride=stride, huber=huber, weight=color_weight, color_huber=color_huber)
    bound = (rcounts[1] + rcounts[2]) * 2.0 ** -52 * rabs
    err = np.abs(sums - rsums)
    share = float((err / np.maximum(bound, 1e-300)).max())
    SHARES.append(share)
    print("system %s stride %d huber %g colour huber %g: n_depth %d, n_valid %d, n_color %d, worst |sum - restatement| / bound = %.3g"
          % (what, stride, huber, color_huber, counts[0], counts[1], counts[2], share))
    assert sums.shape == (29,) and tuple(counts) == tuple(rcounts), what
    assert (err <= bound).all(), (what, err, bound)
    again, counts2 = ctx.tsdf_sdf_system(depth, cam, pose, rgbx=rgbx, stride=stride, huber=huber, color_weight=color_weight, color_huber=color_huber)
    assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts), what
    return counts, sums


def test_system_matches_restatement(gpu_ctx_factory):
    """The 29 sums of one joint step: the three counts exactly; every sum within (n_valid + n_color) 2^-52 sum(|geometric term| +
    |photometric term|) of the restatement's, the bound for any summation order of fp64 terms that are themselves identical; two calls give
    identical bits.  13 x 11: one block with a partial tile; 75 x 58: 5 x 4 blocks with partial tiles on both axes; strides 1 and 3; the
    geometric Huber and the colour Huber on and off; then a band of the frame valid but uncoloured (0 < n_color < n_valid), and a corner
    colour that is NaN (the pixel keeps its geometric row: n_valid as before, n_color lower, every sum finite).
    That is 1 and 20 blocks: k_sdf_solve_color's fold and its row guard beyond 64, 256 and 512 blocks are tests/test_gpu_fold_sizes.py's."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    vol, _, _ = small_model(ctx)
    pose = pose_of(*NEAR)
    frames = {}
    for w, h in ((13, 11), (75, 58)):
        cam, rcam = binding.depth_camera(tum_K(w), w, h), TS.Camera(tum_K(w), w, h)
        d = crafted_frame(w, h)
        rgbx = rendered_colors(vol, np.where(np.isfinite(d), d, f32(1.5)).astype(f32), rcam, np.eye(4, dtype=f32))
        rgbx[::7, :3] = np.random.default_rng(w).integers(0, 256, (len(rgbx[::7]), 3), dtype=np.uint8)      # outliers for the colour Huber
        frames[(w, h)] = (cam, rcam, d, rgbx)
        for stride in (1, 3):
            for huber in (0.0, 0.05):
                for color_huber in (0.0, 0.1):
                    counts, sums = check_system(ctx, vol, cam, rcam, d, rgbx, pose, "%d x %d" % (w, h), stride, huber, color_huber=color_huber)
                    if stride == 1:
                        assert 0.5 * w * h < counts[2] == counts[1] < counts[0] < w * h and 0 < sums[28] < sums[27]
    cam, rcam, d, rgbx = frames[(75, 58)]
    assert (ctx.tsdf_sdf_system(d, cam, pose, rgbx=rgbx, color_weight=0.1, color_huber=0.1)[0][28]
            < ctx.tsdf_sdf_system(d, cam, pose, rgbx=rgbx, color_weight=0.1)[0][28])          # the colour Huber bites
    full, _ = check_system(ctx, vol, cam, rcam, d, rgbx, pose, "75 x 58 full", color_weight=0.3)
    # a band valid but uncoloured
    band = vol.wc.copy(); band[:, :, 20:] = 0
    vol.wc = band; ctx.tsdf_color_upload(vol.rgb, vol.wc)
    counts, _ = check_system(ctx, vol, cam, rcam, d, rgbx, pose, "75 x 58 band", color_weight=0.3)
    assert counts[:2] == full[:2] and 0 < counts[2] < counts[1]
    # a NaN corner colour
    vol.wc = np.ones_like(band)
    t = SC.pixel_terms(vol, d, rgbx, rcam, pose)
    q = t["q"][np.nonzero(t["colored"])[0][1500]].astype(f64)
    i = np.floor((q - vol.o.astype(f64)) / f64(vol.s)).astype(int)
    vol.rgb[i[2], i[1], i[0], 2] = np.nan
    ctx.tsdf_color_upload(vol.rgb, vol.wc)
    counts, sums = check_system(ctx, vol, cam, rcam, d, rgbx, pose, "75 x 58 NaN corner", color_weight=0.3)
    assert counts[:2] == full[:2] and 0 < full[2] - counts[2] < 64 and np.isfinite(sums).all()
    print("system: worst share of the bound over %d cases = %.3g" % (len(SHARES), max(SHARES)))


def test_align_steps_follow_the_restatement(gpu_ctx_factory):
    """8 iterations with the stops off, traced, on a frame whose colours are the volume's own seen from the identity.  Iteration i's pose
    within 1e-5 per element (the project's pose tolerance, the geometric test's bound for the same reason) of step(system(the DEVICE's pose
    i - 1)); n_valid and n_color exactly; the two costs within the summation bound's relative size.  Then the stop with its trace bit-equal
    to the full run's head and zeros behind it, a frame with too few valid pixels and a frame with no usable pixel, pose carried."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    vol, cam, rcam = small_model(ctx)
    d = crafted_frame()
    n_usable = int((np.isfinite(d) & (d > 0) & (d <= f32(2.4))).sum())          # 1200 - 6 - the 3 x 3 hole
    assert n_usable == 1185
    rgbx = rendered_colors(vol, wavy_depth(W, H), rcam, np.eye(4, dtype=f32))
    start = pose_of(*NEAR)
    kw = dict(rgbx=rgbx, color_weight=0.3)
    pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, start, trace=True, n_iterations=8, stop_rotation=0.0, stop_translation=0.0, **kw)
    assert rc == 0 and rec["status"] == 0 and rec["iterations"] == 8 and len(trace) == 8
    prev = start
    for i, t in enumerate(trace):
        counts, sums, _ = SC.system(vol, d, rgbx, rcam, prev, weight=0.3)
        want, _ = SR.step(sums, counts, prev)
        diff = float(np.abs(t["pose"] - want).max())
        print("align step %d: n_valid %d, n_color %d, cost %.6g (colour %.6g), |pose - restatement| = %.3g" % (i, t["n_valid"], t["n_color"], t["cost"], t["cost_color"], diff))
        assert t["status"] == 0 and (t["n_valid"], t["n_color"]) == counts[1:] and t["pad"] == 0, i
        assert diff <= S.POSE_TOL, i
        n2 = (counts[1] + counts[2]) * 2.0 ** -52
        assert abs(t["cost"] - sums[27]) <= n2 * sums[27] and abs(t["cost_color"] - sums[28]) <= n2 * sums[28], i
        prev = t["pose"]
    assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose)
    assert (rec["n_depth"], rec["n_valid_first"], rec["n_valid_last"], rec["n_color_first"], rec["n_color_last"]) == \
        (n_usable, trace[0]["n_valid"], trace[-1]["n_valid"], trace[0]["n_color"], trace[-1]["n_color"])
    assert u64(rec["cost_first"]) == u64(trace[0]["cost"]) and u64(rec["cost_last"]) == u64(trace[-1]["cost"])
    assert u64(rec["cost_color_first"]) == u64(trace[0]["cost_color"]) and u64(rec["cost_color_last"]) == u64(trace[-1]["cost_color"])
    assert rec["cost_last"] < rec["cost_first"] and rec["cost_color_last"] < rec["cost_color_first"]
    # the stop: the head of the full run, zeros behind it
    full_pose, full_rec, rc, full = ctx.tsdf_align_depth(d, cam, start, trace=True, stop_rotation=0.0, stop_translation=0.0, **kw)
    assert rc == 0 and len(full) == 20 and full_rec["iterations"] == 20
    pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, start, trace=True, stop_rotation=1e-4, stop_translation=1e-4, **kw)
    n = rec["iterations"]
    print("stop: %d of 20 iterations" % n)
    assert rc == 0 and 1 <= n < 20 and len(trace) == n
    for a, b in zip(trace, full):
        assert same_iter(a, b)
    assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose)
    o = binding.sdf_options(stop_rotation=1e-4, stop_translation=1e-4); co = binding.sdf_color_options(weight=0.3)
    p = binding.pose_to_c(start); r = binding.IcpSdfColorFrame(); tr = (binding.IcpSdfColorIter * 20)()
    dd = np.ascontiguousarray(d, f32)
    assert ctx.lib.icp_tsdf_align_depth_color(ctx.h, binding._ptr(dd), binding._ptr(rgbx), C.byref(cam), C.byref(o), C.byref(co), binding._ptr(p), C.byref(r), tr) == 0
    assert r.iterations == n and not any(bytes(tr[i]) != bytes(96) for i in range(n, 20)) and bytes(tr[n - 1]) != bytes(96)
    pose2, rec2, rc2 = ctx.tsdf_align_depth(d, cam, start, stop_rotation=1e-4, stop_translation=1e-4, **kw)
    assert rc2 == 0 and same_record(rec2, rec) and same_bits(pose2, pose)
    # too few valid pixels: the first step fails, the pose is carried
    away = pose_of(*AWAY)
    pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, away, trace=True, **kw)
    assert rc == ERR_NO_CORRESPONDENCES and rec["status"] == rc and same_bits(pose, away) and same_bits(rec["pose"], away)
    assert rec["iterations"] == 1 and rec["n_depth"] == n_usable and rec["n_valid_first"] == 0 and rec["n_color_first"] == 0 and len(trace) == 1 and trace[0]["status"] == rc
    assert "icp_tsdf_align_depth_color" in ctx.lib.icp_last_error(ctx.h).decode()
    # no usable pixel
    pose, rec, rc = ctx.tsdf_align_depth(np.full((H, W), MINF, f32), cam, start, **kw)
    assert rc == ERR_NO_SOURCE and rec["status"] == rc and rec["n_depth"] == 0 and same_bits(pose, start)


def test_colour_restores_the_rank(gpu_ctx_factory):
    """The geometric test's rank-deficient volume -- a field that depends on z alone, a plane at z = 1 on a dyadic grid -- with a colour
    field that varies in x and y.  The frame: a constant depth of 1.05 whose colours are the volume's, read 2 cm / -1 cm aside.  The
    geometric call finds three directions free and takes the truncated eigen-solve (x_3 = x_4 = 0 exactly: no lateral motion); the joint
    system is full rank -- the device's own guard, (6 eps_f32)^2 trace(H) trace(H^-1) < 1, evaluated on the restatement's sums --, so the
    step takes the LDL^T path, matches the restatement's full solve within 1e-5 and moves laterally, along the shift."""
    from icp_amd import binding
    opts = dict(dims=(24, 24, 24), origin=(-1.0, -1.0, 0.0), voxel_size=0.125, truncation=0.25, min_depth=0.25, max_depth=2.5)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create(color=True, **opts)
    vol = TC.add_color(TS.Volume(**opts))
    z = (np.arange(24, dtype=f32) * f32(0.125))[:, None, None]
    vol.tsdf = np.broadcast_to(np.clip((f32(1.0) - z) / f32(0.25), -1, 1), (24, 24, 24)).astype(f32).copy(); vol.weight = np.ones((24, 24, 24), f32)
    x = (-1.0 + np.arange(24) * 0.125)[None, None, :]; y = (-1.0 + np.arange(24) * 0.125)[None, :, None]
    vol.rgb = np.stack([128 + 60 * np.sin(2 * np.pi * x / 1.1) + 0 * y + 0 * z, 120 + 50 * np.sin(2 * np.pi * y / 0.9) + 0 * x + 0 * z,
                        100 + 30 * np.cos(2 * np.pi * (x + y) / 1.3) + 0 * z], -1).astype(f32)
    vol.wc = np.ones((24, 24, 24), f32)
    ctx.tsdf_upload(vol.tsdf, vol.weight); ctx.tsdf_color_upload(vol.rgb, vol.wc)
    cam, rcam = binding.depth_camera(tum_K(W), W, H), TS.Camera(tum_K(W), W, H)
    d = np.full((H, W), 1.05, f32)
    eye = np.eye(4, dtype=f32)
    shift = (0.02, -0.01, 0.0)
    rgbx = rendered_colors(vol, d, rcam, eye, shift)
    # the geometric call on this volume: rank 3, the eigen-solve, no lateral motion
    gcounts, gsums, _ = SR.system(vol, d, rcam, eye)
    assert gsums[11] == 0 and gsums[15] == 0 and gsums[18] == 0
    gpose, grec, grc, gtrace = ctx.tsdf_align_depth(d, cam, eye, trace=True, n_iterations=1)
    gwant, gx = SR.step(gsums, gcounts, eye)
    assert grc == 0 and float(np.abs(gpose - gwant).max()) <= S.POSE_TOL and gx[3] == 0 and gx[4] == 0 and gpose[0, 3] == 0 and gpose[1, 3] == 0
    # the joint system: full rank by the device's own guard
    counts, sums, _ = SC.system(vol, d, rgbx, rcam, eye, weight=0.5)
    Hm = np.zeros((6, 6)); k = 0
    for i in range(6):
        for j in range(i, 6):
            Hm[i, j] = Hm[j, i] = sums[k]; k += 1
    guard = (6 * 2.0 ** -23) ** 2 * np.trace(Hm) * np.trace(np.linalg.inv(Hm))
    assert counts == (W * H, W * H, W * H) and np.linalg.eigvalsh(Hm).min() > 0 and guard < 1e-3
    want, xr = SR.step(sums, counts, eye, min_valid=64)
    pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, eye, trace=True, n_iterations=1, rgbx=rgbx, color_weight=0.5)
    diff = float(np.abs(pose - want).max())
    print("rank: guard %.3g; x = %s, |pose - restatement| = %.3g; geometric x = %s" % (guard, np.array2string(xr, precision=5), diff, np.array2string(gx, precision=5)))
    assert rc == 0 and rec["n_color_first"] == W * H and trace[0]["status"] == 0 and diff <= S.POSE_TOL
    # lateral motion, along the shift: more than half of it in one Gauss-Newton step on a smooth field
    assert 0.5 * shift[0] < pose[0, 3] < 1.5 * shift[0] and 1.5 * shift[1] < pose[1, 3] < 0.5 * shift[1] and abs(pose[2, 3] + 0.05) < 0.01


def python_loop(ctx, depth, cam, rgbx, **kw):
    """icp_track_depth_sdf_color as a composition of public calls (the volume exists)."""
    pose = np.eye(4, dtype=f32)
    ctx.tsdf_integrate(depth[0], cam, pose, rgbx=rgbx[0])
    recs = []
    for k in range(1, len(depth)):
        pose, rec, rc = ctx.tsdf_align_depth(depth[k], cam, pose, rgbx=rgbx[k], **kw)
        if rc == 0:
            ctx.tsdf_integrate(depth[k], cam, pose, rgbx=rgbx[k])
        recs.append(rec)
    return pose, recs


def test_track_depth_sdf_color_matches_composition_of_public_calls(gpu_ctx_factory):
    """5 frames of 40 x 30 of the synthetic room with their colour frames, frame 2 all MINF: records, poses and all four volume arrays bit
    for bit."""
    from icp_amd import binding
    K, depth, rgbx, gt = camera_sequence(5, W, H)
    depth[2][:] = MINF
    cam = binding.depth_camera(K, W, H)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.tsdf_create(color=True, **ROOM_OPTS)
    kw = dict(stride=1, n_iterations=12, color_weight=0.1, color_huber=0.2)
    pose, recs, rc = a.track_depth_sdf(depth, cam, rgbx_frames=rgbx, **kw)
    ref_pose, ref = python_loop(b, depth, cam, rgbx, **kw)
    print("track_depth_sdf_color: statuses %s, iterations %s, n_valid %s, n_color %s" % ([r["status"] for r in recs], [r["iterations"] for r in recs],
                                                                                         [r["n_valid_last"] for r in recs], [r["n_color_last"] for r in recs]))
    assert len(recs) == 4 and rc == ERR_NO_SOURCE
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert same_record(r, h), (k, r, h)
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    assert [r["status"] for r in recs] == [0, ERR_NO_SOURCE, 0, 0] and same_bits(recs[1]["pose"], recs[0]["pose"])
    assert all(r["n_color_last"] > 100 for r in recs if r["status"] == 0)
    ta, wa = a.tsdf_volume(); tb, wb = b.tsdf_volume()
    assert same_bits(ta, tb) and same_bits(wa, wb) and wa.max() == 4          # frames 0, 1, 3 and 4: the empty one was not fused
    ca, cwa = a.tsdf_color_volume(); cb, cwb = b.tsdf_color_volume()
    assert same_bits(ca, cb) and same_bits(cwa, cwb) and cwa.max() == 4


configure = functools.partial(S.configure, n_iterations=35, max_distance=0.1, seed=0)


def test_refusals_and_untouched_neighbours(gpu_ctx_factory):
    from icp_amd import binding
    K, depth, rgbx, gt = camera_sequence(3, 80, 60)
    cam = binding.depth_camera(K, 80, 60)
    eye = np.eye(4, dtype=f32)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    d = np.ascontiguousarray(depth, f32); cols = np.ascontiguousarray(rgbx, np.uint8)
    p = binding.pose_to_c(eye); o = binding.sdf_options(); co = binding.sdf_color_options()
    out = (binding.IcpSdfColorFrame * 2)(); rec = binding.IcpSdfColorFrame()
    sums = np.zeros(29); cnt = (C.c_int32 * 3)()
    P = binding._ptr
    msg = lambda: a.lib.icp_last_error(a.h).decode()
    sample = lambda: a.lib.icp_tsdf_sample_color(a.h, P(d), C.c_int32(8), None, None, None)
    system = lambda cm=cam, op=o, cp=co, cl=cols: a.lib.icp_tsdf_sdf_system_color(a.h, P(d), P(cl), C.byref(cm), P(p), C.byref(op), C.byref(cp), P(sums), cnt)
    align = lambda cm=cam, op=o, cp=co, cl=cols: a.lib.icp_tsdf_align_depth_color(a.h, P(d), P(cl), C.byref(cm), C.byref(op), C.byref(cp), P(p), C.byref(rec), None)
    track = lambda cm=cam, op=o, cp=co, cl=cols: a.lib.icp_track_depth_sdf_color(a.h, P(d), P(cl), C.c_int32(3), C.byref(cm), C.byref(op), C.byref(cp), P(p), out)
    # no volume; a volume without the colour array
    for call in (sample, system, align, track):
        assert call() == ERR_INVALID_ARG and "no volume" in msg()
    a.tsdf_create(**ROOM_OPTS)
    for call in (sample, system, align, track):
        assert call() == ERR_INVALID_ARG and "colour array" in msg()
    a.tsdf_color_create()
    # a null colour frame; non-identity depth extrinsics; bad options of either kind
    for call in (system, align, track):
        assert call(cl=None) == ERR_INVALID_ARG and "rgbx" in msg()
    moved = binding.depth_camera(K, 80, 60, pose_of((0, 0, 0), (0.1, 0, 0)))
    for call in (system, align, track):
        assert call(moved) == ERR_INVALID_ARG and "extrinsics" in msg()
    for kw, word in ((dict(stride=0), "stride"), (dict(n_iterations=0), "n_iterations"), (dict(huber=-1.0), "huber")):
        for call in (system, align, track):
            assert call(cam, binding.sdf_options(**kw)) == ERR_INVALID_ARG and word in msg(), kw
    for kw, word in ((dict(weight=0.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(huber=-0.5), "colour huber")):
        for call in (system, align, track):
            assert call(cam, o, binding.sdf_color_options(**kw)) == ERR_INVALID_ARG and word in msg(), kw
    assert a.lib.icp_tsdf_sample_color(a.h, None, C.c_int32(4), None, None, None) == ERR_INVALID_ARG
    assert a.lib.icp_track_depth_sdf_color(a.h, P(d), P(cols), C.c_int32(0), C.byref(cam), C.byref(o), C.byref(co), P(p), out) == ERR_INVALID_ARG
    assert same_bits(binding.pose_from_c(p), eye)                              # no refusal touched the pose
    with pytest.raises(ValueError):
        a.tsdf_align_depth(depth[1], cam, eye, color_weight=0.1)              # a colour weight without the colour frame
    with pytest.raises(ValueError):
        a.track_depth_sdf(depth, cam, color_weight=0.1)
    # colour-SDF calls that run; then the neighbours, against a context that never made one
    configure(a); configure(b)
    a.tsdf_sample_color(np.zeros((5, 3), f32))
    _, _, rc = a.track_depth_sdf(depth, cam, rgbx_frames=rgbx, n_iterations=5, color_weight=0.1)
    assert rc == 0
    a.tsdf_sdf_system(depth[0], cam, eye, rgbx=rgbx[0], color_weight=0.1)
    a.tsdf_align_depth(depth[1], cam, eye, rgbx=rgbx[1], n_iterations=3, color_weight=0.1)
    b.tsdf_create(color=True, **ROOM_OPTS)
    # icp_track_depth_sdf, with and without painting
    for cl in (None, rgbx):
        a.tsdf_reset(); b.tsdf_reset()
        (pa, ra, rca), (pb, rb, rcb) = [c.track_depth_sdf(depth, cam, rgbx_frames=cl, n_iterations=6) for c in (a, b)]
        assert rca == rcb == 0 and same_bits(pa, pb) and set(ra[0]) == set(rb[0]) and "n_color_last" not in ra[0]
        for x, y in zip(ra, rb):
            assert all(x[k] == y[k] for k in ("n_depth", "n_valid_first", "n_valid_last", "iterations", "status")) and same_bits(x["pose"], y["pose"])
            assert u64(x["cost_first"]) == u64(y["cost_first"]) and u64(x["cost_last"]) == u64(y["cost_last"])
    # icp_track_depth_model_color
    so = binding.depth_options(False, 2, fix_color_index=True)
    a.tsdf_reset(); b.tsdf_reset()
    (pa, ra, rca), (pb, rb, rcb) = [c.track_depth_model(depth, cam, so, gt=gt, rgbx_frames=rgbx) for c in (a, b)]
    assert rca == rcb == 0 and same_bits(pa, pb)
    for x, y in zip(ra, rb):
        assert (x["n_src"], x["iterations"], x["status"]) == (y["n_src"], y["iterations"], y["status"]) and same_bits(x["pose"], y["pose"])
        assert bits(f32(x["initial_rmse"])) == bits(f32(y["initial_rmse"])) and bits(f32(x["final_rmse"])) == bits(f32(y["final_rmse"]))
    for ga, gb in zip(a.tsdf_volume() + a.tsdf_color_volume(), b.tsdf_volume() + b.tsdf_color_volume()):
        assert same_bits(ga, gb)
    # color_weight = 0 through Python is today's call: against the library called directly
    a.tsdf_reset(); b.tsdf_reset()
    for c in (a, b):
        c.tsdf_integrate(depth[0], cam, eye, rgbx=rgbx[0])
    s_py, c_py = a.tsdf_sdf_system(depth[1], cam, eye, rgbx=rgbx[1], color_weight=0.0, stride=2)
    s28 = np.zeros(28); c2 = (C.c_int32 * 2)(); o2 = binding.sdf_options(stride=2)
    assert b.lib.icp_tsdf_sdf_system(b.h, P(d[1]), C.byref(cam), P(binding.pose_to_c(eye)), C.byref(o2), P(s28), c2) == 0
    assert s_py.shape == (28,) and np.array_equal(u64(s_py), u64(s28)) and tuple(c_py) == (c2[0], c2[1])
    pose_py, rec_py, rc_py = a.tsdf_align_depth(depth[1], cam, eye, rgbx=rgbx[1], color_weight=0.0, stride=2)
    r2 = binding.IcpSdfFrame(); p2 = binding.pose_to_c(eye)
    assert b.lib.icp_tsdf_align_depth(b.h, P(d[1]), C.byref(cam), C.byref(o2), P(p2), C.byref(r2), None) == rc_py == 0
    assert same_bits(pose_py, binding.pose_from_c(p2)) and rec_py["iterations"] == r2.iterations and u64(rec_py["cost_last"]) == u64(r2.cost_last) and "n_color_last" not in rec_py
    a.tsdf_reset(); b.tsdf_reset()
    pose_py, recs_py, rc_py = a.track_depth_sdf(depth, cam, rgbx_frames=rgbx, color_weight=0.0, stride=2)
    out2 = (binding.IcpSdfFrame * 2)(); p2 = binding.pose_to_c(eye)
    assert b.lib.icp_track_depth_sdf(b.h, P(d), P(cols), C.c_int32(3), C.byref(cam), C.byref(o2), P(p2), out2) == rc_py == 0
    assert same_bits(pose_py, binding.pose_from_c(p2))
    for x, y in zip(recs_py, out2):
        assert x["iterations"] == y.iterations and u64(x["cost_last"]) == u64(y.cost_last) and same_bits(x["pose"], binding.pose_from_c(y.pose))
    for ga, gb in zip(a.tsdf_volume() + a.tsdf_color_volume(), b.tsdf_volume() + b.tsdf_color_volume()):
        assert same_bits(ga, gb)


def test_outcome_on_the_textured_wall(gpu_ctx_factory):
    """The textured wall of tests/tsdf_color_outcome_fixture.py (12 frames of 160 x 120, 1 cm of lateral travel per frame, 0.11 m in all)
    through tum.track with a coloured model and sdf=dict(stride=2, n_iterations=20, color_weight=0.1), and the same frames through the
    geometric direct tracker.  Figures (translation error [m]):
      restatement, coloured (tests/golden/sdf_color_outcome.json): worst 0.0018, last 0.0007, 3 - 5 iterations per frame
      restatement, geometric: worst 0.0930, last 0.0883, all 20 iterations on 10 of 11 frames
      device (MI355X): coloured worst 0.0018, last 0.0007, the restatement's iteration count on every frame; geometric worst 0.0930, last 0.0883
    Asked of the device: status 0 on every frame; the worst error within TWICE the restatement's and every frame's iteration count within
    twice the restatement's (the margin DESIGN.md section 6m gives a chain of frames through a model that is not bit-reproducible between a
    CPU solve and the device's); the geometric device loop ends more than half the travel away."""
    from icp_amd import tum
    with open(CO.GOLDEN) as f:
        ref = json.load(f)
    K, depth, rgbx, gt = CF.fixture()
    seq = dict(depth=depth, rgbx=rgbx, gt=gt, K=K, width=CF.W, height=CF.H)
    ctx = gpu_ctx_factory()
    poses, recs, rc = tum.track(ctx, seq, with_gt=False, model=dict(color=True, **CF.VOLUME), sdf=dict(color_weight=CO.COLOR_OPTIONS["weight"], **CO.OPTIONS))
    err = CF.translation_errors([np.eye(4)] + [r["pose"] for r in recs], gt)
    its = [r["iterations"] for r in recs]
    print("restatement: worst %.4f m, iterations %s; device coloured SDF loop: worst %.4f m (bound %.4f), last %.4f m, status %d, iterations %s, n_color %s"
          % (ref["colored_worst_translation_m"], ref["colored_iterations"], max(err), 2 * ref["colored_worst_translation_m"], err[-1], rc, its,
             [r["n_color_last"] for r in recs]))
    assert rc == 0 and all(r["status"] == 0 for r in recs) and len(recs) == CF.N_FRAMES - 1
    assert same_bits(np.linalg.inv(recs[-1]["pose"].astype(np.float64)).astype(f32), poses[-1])
    assert max(err) <= 2 * ref["colored_worst_translation_m"]
    assert all(i <= 2 * j for i, j in zip(its, ref["colored_iterations"]))
    travel = ref["lateral_travel_m"]
    gposes, grecs, grc = tum.track(ctx, seq, with_gt=False, model=dict(color=True, **CF.VOLUME), sdf=dict(CO.OPTIONS))
    gerr = CF.translation_errors([np.eye(4)] + [r["pose"] for r in grecs], gt)
    print("device geometric SDF loop: worst %.4f m, last %.4f m (restatement %.4f / %.4f), iterations %s" % (max(gerr), gerr[-1], ref["geometric_worst_translation_m"],
                                                                                                            ref["geometric_last_translation_m"], [r["iterations"] for r in grecs]))
    assert grc == 0 and gerr[-1] > travel / 2 and 2 * max(err) < travel / 2
