"""Direct SDF tracking on the device (icp_tsdf_sample, icp_tsdf_sdf_system, icp_tsdf_align_depth, icp_track_depth_sdf) against the numpy
restatement of the contract (tests/sdf_restatement.py): the field sample bit for bit, the sums of a step within what a summation order may
change, every step of an alignment from the device's own previous pose, the stop and the drain, the tracking loop against a composition
of public calls, the refusals, the untouched model loop, and the outcome on the 41-frame pan."""
import ctypes as C
import functools
import json
import numpy as np
import pytest

import support as S
import sdf_restatement as SR
import tsdf_restatement as TS
import tsdf_outcome_fixture as OF
import sdf_outcome_fixture as SF
from icp_amd.synth import camera_sequence, tum_K, wavy_depth
from support import bits, same_bits, pose_of

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = 1, 4, 8
W, H = 40, 30
SMALL = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=2.4)
ROOM_OPTS = dict(dims=(71, 35, 89), origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
NEAR = ((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))
FAR = ((0.05, 0.04, -0.03), (0.06, 0.05, -0.04))
AWAY = ((0, 3.0, 0), (0.0, 0.0, -1.0))                      # looks away from the model
RECORD_KEYS = ("n_depth", "n_valid_first", "n_valid_last", "iterations", "status")


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_record(a, b):
    return all(a[k] == b[k] for k in RECORD_KEYS) and u64(a["cost_first"]) == u64(b["cost_first"]) and u64(a["cost_last"]) == u64(b["cost_last"]) \
        and same_bits(a["pose"], b["pose"])


def crafted_frame():
    """40 x 30 holding every kind of depth the contract names: MINF, NaN, +inf, 0, a negative depth, a depth beyond max_depth (2.4), a hole."""
    d = wavy_depth(W, H)
    d[0, :6] = [MINF, np.nan, np.inf, 0.0, -1.0, 2.5]
    d[10:14, 20:24] = MINF
    return d


def small_model(ctx):
    """The 37 x 21 x 29 volume fused on the device from two wavy_depth frames, and the same volume in the restatement's hands."""
    from icp_amd import binding
    cam, rcam = binding.depth_camera(tum_K(W), W, H), TS.Camera(tum_K(W), W, H)
    ctx.tsdf_create(**SMALL)
    for _ in range(2):
        ctx.tsdf_integrate(wavy_depth(W, H), cam, np.eye(4, dtype=f32))
    vol = TS.Volume(**SMALL)
    vol.tsdf, vol.weight = ctx.tsdf_volume()
    return vol, cam, rcam


def test_sample_matches_restatement_bit_for_bit(gpu_ctx_factory):
    """Volume 37 x 21 x 29 with crafted values -- arbitrary fields beyond +-1, zero weights, NaNs with a payload in both arrays, infinities --
    on a dyadic grid (origin (-2, -1, -0.5), voxel 0.125), so that coordinates exactly on a voxel plane exist in fp32.  4099 points (no
    multiple of the 256-thread block): random ones in and around the volume, and on every axis a coordinate exactly on g = 0 and on
    g = n - 2 (valid), on g = n - 1 and just below 0 (invalid), far outside, NaN, +inf and -inf.  F, G and valid bit for bit."""
    opts = dict(dims=(37, 21, 29), origin=(-2.0, -1.0, -0.5), voxel_size=0.125, truncation=0.3)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create(**opts)
    vol = TS.Volume(**opts)
    rng = np.random.default_rng(11)
    shape = (29, 21, 37)
    t0 = rng.uniform(-1.5, 1.5, shape).astype(f32); w0 = rng.choice(np.array([1, 1.5, 7], f32), shape)
    w0[rng.random(shape) < 0.03] = 0
    t0.view(np.uint32)[rng.random(shape) < 0.01] = 0x7FC12345
    w0.view(np.uint32)[rng.random(shape) < 0.005] = 0xFFC54321
    t0[rng.random(shape) < 0.003] = np.inf; t0[rng.random(shape) < 0.003] = -np.inf
    t0[:, :, 0] = np.abs(t0[:, :, 0]); w0[:, :, 0] = 1; w0[:, :, 1] = 1; t0[:, :, 1] = 0.25      # the cells on g_x = 0 are valid and finite
    w0[:, :, 35:] = 1; t0[:, :, 35:] = -0.5                                                    # and those on g_x = n - 2
    ctx.tsdf_upload(t0, w0)
    vol.tsdf, vol.weight = t0.copy(), w0.copy()
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
    F, G, ok = ctx.tsdf_sample(pts)
    rF, rG, rok = SR.sample(vol, pts)
    print("sample: %d of %d points valid, %d of them with a NaN field, %d with |F| >= 1" % (rok.sum(), n, np.isnan(rF[rok > 0]).sum(), (np.abs(rF[rok > 0]) >= 1).sum()))
    assert np.array_equal(ok, rok.astype(bool))
    assert same_bits(F, rF) and same_bits(G, rG)
    # the planes: g = 0 and g = n - 2 valid, g = n - 1 invalid, on every axis
    for a in range(3):
        assert rok[9 * a] == 1 and rok[9 * a + 1] == 1 and rok[9 * a + 2] == 0, a
        assert not rok[9 * a + 3: 9 * a + 9].any(), a
    assert not rok[27]
    assert 1000 < rok.sum() < n - 500 and np.isnan(rF[rok > 0]).sum() > 10 and (rF[rok == 0] == 0).all() and (rG[rok == 0] == 0).all()
    # no output is mandatory, and no point is no work
    assert ctx.lib.icp_tsdf_sample(ctx.h, S.u32(pts).ctypes.data_as(C.c_void_p), C.c_int32(n), None, None, None) == 0
    assert ctx.lib.icp_tsdf_sample(ctx.h, None, C.c_int32(0), None, None, None) == 0


def check_system(ctx, vol, cam, rcam, depth, pose, what, **kw):
    sums, counts = ctx.tsdf_sdf_system(depth, cam, pose, **kw)
    rcounts, rsums, rabs = SR.system(vol, depth, rcam, pose, **kw)
    bound = rcounts[1] * 2.0 ** -52 * rabs
    err = np.abs(sums - rsums)
    print("system %s %s: n_depth %d, n_valid %d, worst |sum - restatement| / bound = %.3g" % (what, kw, counts[0], counts[1], (err / np.maximum(bound, 1e-300)).max()))
    assert tuple(counts) == tuple(rcounts), what
    assert (err <= bound).all(), (what, kw, err, bound)
    again, counts2 = ctx.tsdf_sdf_system(depth, cam, pose, **kw)
    assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts), what
    return counts


def test_system_matches_restatement(gpu_ctx_factory):
    """The sums of one step: counts exactly; every sum within n_valid 2^-52 sum |term| of the restatement's, the bound for any summation
    order of fp64 terms that are themselves identical; two calls give identical bits.  40 x 30 at strides 1 and 3 (3 does not divide 40:
    partial tiles, one block and several), huber 0 and 0.05, two poses; 70 x 50 at stride 1: 5 x 4 blocks, partial tiles on both axes.
    That is 6 and 20 blocks (1 at stride 3): k_sdf_solve's fold beyond 64, 256 and 512 blocks is tests/test_gpu_fold_sizes.py's."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    vol, cam, rcam = small_model(ctx)
    d = crafted_frame()
    for pose in (np.eye(4, dtype=f32), pose_of(*NEAR)):
        for stride in (1, 3):
            for huber in (0.0, 0.05):
                counts = check_system(ctx, vol, cam, rcam, d, pose, "40 x 30", stride=stride, huber=huber)
                if stride == 1:
                    assert 500 < counts[1] < counts[0] < W * H          # (CPU: 906 and 874 of 1178)
    cam70, rcam70 = binding.depth_camera(tum_K(70), 70, 50), TS.Camera(tum_K(70), 70, 50)
    counts = check_system(ctx, vol, cam70, rcam70, wavy_depth(70, 50), pose_of(*NEAR), "70 x 50", stride=1)
    assert counts[0] == 3500 - (wavy_depth(70, 50) > 2.4).sum() and counts[1] > 1000


def test_align_steps_follow_the_restatement(gpu_ctx_factory):
    """8 iterations with the stops off, traced.  Iteration i's pose within 1e-5 per element (the project's pose tolerance) of
    step(system(the DEVICE's pose i - 1)): feeding the device's own previous pose keeps a pixel that flips validity from compounding.
    n_valid exactly.  The final pose's rotation and translation distance to the identity below half the start's (CPU: 0.0072 rad /
    0.0132 m from 0.0269 / 0.0412; the minimum is not the identity at 10 cm voxels), and a second, farther start ends within 1e-3."""
    ctx = gpu_ctx_factory()
    vol, cam, rcam = small_model(ctx)
    d = crafted_frame()
    ends = []
    for start in (pose_of(*NEAR), pose_of(*FAR)):
        pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, start, trace=True, n_iterations=8, stop_rotation=0.0, stop_translation=0.0)
        assert rc == 0 and rec["status"] == 0 and rec["iterations"] == 8 and len(trace) == 8
        prev = start
        for i, t in enumerate(trace):
            counts, sums, _ = SR.system(vol, d, rcam, prev)
            want, _ = SR.step(sums, counts, prev)
            diff = float(np.abs(t["pose"] - want).max())
            print("align step %d: n_valid %d, cost %.6g, |pose - restatement| = %.3g" % (i, t["n_valid"], t["cost"], diff))
            assert t["status"] == 0 and t["n_valid"] == counts[1], i
            assert diff <= S.POSE_TOL, i
            assert abs(t["cost"] - sums[27]) <= counts[1] * 2.0 ** -52 * sums[27], i
            prev = t["pose"]
        assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose)
        assert (rec["n_depth"], rec["n_valid_first"], rec["n_valid_last"]) == (1178, trace[0]["n_valid"], trace[-1]["n_valid"])
        assert u64(rec["cost_first"]) == u64(trace[0]["cost"]) and u64(rec["cost_last"]) == u64(trace[-1]["cost"]) and rec["cost_last"] < rec["cost_first"]
        ends.append(pose)
    e0, e1 = OF.pose_error(pose_of(*NEAR), np.eye(4)), OF.pose_error(ends[0], np.eye(4))
    print("align: start %.4f rad / %.4f m, end %.4f rad / %.4f m; the two ends differ by %.3g" % (e0 + e1 + (np.abs(ends[0] - ends[1]).max(),)))
    assert e1[0] < 0.5 * e0[0] and e1[1] < 0.5 * e0[1]
    assert np.abs(ends[0] - ends[1]).max() < 1e-3


def test_stop_and_drain(gpu_ctx_factory):
    """With the stops at 1e-4 the frame ends early; its trace is bit for bit the head of the full run's, the returned pose is the stop
    iteration's, and the records past it stay zero: the launches behind the stop have drained.  A pose that looks away from the model, or a
    frame without a usable pixel, fails and leaves the pose as it was."""
    ctx = gpu_ctx_factory()
    vol, cam, rcam = small_model(ctx)
    d = crafted_frame()
    start = pose_of(*NEAR)
    full_pose, full_rec, rc, full = ctx.tsdf_align_depth(d, cam, start, trace=True, stop_rotation=0.0, stop_translation=0.0)
    assert rc == 0 and len(full) == 20 and full_rec["iterations"] == 20
    pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, start, trace=True, stop_rotation=1e-4, stop_translation=1e-4)
    n = rec["iterations"]
    print("stop: %d of 20 iterations (CPU: 4)" % n)
    assert rc == 0 and 1 <= n < 20 and len(trace) == n
    for a, b in zip(trace, full):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose)
    # the raw trace: nothing behind the stop was written
    from icp_amd import binding
    o = binding.sdf_options(stop_rotation=1e-4, stop_translation=1e-4)
    p = binding.pose_to_c(start); r = binding.IcpSdfFrame(); tr = (binding.IcpSdfIter * 20)()
    assert ctx.lib.icp_tsdf_align_depth(ctx.h, binding._ptr(d), C.byref(cam), C.byref(o), binding._ptr(p), C.byref(r), tr) == 0
    assert r.iterations == n and not any(bytes(tr[i]) != bytes(80) for i in range(n, 20)) and bytes(tr[n - 1]) != bytes(80)
    # the same without a trace
    pose2, rec2, rc2 = ctx.tsdf_align_depth(d, cam, start, stop_rotation=1e-4, stop_translation=1e-4)
    assert rc2 == 0 and same_record(rec2, rec) and same_bits(pose2, pose)
    # looking away: no valid pixel, the first step fails
    away = pose_of(*AWAY)
    pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, away, trace=True)
    assert rc == ERR_NO_CORRESPONDENCES and rec["status"] == rc and same_bits(pose, away) and same_bits(rec["pose"], away)
    assert rec["iterations"] == 1 and rec["n_depth"] == 1178 and rec["n_valid_first"] == 0 and len(trace) == 1 and trace[0]["status"] == rc
    assert "icp_tsdf_align_depth" in ctx.lib.icp_last_error(ctx.h).decode()
    # a frame without a usable pixel
    pose, rec, rc = ctx.tsdf_align_depth(np.full((H, W), MINF, f32), cam, start)
    assert rc == ERR_NO_SOURCE and rec["n_depth"] == 0 and same_bits(pose, start)


def test_rank_deficient_step_takes_the_eigen_solve(gpu_ctx_factory):
    """A volume whose field depends on z alone (a plane at z = 1 on a dyadic grid) leaves three of the six directions free: G_x = G_y = 0
    exactly, so three columns of J vanish, the LDL^T path meets a zero pivot and the step goes through the truncated eigen-solve and the
    single-thread composition.  One step from the identity on a constant depth of 1.05: the pose within 1e-5 of the restatement's, whose
    solution is the minimum-norm one; the residual -0.05 m is taken out along z (the plane through the moved points lies on z = 1 to 1e-4)."""
    from icp_amd import binding
    opts = dict(dims=(24, 24, 24), origin=(-1.0, -1.0, 0.0), voxel_size=0.125, truncation=0.25, min_depth=0.25, max_depth=2.5)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create(**opts)
    vol = TS.Volume(**opts)
    z = (np.arange(24, dtype=f32) * f32(0.125))[:, None, None]
    vol.tsdf = np.broadcast_to(np.clip((f32(1.0) - z) / f32(0.25), -1, 1), (24, 24, 24)).astype(f32).copy(); vol.weight = np.ones((24, 24, 24), f32)
    ctx.tsdf_upload(vol.tsdf, vol.weight)
    cam, rcam = binding.depth_camera(tum_K(W), W, H), TS.Camera(tum_K(W), W, H)
    d = np.full((H, W), 1.05, f32)
    eye = np.eye(4, dtype=f32)
    counts, sums, _ = SR.system(vol, d, rcam, eye)
    assert counts == (W * H, W * H) and sums[11] == 0 and sums[15] == 0 and sums[18] == 0 and sums[20] > 0          # the diagonal: (2,2), (3,3), (4,4) vanish
    want, x = SR.step(sums, counts, eye)
    pose, rec, rc, trace = ctx.tsdf_align_depth(d, cam, eye, trace=True, n_iterations=1)
    diff = float(np.abs(pose - want).max())
    print("rank-deficient step: x = %s, |pose - restatement| = %.3g, cost %.6g" % (np.array2string(x, precision=5), diff, rec["cost_first"]))
    assert rc == 0 and rec["iterations"] == 1 and rec["n_valid_first"] == W * H and trace[0]["status"] == 0
    assert diff <= S.POSE_TOL
    assert x[2] == 0 and x[3] == 0 and x[4] == 0 and abs(x[5] + 0.05) < 0.01
    sums_after, _ = ctx.tsdf_sdf_system(d, cam, pose)
    assert sums_after[27] < 1e-4 * sums[27]                    # the step took the whole residual out


def python_loop(ctx, depth, cam, rgbx, **kw):
    """icp_track_depth_sdf as a composition of public calls (the volume exists)."""
    pose = np.eye(4, dtype=f32)
    ctx.tsdf_integrate(depth[0], cam, pose, rgbx=None if rgbx is None else rgbx[0])
    recs = []
    for k in range(1, len(depth)):
        pose, rec, rc = ctx.tsdf_align_depth(depth[k], cam, pose, **kw)
        if rc == 0:
            ctx.tsdf_integrate(depth[k], cam, pose, rgbx=None if rgbx is None else rgbx[k])
        recs.append(rec)
    return pose, recs


@pytest.mark.parametrize("color", [False, True])
def test_track_depth_sdf_matches_composition_of_public_calls(gpu_ctx_factory, color):
    """5 frames of 40 x 30 of the synthetic room, frame 2 all MINF: records, poses and the volume (with its colour array) bit for bit."""
    from icp_amd import binding
    K, depth, _, gt = camera_sequence(5, W, H)
    depth[2][:] = MINF
    cam = binding.depth_camera(K, W, H)
    rgbx = np.random.default_rng(5).integers(0, 256, (5, W * H, 4), dtype=np.uint8) if color else None
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.tsdf_create(color=color, **ROOM_OPTS)
    kw = dict(stride=1, n_iterations=12)
    pose, recs, rc = a.track_depth_sdf(depth, cam, rgbx_frames=rgbx, **kw)
    ref_pose, ref = python_loop(b, depth, cam, rgbx, **kw)
    print("track_depth_sdf: statuses %s, iterations %s, n_valid %s" % ([r["status"] for r in recs], [r["iterations"] for r in recs], [r["n_valid_last"] for r in recs]))
    assert len(recs) == 4 and rc == ERR_NO_SOURCE
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert same_record(r, h), (k, r, h)
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    assert [r["status"] for r in recs] == [0, ERR_NO_SOURCE, 0, 0] and same_bits(recs[1]["pose"], recs[0]["pose"])
    ta, wa = a.tsdf_volume(); tb, wb = b.tsdf_volume()
    assert same_bits(ta, tb) and same_bits(wa, wb) and wa.max() == 4          # frames 0, 1, 3 and 4: the empty one was not fused
    if color:
        ca, cwa = a.tsdf_color_volume(); cb, cwb = b.tsdf_color_volume()
        assert same_bits(ca, cb) and same_bits(cwa, cwb) and cwa.max() == 4
    # the frames were tracked, not carried: every pose within the sequence's step of its ground truth
    for r, g in zip(recs, gt):
        if r["status"] == 0:
            e = OF.pose_error(r["pose"], g)
            assert e[0] < 0.05 and e[1] < 0.1, e


configure = functools.partial(S.configure, n_iterations=35, max_distance=0.1, seed=0)


def test_refusals_and_untouched_model_loop(gpu_ctx_factory):
    from icp_amd import binding
    K, depth, _, gt = camera_sequence(3, 80, 60)
    cam = binding.depth_camera(K, 80, 60)
    so = binding.depth_options(False, 2)
    eye = np.eye(4, dtype=f32)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    d = np.ascontiguousarray(depth, f32)
    p = binding.pose_to_c(eye); o = binding.sdf_options(); out = (binding.IcpSdfFrame * 2)(); rec = binding.IcpSdfFrame()
    sums = np.zeros(28); cnt = (C.c_int32 * 2)(); rgbx = np.zeros((3, 80 * 60, 4), np.uint8)
    msg = lambda: a.lib.icp_last_error(a.h).decode()
    sample = lambda: a.lib.icp_tsdf_sample(a.h, binding._ptr(d), C.c_int32(8), None, None, None)
    system = lambda cm=cam, op=o: a.lib.icp_tsdf_sdf_system(a.h, binding._ptr(d), C.byref(cm), binding._ptr(p), C.byref(op), binding._ptr(sums), cnt)
    align = lambda cm=cam, op=o: a.lib.icp_tsdf_align_depth(a.h, binding._ptr(d), C.byref(cm), C.byref(op), binding._ptr(p), C.byref(rec), None)
    track = lambda cm=cam, op=o, col=None: a.lib.icp_track_depth_sdf(a.h, binding._ptr(d), binding._ptr(col), C.c_int32(3), C.byref(cm), C.byref(op), binding._ptr(p), out)
    # no volume
    for call in (sample, system, align, track):
        assert call() == ERR_INVALID_ARG and "no volume" in msg()
    a.tsdf_create(**ROOM_OPTS)
    # non-identity depth extrinsics
    moved = binding.depth_camera(K, 80, 60, pose_of((0, 0, 0), (0.1, 0, 0)))
    for call in (system, align, track):
        assert call(moved) == ERR_INVALID_ARG and "extrinsics" in msg()
    # bad options, with a message
    for kw, word in ((dict(stride=0), "stride"), (dict(n_iterations=0), "n_iterations"), (dict(min_valid=3), "min_valid"), (dict(huber=-1.0), "huber"),
                     (dict(stop_rotation=float("nan")), "stop_rotation")):
        bad = binding.sdf_options(**kw)
        for call in (system, align, track):
            assert call(cam, bad) == ERR_INVALID_ARG and word in msg(), kw
    # colour frames without a colour array; null arguments
    assert track(cam, o, rgbx) == ERR_INVALID_ARG and "colour" in msg()
    assert a.lib.icp_tsdf_sample(a.h, None, C.c_int32(4), None, None, None) == ERR_INVALID_ARG
    assert a.lib.icp_tsdf_sample(a.h, binding._ptr(d), C.c_int32(-1), None, None, None) == ERR_INVALID_ARG
    assert a.lib.icp_tsdf_align_depth(a.h, None, C.byref(cam), C.byref(o), binding._ptr(p), C.byref(rec), None) == ERR_INVALID_ARG
    assert a.lib.icp_track_depth_sdf(a.h, binding._ptr(d), None, C.c_int32(0), C.byref(cam), C.byref(o), binding._ptr(p), out) == ERR_INVALID_ARG
    assert same_bits(binding.pose_from_c(p), eye)                              # no refusal touched the pose
    # SDF calls that run, then the model loop: against a context that never made one
    configure(a); configure(b)
    a.tsdf_sample(np.zeros((5, 3), f32)); a.tsdf_sdf_system(depth[0], cam, eye)
    _, _, rc = a.track_depth_sdf(depth, cam, n_iterations=5)
    assert rc == 0
    a.tsdf_align_depth(depth[1], cam, eye, n_iterations=3)
    a.tsdf_reset()
    b.tsdf_create(**ROOM_OPTS)
    (pa, ra, rca), (pb, rb, rcb) = [c.track_depth_model(depth, cam, so, gt=gt) for c in (a, b)]
    assert rca == rcb == 0 and same_bits(pa, pb)
    for x, y in zip(ra, rb):
        assert (x["n_src"], x["iterations"], x["status"]) == (y["n_src"], y["iterations"], y["status"]) and same_bits(x["pose"], y["pose"])
        assert bits(f32(x["initial_rmse"])) == bits(f32(y["initial_rmse"])) and bits(f32(x["final_rmse"])) == bits(f32(y["final_rmse"]))
    ta, wa = a.tsdf_volume(); tb, wb = b.tsdf_volume()
    assert same_bits(ta, tb) and same_bits(wa, wb)


def test_outcome_on_the_pan(gpu_ctx_factory):
    """The 41-frame, 60 degree pan of tests/tsdf_outcome_fixture.py through tum.track with the model and sdf=dict(stride=4, n_iterations=20).
    Figures (worst frame, rotation [rad] / translation [m]):
      restatement loop on the CPU (tests/golden/sdf_outcome.json): 0.0074 rad / 0.0391 m
      ray-cast model loop on the CPU (tests/golden/tsdf_outcome.json): 0.0187 rad / 0.0702 m
      device (MI355X): 0.0074 rad / 0.0391 m, the restatement's iteration count on every frame (printed below next to the bound)
    The bound is TWICE the restatement's worst frame, the margin DESIGN.md section 6m gives a 40-frame chain through the model that is not
    bit-reproducible between a CPU solve and the device's."""
    from icp_amd import tum
    with open(SF.GOLDEN) as f:
        ref = json.load(f)
    K, depth, gt = OF.fixture()
    seq = dict(depth=depth, rgbx=None, gt=gt, K=K, width=OF.W, height=OF.H)
    ctx = gpu_ctx_factory()
    poses, recs, rc = tum.track(ctx, seq, with_gt=False, model=OF.VOLUME, sdf=dict(SF.OPTIONS))
    rot, tr, last = OF.worst_errors([np.eye(4)] + [r["pose"] for r in recs], gt)
    print("restatement: worst %.4f rad / %.4f m; device SDF loop: worst %.4f rad / %.4f m (bound %.4f / %.4f), last %.4f rad / %.4f m, status %d, iterations %s"
          % (ref["worst_rotation_rad"], ref["worst_translation_m"], rot, tr, 2 * ref["worst_rotation_rad"], 2 * ref["worst_translation_m"], last[0], last[1], rc,
             [r["iterations"] for r in recs]))
    assert rc == 0 and all(r["status"] == 0 for r in recs) and len(recs) == OF.N_FRAMES - 1
    assert same_bits(np.linalg.inv(recs[-1]["pose"].astype(np.float64)).astype(f32), poses[-1])
    assert rot <= 2 * ref["worst_rotation_rad"] and tr <= 2 * ref["worst_translation_m"]
