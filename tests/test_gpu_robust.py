"""Trimmed ICP and the robust kernels (icp_set_robust_options) on the device against the numpy restatement tests/robust_restatement.py:
off is untouched, teacher-forced iterations on the context's own robust-off records, selection edge cases, free-running runs, the
partial-overlap fixture the feature exists for, the batch and tracking entry points, refusals and isolation."""
import ctypes as C
import gc
import numpy as np
import pytest

import gicp_restatement as G
import robust_restatement as R
from conftest import pose_error
from support import check_stats, configure, load, u32

pytestmark = pytest.mark.gpu
f32 = np.float32
EPS = 1e-3
KERNELS = ("none", "huber", "cauchy", "tukey")


@pytest.fixture(scope="module")
def depth_pair():
    from icp_amd import synth
    return synth.compact_rgbd_pair()


def teacher_forced(ctx, d, pose, metric, opts, label, tol=1e-9):
    """icp_correspond with robust mode off, then with each option set of `opts` on, at `pose`: records and stats bit-identical to the
    restatement applied to the robust-off records, sums within `tol` of its fp64 sums (relative to the absolute sums)."""
    ctx.set_robust_options()
    base, _, _ = ctx.correspond(pose)
    assert ctx.robust_stats() == []
    p = ctx.transform_points(d["src_pts"], pose)
    ns_t = ctx.transform_normals(d["src_nrm"], pose) if metric == 2 else None
    if metric == 3:
        tg, b = ctx.gicp_normals("target"), ctx.transform_normals(ctx.gicp_normals("source"), pose)
    for o in opts:
        ctx.set_robust_options(**o)
        recs, sums, nv = ctx.correspond(pose)
        st = ctx.robust_stats()
        ref = R.robust(base, p, d["tgt_pts"], dict(o, kernel=KERNELS.index(o.get("kernel", "none"))), metric)
        lab = "%s %s" % (label, o)
        assert len(st) == 1
        check_stats(st[0], ref["stats"], lab)
        assert np.array_equal(recs["idx"], ref["recs"]["idx"]), lab
        assert np.array_equal(u32(recs["weight"]), u32(ref["recs"]["weight"])), lab
        if ref["m"] == 0:
            continue
        means = (f32(sums[1:4] / sums[0]), f32(sums[4:7] / sums[0])) if metric == 2 and sums[0] > 0 else None
        gi = None
        if metric == 3:
            j = np.maximum(recs["idx"], 0)
            gi = dict(a=tg[j], b=b, eps=EPS)
        s_ref, sa = R.sums(metric, p, d["tgt_pts"], recs, tgt_nrm=d["tgt_nrm"], src_nrm_t=ns_t, means=means, gicp=gi)
        assert nv == int(s_ref[0]) and sums[0] == s_ref[0], (lab, nv, s_ref[0])
        if metric != 3:
            assert nv == ref["M"], lab                       # every kept pair passed the validity filter already
        err = np.abs(sums[1:34] - s_ref[1:34]) / (sa[1:34] + 1e-300)
        assert err.max() <= tol, (lab, int(np.argmax(err)) + 1)
    ctx.set_robust_options()


def option_grid(sigma_fixed):
    out = []
    for k in KERNELS:
        for ov in (1.0, 0.7, 0.3):
            for sg in (0.0, sigma_fixed):
                if k == "none" and (ov == 1.0 or sg > 0):
                    continue
                out.append(dict(kernel=k, overlap=ov, sigma=sg))
    return out


@pytest.mark.parametrize("metric", [0, 1, 2, 3])
@pytest.mark.parametrize("weighting", [0, 1, 2, 3])
@pytest.mark.parametrize("rejection", [0, 1])
def test_teacher_forced(gpu_ctx_factory, bunny, depth_pair, metric, weighting, rejection):
    from icp_amd import synth
    ctx = gpu_ctx_factory()
    configure(ctx, metric=metric, weighting=weighting, rejection=rejection)
    ctx.set_gicp_options(EPS, 10)
    load(ctx, bunny)
    pose = synth.make_pose((0.01, -0.015, 0.02), (0.002, -0.003, 0.001)).astype(f32)
    teacher_forced(ctx, bunny, pose, metric, option_grid(0.002), "bunny")
    configure(ctx, metric=metric, weighting=weighting, rejection=rejection, max_distance=0.01)
    load(ctx, depth_pair)
    teacher_forced(ctx, depth_pair, np.eye(4, dtype=f32), metric, option_grid(0.005), "depth/8")


@pytest.mark.parametrize("knn_backend,color_icp", [(0, 0), (0, 1), (1, 1)])
def test_teacher_forced_matchers(gpu_ctx_factory, depth_pair, knn_backend, color_icp):
    ctx = gpu_ctx_factory()
    opts = [dict(kernel="huber", overlap=0.7), dict(kernel="tukey", overlap=0.3, sigma=0.005), dict(kernel="cauchy")]
    for metric in (0, 1, 2):
        configure(ctx, metric=metric, knn_backend=knn_backend, color_icp=color_icp, weighting=3 if color_icp else 0, max_distance=0.01)
        load(ctx, depth_pair)
        teacher_forced(ctx, depth_pair, np.eye(4, dtype=f32), metric, opts, "depth/8 backend %d colour %d" % (knn_backend, color_icp))


def test_teacher_forced_projective(gpu_ctx_factory, depth_pair):
    o = depth_pair["organised"]; K = depth_pair["K"]
    d = dict(src_pts=o["src_pts"], src_nrm=o["src_nrm"], tgt_pts=o["tgt_pts"], tgt_nrm=o["tgt_nrm"])
    ctx = gpu_ctx_factory()
    opts = [dict(kernel="huber", overlap=0.7), dict(kernel="tukey", overlap=0.3), dict(kernel="none", overlap=0.5), dict(kernel="cauchy", sigma=0.01)]
    for metric in (0, 1, 2):
        configure(ctx, metric=metric, matching=1, max_distance=0.1)
        p = ctx.params
        p.fx, p.fy, p.cx, p.cy, p.width, p.height = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), 80, 60
        ctx.push_params()
        load(ctx, d, colors=False)
        teacher_forced(ctx, d, np.eye(4, dtype=f32), metric, opts, "projective")


def test_teacher_forced_fullsize(gpu_ctx_factory):
    from icp_amd import synth
    d = synth.eth_like_pair(0)
    assert len(d["src_pts"]) == 370488
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, max_distance=10.0)
    load(ctx, d, colors=False)
    teacher_forced(ctx, d, np.eye(4, dtype=f32), 1, [dict(kernel="huber", overlap=0.6), dict(kernel="tukey", overlap=0.9, sigma=0.05)], "370k",
                   tol=1e-8)


def raw_correspond(ctx, tgt, src, opts):
    """Target / source as given (no normals needed: constant weights, no rejection, point-to-point), robust-off records, then each option set."""
    ctx.set_target(tgt, np.zeros_like(tgt)); ctx.set_source(src, np.zeros_like(src))
    eye = np.eye(4, dtype=f32)
    ctx.set_robust_options()
    base, _, _ = ctx.correspond(eye)
    p = ctx.transform_points(src, eye)
    for o in opts:
        ctx.set_robust_options(**o)
        recs, sums, nv = ctx.correspond(eye)
        ref = R.robust(base, p, tgt, dict(o, kernel=KERNELS.index(o.get("kernel", "none"))), 0)
        check_stats(ctx.robust_stats()[0], ref["stats"], str(o))
        assert np.array_equal(recs["idx"], ref["recs"]["idx"]) and np.array_equal(u32(recs["weight"]), u32(ref["recs"]["weight"])), o
        yield o, ref, nv
    ctx.set_robust_options()


def test_selection_edge_cases(gpu_ctx_factory):
    """r^2 with ties across the threshold, all-equal values, values that differ only in the last digit pass, values at the top of the
    float range (huge finite coordinates), m = 1 and m = 2, and a multi-block n: stats and records bit-identical to the restatement."""
    ctx = gpu_ctx_factory()
    configure(ctx, metric=0, weighting=0, rejection=0, knn_backend=0, max_distance=3e38)
    opts = [dict(kernel="huber", overlap=ov) for ov in (1.0, 0.7, 0.5, 0.3, 0.01)] + [dict(kernel="tukey", overlap=0.5), dict(kernel="none", overlap=0.25)]
    rng = np.random.default_rng(5)
    # ties: residuals from a handful of distinct offsets along x (one target point at the origin, far from the others)
    n = 3000
    off = rng.choice(np.array([0.1, 0.2, 0.3, 0.4], f32), n)
    src = np.zeros((n, 3), f32); src[:, 0] = off; tgt = np.zeros((1, 3), f32)
    for o, ref, nv in raw_correspond(ctx, tgt, src, opts):
        assert ref["M"] >= ref["K"] and nv == ref["M"]
    # all equal
    src = np.full((500, 3), 0.25, f32)
    for o, ref, nv in raw_correspond(ctx, tgt, src, opts):
        assert ref["M"] == 500
    # keys that differ only in their lowest bits (the last 10-bit digit): consecutive floats x near 0.5
    x = (np.uint32(np.float32(0.5).view(np.uint32)) + rng.permutation(np.arange(700, dtype=np.uint32))).view(f32)
    src = np.zeros((700, 3), f32); src[:, 0] = x
    for o, ref, nv in raw_correspond(ctx, tgt, src, opts):
        assert len(np.unique(ref["keys"] >> 10)) <= 3
    # the top of the key range: r^2 near FLT_MAX.  (+inf keys cannot come out of a matcher -- a candidate needs d^2 < FLT_MAX -- so the
    # restatement's handling of them is checked on the host, tests/test_robust_host.py.)
    src = rng.normal(0, 1, (400, 3)).astype(f32); src[:50, 0] = f32(1.3e19) * (1 + rng.random(50).astype(f32) * f32(0.001))
    for o, ref, nv in raw_correspond(ctx, tgt, src, [dict(kernel="huber", overlap=0.8), dict(kernel="cauchy", overlap=0.5, sigma=1.0),
                                                     dict(kernel="tukey", overlap=0.95), dict(kernel="huber", overlap=1.0)]):
        k = ref["keys"]
        assert ((k >= np.uint32(0x7E000000)) & (k < np.uint32(0x7F800000))).sum() == 50 and ref["m"] == 400
    # m = 1, m = 2 (K = 1)
    for m in (1, 2):
        src = np.arange(m * 3, dtype=f32).reshape(m, 3) + 1
        for o, ref, nv in raw_correspond(ctx, tgt, src, opts):
            assert ref["m"] == m and ref["K"] >= 1
    # multi-block n with random residuals (several blocks of every select pass)
    src = rng.normal(0, 1, (300000, 3)).astype(f32)
    for o, ref, nv in raw_correspond(ctx, tgt, src, [dict(kernel="huber", overlap=0.6), dict(kernel="cauchy", overlap=0.3), dict(kernel="tukey")]):
        assert ref["m"] == 300000


def test_off_is_untouched(gpu_ctx_factory, bunny):
    import support as M
    eye = np.eye(4, dtype=f32)
    a = gpu_ctx_factory(); configure(a, metric=1, n_iterations=10); load(a, bunny)
    pa, ra, _ = a.run(eye)
    b = gpu_ctx_factory(); configure(b, metric=1, n_iterations=10); load(b, bunny)
    b.set_robust_options()
    m0 = M.counters(b)[0]
    pb, rb, _ = b.run(eye)
    assert M.counters(b)[0] == m0 + 1                      # the merged loop was taken
    b.set_robust_options("huber", overlap=0.5)
    b.run(eye)
    assert M.counters(b)[0] == m0 + 1                      # robust mode does not take it
    b.set_robust_options("none", 0.0, 0.0, 1.0)
    pc, rc_, _ = b.run(eye)
    assert M.counters(b)[0] == m0 + 2 and b.robust_stats() == []
    for p_, r_ in ((pb, rb), (pc, rc_)):
        assert np.array_equal(u32(pa), u32(p_))
        assert all(np.array_equal(u32(x["pose"]), u32(y["pose"])) and x["n_valid"] == y["n_valid"] for x, y in zip(ra, r_))


@pytest.mark.parametrize("multires,selection", [(1, 0), (0, 1), (1, 1)])
def test_free_running(gpu_ctx_factory, bunny, multires, selection):
    """icp_run with multires / random sampling: every iteration's stats are consistent (K, M, n_valid), the iterations at full
    resolution without resampling equal the restatement on the robust-off records at the incoming pose, and a second run is bit-identical.
    The iterations on levels and samples are compared with the restatement (stats, n_valid and pose) in tests/test_gpu_query_sets.py."""
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, n_iterations=6, multires=multires, selection=selection, proba=0.5)
    load(ctx, bunny)
    o = dict(kernel="huber", overlap=0.7)
    ctx.set_robust_options(**o)
    eye = np.eye(4, dtype=f32)
    pose, recs, rc = ctx.run(eye)
    st = ctx.robust_stats()
    assert rc == 0 and len(st) == len(recs) > 0
    for r, s in zip(recs, st):
        K = int(min(max(np.ceil(np.float64(f32(0.7)) * s["n_entering"]), 1), s["n_entering"]))
        assert s["n_kept"] >= K and r["n_valid"] == s["n_kept"] and s["trim_d2"] >= 0 and s["sigma"] > 0
    prev = eye
    for i, r in enumerate(recs):
        if r["n_src"] == len(bunny["src_pts"]) and selection == 0:
            ctx.set_robust_options()
            base, _, _ = ctx.correspond(prev)
            p = ctx.transform_points(bunny["src_pts"], prev)
            ref = R.robust(base, p, bunny["tgt_pts"], dict(o, kernel=1), 1)
            check_stats(st[i], ref["stats"], "iteration %d" % i)
            ctx.set_robust_options(**o)
        prev = r["pose"]
    pose2, recs2, _ = ctx.run(eye)
    assert np.array_equal(u32(pose), u32(pose2)) and ctx.robust_stats() == st


def partial_overlap_fixture():
    """ETH-like pair at 86 x 270 (23 220 source points); the target loses every point beyond the 60 % quantile of the unperturbed
    source's x, so 40 % of the source has no counterpart."""
    from icp_amd import synth
    return synth.partial_overlap_pair(0, 86, 270, 0.6, drop_target_normals=False)


def test_partial_overlap():
    """The reason for the feature.  Point-to-plane, max distance 10 (the reference's ETH value), 20 iterations from the perturbed pose.
    The restatement (tests/robust_restatement.py step, nearest neighbour in fp64) gave: plain ICP 0.575 rad / 1.066 m off the ground
    truth, trimmed (overlap 0.6) + Huber 6.3e-4 rad / 2.1e-3 m.  The device (exact k-NN) gave plain 0.344 rad / 0.945 m, trimmed + Huber
    6.4e-4 rad / 1.05e-3 m."""
    from icp_amd import binding
    d = partial_overlap_fixture()
    errs = {}
    for label, o in (("plain", None), ("trimmed", dict(kernel="huber", overlap=0.6))):
        ctx = binding.Context(0)
        try:
            configure(ctx, metric=1, n_iterations=20, max_distance=10.0)
            load(ctx, d, colors=False)
            if o:
                ctx.set_robust_options(**o)
            pose, recs, rc = ctx.run(np.eye(4, dtype=f32))
            errs[label] = pose_error(pose, d["gt"])
        finally:
            ctx.close()
    (ap, tp_), (at, tt) = errs["plain"], errs["trimmed"]
    print("partial overlap: plain %.3g rad / %.3g m, trimmed + Huber %.3g rad / %.3g m" % (ap, tp_, at, tt))
    assert at <= 1e-3 and tt <= 1e-2, errs
    assert ap >= 5 * at and tp_ >= 5 * tt, errs


def test_batch_and_tracking_equal_per_pair_runs(gpu_ctx_factory):
    from icp_amd import binding, eth, synth
    scans = [tuple(np.ascontiguousarray(a, f32) for a in synth.laser_scan(synth.scan_pose(k), 40 + k, n_tilt=43, n_beam=135)[:2]) for k in range(3)]
    pairs = [dict(src_pts=scans[k + 1][0], src_nrm=scans[k + 1][1], tgt_pts=scans[k][0], tgt_nrm=scans[k][1]) for k in range(2)]
    pairs.append(dict(src_pts=scans[0][0], src_nrm=scans[0][1], tgt_pts=scans[2][0], tgt_nrm=scans[2][1]))
    o = dict(kernel="cauchy", overlap=0.8)
    ctxs = [gpu_ctx_factory(), gpu_ctx_factory()]
    for c in ctxs:
        configure(c, n_iterations=12, max_distance=0.05)
        c.set_robust_options(**o)
    poses, status, rc = binding.batch_run(ctxs, pairs)
    ref = gpu_ctx_factory()
    configure(ref, n_iterations=12, max_distance=0.05)
    ref.set_robust_options(**o)
    per_pair = []
    for i, d in enumerate(pairs):
        pose, recs, st = eth.align(ref, d, check=False)
        assert st == status[i]
        assert np.array_equal(u32(binding.pose_to_c(pose)), u32(poses[i])), i
        per_pair.append(ref.robust_stats())
    for c in ctxs:                                            # each context keeps the records of its own last pair
        assert len(c.robust_stats()) == 12 and c.robust_stats() in per_pair
    # tracking
    W, H = 80, 60
    K = np.array([[525.0 / 8, 0, 319.5 / 8], [0, 525.0 / 8, 239.5 / 8], [0, 0, 1]], f32)
    depth = np.stack([synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), W, H, 0x7A11 + k)[0][:, 2].reshape(H, W).copy() for k in range(3)])
    cam = binding.depth_camera(K, W, H)
    to, so = binding.depth_options(False, 1), binding.depth_options(False, 2)
    a = gpu_ctx_factory(); configure(a, n_iterations=15, max_distance=0.01); a.set_robust_options("tukey", overlap=0.7)
    _, trecs, _ = a.track_depth_frames(depth, None, cam, to, so)
    b = gpu_ctx_factory(); configure(b, n_iterations=15, max_distance=0.01); b.set_robust_options("tukey", overlap=0.7)
    b.set_target_depth(depth[0], None, cam, to)
    pose = np.eye(4, dtype=f32)
    for k in range(1, 3):
        b.set_source_depth(depth[k], None, cam, so)
        pose, _, st = b.run(pose, check=False)
        assert trecs[k - 1]["status"] == st
        assert np.array_equal(u32(trecs[k - 1]["pose"]), u32(pose)), k
    assert a.robust_stats() == b.robust_stats() and len(a.robust_stats()) == 15


def test_refusals_and_isolation(gpu_ctx_factory, bunny):
    from icp_amd import binding
    lib = binding.load_library()

    def live():
        v = C.c_int64(0)
        assert lib.icp_debug_live_bytes(C.byref(v)) == 0
        return v.value
    ctx = gpu_ctx_factory()
    for bad in (dict(kernel=4), dict(kernel=-1), dict(tuning=-1.0), dict(tuning=float("inf")), dict(sigma=float("nan")), dict(sigma=-0.5),
                dict(overlap=0.0), dict(overlap=1.5), dict(overlap=float("nan"))):
        with pytest.raises(binding.IcpError) as ei:
            ctx.set_robust_options(**bad)
        assert ei.value.code == 1 and "icp_set_robust_options" in str(ei.value)
    configure(ctx, metric=1, n_iterations=8)
    load(ctx, bunny)
    eye = np.eye(4, dtype=f32)
    ctx.set_robust_options("huber", overlap=0.8)
    ctx.set_optimizer(True)
    assert ctx.run(eye, check=False)[2] == 1 and "robust" in lib.icp_last_error(ctx.h).decode()
    ctx.set_optimizer(None)
    for call in (lambda: ctx.run_multistart([eye]), lambda: ctx.match_seeded([eye])):
        with pytest.raises(binding.IcpError) as ei:
            call()
        assert ei.value.code == 1
    p1, r1, _ = ctx.run(eye)
    s1 = ctx.robust_stats()
    # another context, robust off, runs in between: neither disturbs the other
    other = gpu_ctx_factory(); configure(other, metric=1, n_iterations=8); load(other, bunny)
    q1, _, _ = other.run(eye)
    p2, r2, _ = ctx.run(eye)
    q2, _, _ = other.run(eye)
    assert np.array_equal(u32(p1), u32(p2)) and ctx.robust_stats() == s1 and np.array_equal(u32(q1), u32(q2))
    fresh = gpu_ctx_factory(); configure(fresh, metric=1, n_iterations=8); load(fresh, bunny)
    assert np.array_equal(u32(fresh.run(eye)[0]), u32(q1))
    # device bytes back to the baseline after destroy
    gc.collect()
    before = live()
    c = binding.Context(0)
    configure(c, metric=2, n_iterations=4); load(c, bunny)
    c.set_robust_options("tukey", overlap=0.5)
    c.run(eye); c.correspond(eye)
    assert live() > before
    c.close()
    assert live() == before
