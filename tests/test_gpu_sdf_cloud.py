"""A laser scan aligned to the TSDF volume on the device (icp_tsdf_cloud_system, icp_tsdf_align_cloud, icp_track_scans_sdf; DESIGN.md section
6zf) against the numpy restatement of the contract (tests/sdf_cloud_restatement.py).  The counts are compared exactly; every sum with the
contract's bound, n_valid 2^-52 sum |term| with sum |term| from the restatement; two runs bit for bit; every traced iteration's pose within
support.POSE_TOL of the restatement's step from the DEVICE's previous pose, as tests/test_gpu_fold_sizes.py does.  Sizes around a wave, a
work-group's pass, one block's and two blocks' points, both storages, the target as well as the source; the sizes at which k_sdf_solve's
fold changes shape; clouds without a valid or a finite point; min_valid met and missed by one; cells across blocks 0 / -1 and in the last
layer of a dense box; the stop's drain; the loop with a scan that fails in the middle; evict and insert; the refusals; and the outcome on
the twelve scans of tests/tsdf_cloud_outcome_fixture.py."""
import ctypes

import numpy as np
import pytest

import htsdf_restatement as HR
import sdf_cloud_cases as K
import sdf_cloud_outcome_fixture as OF
import sdf_cloud_restatement as SC
import sdf_restatement as SR
import support as S
import tsdf_cloud_outcome_fixture as CF
import tsdf_cloud_restatement as CR
from support import same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = 0, 1, 3, 4, 8
STEPS = 3
STORAGES = ("dense", "hashed")


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def upload(ctx, vol):
    """A restatement's volume, dense or hashed, into the context."""
    opts = dict(origin=tuple(float(x) for x in vol.o), voxel_size=float(vol.s), truncation=float(vol.trunc), max_weight=float(vol.max_w), max_depth=float(vol.max_d))
    if isinstance(vol, HR.HVolume):
        ctx.tsdf_create_hashed(block_capacity=max(64, len(vol.blocks)), **opts)
        ctx.tsdf_upload_blocks(*vol.sorted_blocks())
    else:
        ctx.tsdf_create(dims=vol.dims, **opts)
        ctx.tsdf_upload(vol.tsdf, vol.weight)
    return ctx


def state(ctx, hashed):
    return ctx.tsdf_blocks() if hashed else ctx.tsdf_volume()


def same_state(a, b, hashed):
    if hashed:
        return a[0]["n_blocks"] == b[0]["n_blocks"] and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])
    return same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def resident(ctx, which, pts):
    (ctx.set_source if which == "source" else ctx.set_target)(pts)


@pytest.fixture(scope="module")
def ctxs(gpu_ctx_factory):
    """One context per storage holding sdf_cloud_cases.model(): the dense box, and the same voxels in blocks."""
    return {"dense": upload(gpu_ctx_factory(), K.model(False)), "hashed": upload(gpu_ctx_factory(), K.model(True))}


def check_system(what, ctx, vol, pts, pose, which="source", huber=0.0, ref=None):
    """Counts exactly; every sum within n_valid 2^-52 sum |term| of the restatement's; a second call the same bits."""
    rcounts, rsums, rabs = ref if ref is not None else SC.system(vol, pts, pose, huber=huber)
    sums, counts = ctx.tsdf_cloud_system(which, pose, huber=huber)
    sums2, counts2 = ctx.tsdf_cloud_system(which, pose, huber=huber)
    bound = rcounts[1] * 2.0 ** -52 * rabs
    err = np.abs(sums - rsums)
    print("%s: counts %s, worst |sum - restatement| / bound = %.3g" % (what, tuple(counts), (err / np.maximum(bound, 1e-300)).max()))
    assert tuple(counts) == tuple(rcounts), (what, counts, rcounts)
    assert (err <= bound).all(), (what, err, bound)
    assert np.array_equal(u64(sums), u64(sums2)) and tuple(counts2) == tuple(counts), what
    return sums, counts


def follow(what, vol, pts, start, rec, rc, trace, **opt):
    """Every iteration's pose within S.POSE_TOL of the restatement's step from the DEVICE's previous pose, n_valid exactly, the cost within
    the summation bound; a step the restatement fails is failed on the device, with the pose carried."""
    o = SC.options(**opt)
    prev = np.asarray(start, f32)
    first = None
    assert len(trace) == rec["iterations"] >= 1
    for i, t in enumerate(trace):
        counts, sums, sabs = SC.system(vol, pts, prev, **o)
        first = counts if first is None else first
        want, x = (None, None) if counts[0] == 0 else SR.step(sums, counts, prev, **o)
        bound = counts[1] * 2.0 ** -52 * sabs[27]
        assert t["n_valid"] == counts[1] and abs(t["cost"] - sums[27]) <= bound, (what, i, t["n_valid"], counts)
        if want is None:
            status = ERR_NO_SOURCE if counts[0] == 0 else ERR_NO_CORRESPONDENCES
            assert t["status"] == status == rec["status"] == rc and i == len(trace) - 1, (what, i, t["status"])
            assert same_bits(t["pose"], prev) and same_bits(rec["pose"], np.asarray(start, f32)), (what, i)
            break
        diff = float(np.abs(t["pose"] - want).max())
        print("%s, step %d: n_valid %d of %d, cost %.6g, |pose - restatement| = %.3g" % (what, i, counts[1], counts[0], t["cost"], diff))
        assert t["status"] == OK and diff <= S.POSE_TOL, (what, i, diff)
        prev = t["pose"]
        if i == len(trace) - 1:
            assert rc == OK and rec["status"] == OK and same_bits(rec["pose"], t["pose"])
            assert SR.stopped(x, **o) or i == o["n_iterations"] - 1, (what, i)
    assert (rec["n_depth"], rec["n_valid_first"], rec["n_valid_last"]) == (first[0], trace[0]["n_valid"], trace[-1]["n_valid"])
    assert u64(rec["cost_first"]) == u64(trace[0]["cost"]) and u64(rec["cost_last"]) == u64(trace[-1]["cost"])


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("storage", STORAGES)
def test_sizes(ctxs, storage, n):
    """The sums and three traced steps at every size, the cloud as the source and as the target (whose planes are padded to a wave)."""
    ctx, vol = ctxs[storage], K.model(storage == "hashed")
    pts = K.cloud(n, seed=100 + n)
    ref = SC.system(vol, pts, K.START)
    for which in ("source", "target"):
        resident(ctx, which, pts)
        what = "%s, %d points as the %s" % (storage, n, which)
        check_system(what, ctx, vol, pts, K.START, which, ref=ref)
        opt = dict(n_iterations=STEPS, min_valid=6, stop_rotation=0.0, stop_translation=0.0)
        pose, rec, rc, trace = ctx.tsdf_align_cloud(which, K.START, trace=True, **opt)
        follow(what, vol, pts, K.START, rec, rc, trace, **opt)
        assert same_bits(pose, rec["pose"])
    if n >= 255:
        assert ref[0][1] >= 64 and rec["iterations"] == STEPS and rc == OK


@pytest.mark.parametrize("blocks", K.FOLD_BLOCKS)
@pytest.mark.parametrize("storage", STORAGES)
def test_fold_sizes(ctxs, storage, blocks):
    """The accumulate over 1, 64, 65, 256, 257 and 513 blocks: the sizes at which k_sdf_solve's four-in-flight fold changes shape.  The
    dense and the hashed model hold the same field (tests/test_sdf_cloud_host.py), so one reference serves both."""
    ctx = ctxs[storage]
    pts = K.fold_cloud()[:blocks * K.PER_BLOCK]
    ctx.set_source(pts)
    ref = K.fold_reference(blocks)
    assert ref[0][0] == len(pts) and ref[0][1] > 0.5 * len(pts)
    check_system("%s, %d blocks" % (storage, blocks), ctx, None, pts, K.START, ref=ref)
    if blocks in (257, 513):
        opt = dict(n_iterations=STEPS, stop_rotation=0.0, stop_translation=0.0)
        pose, rec, rc, trace = ctx.tsdf_align_cloud("source", K.START, trace=True, **opt)
        follow("%s, %d blocks" % (storage, blocks), K.model(), pts, K.START, rec, rc, trace, **opt)


@pytest.mark.parametrize("storage", STORAGES)
def test_huber_orders_and_special_points(gpu_ctx_factory, storage):
    """The Huber bound on and off; the cloud reversed and shuffled gives the same counts and sums within the bound of the same reference;
    the special points (a NaN, infinities, an unobserved cell, |F| == 1, outside each face) are counted as the restatement counts them."""
    vol = K.model(storage == "hashed", True)
    ctx = upload(gpu_ctx_factory(), vol)
    pts = K.cloud(3000, seed=5)
    perm = np.random.default_rng(9).permutation(len(pts))
    for huber in (0.0, 0.02):
        ref = SC.system(vol, pts, K.START, huber=huber)
        got = []
        for name, p in (("as uploaded", pts), ("reversed", pts[::-1].copy()), ("shuffled", pts[perm])):
            ctx.set_source(p)
            got.append(check_system("%s, huber %g, %s" % (storage, huber, name), ctx, vol, p, K.START, huber=huber, ref=ref))
        assert all(tuple(g[1]) == tuple(got[0][1]) for g in got)
    assert SC.system(vol, pts, K.START, huber=0.02)[1][27] < SC.system(vol, pts, K.START)[1][27]
    sp, names = K.special()
    ctx.set_source(sp)
    sums, counts = check_system("%s, special points" % storage, ctx, vol, sp, K.START)
    assert counts[0] == len(sp) - 3 and counts[1] < counts[0] - (len(names) - 3) + 1


def test_block_straddle_and_box_faces(gpu_ctx_factory):
    """Hashed: cells whose corners lie in blocks -1 and 0 on one, two and three axes, and cells whose neighbouring block does not exist.
    Dense: the first and the last cell of each axis, and the cells one step outside them."""
    for name, vol, (inside, outside) in (("hashed", K.plane_hashed(), K.straddle_cells()), ("dense", K.plane_dense(), K.face_cells())):
        ctx = upload(gpu_ctx_factory(), vol)
        pin, pout = K.cell_points(vol, inside), K.cell_points(vol, outside, seed=1)
        pts = np.concatenate([pin, pout])
        ctx.set_source(pts)
        sums, counts = check_system(name + ", crafted cells", ctx, vol, pts, K.EYE)
        assert tuple(counts) == (len(pts), len(pin))
        ctx.set_source(pout)
        assert tuple(ctx.tsdf_cloud_system("source", K.EYE)[1]) == (len(pout), 0)
        tilt = S.pose_of((0.004, -0.003, 0.002), (0.004, -0.003, 0.002))
        ctx.set_source(pts)
        check_system(name + ", crafted cells, tilted", ctx, vol, pts, tilt)


@pytest.mark.parametrize("storage", STORAGES)
def test_failures_and_min_valid(ctxs, storage):
    """A cloud whose points are all invalid fails with NO_CORRESPONDENCES and carries the pose; an all-NaN cloud fails with NO_SOURCE;
    min_valid == n_valid takes the step, min_valid == n_valid + 1 fails it."""
    ctx, vol = ctxs[storage], K.model(storage == "hashed")
    away = (K.cloud(500, seed=3) + f32(40.0)).astype(f32)
    ctx.set_source(away)
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START)
    assert rc == ERR_NO_CORRESPONDENCES == rec["status"] and same_bits(pose, K.START) and (rec["n_depth"], rec["n_valid_first"], rec["iterations"]) == (500, 0, 1)
    assert "icp_tsdf_align_cloud" in ctx.lib.icp_last_error(ctx.h).decode() and "valid points" in ctx.lib.icp_last_error(ctx.h).decode()
    ctx.set_source(np.full((130, 3), np.nan, f32))
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START)
    assert rc == ERR_NO_SOURCE == rec["status"] and same_bits(pose, K.START) and rec["n_depth"] == 0
    assert tuple(ctx.tsdf_cloud_system("source", K.START)[1]) == (0, 0)
    pts = K.cloud(300, seed=12)
    n_valid = SC.system(vol, pts, K.START)[0][1]
    assert 64 < n_valid < 300
    ctx.set_source(pts)
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START, n_iterations=1, min_valid=n_valid)
    assert rc == OK and rec["n_valid_first"] == n_valid and not same_bits(pose, K.START)
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START, n_iterations=1, min_valid=n_valid + 1)
    assert rc == ERR_NO_CORRESPONDENCES and rec["n_valid_first"] == n_valid and same_bits(pose, K.START)


@pytest.mark.parametrize("storage", STORAGES)
def test_the_stop_drains(ctxs, storage):
    """A 1000-iteration call whose record says it stopped early equals the 20-iteration one: what is enqueued behind the stop does nothing."""
    ctx, vol = ctxs[storage], K.model(storage == "hashed")
    pts = K.cloud(3000, seed=5)
    ctx.set_source(pts)
    short = ctx.tsdf_align_cloud("source", K.START, n_iterations=20, trace=True)
    long_ = ctx.tsdf_align_cloud("source", K.START, n_iterations=1000, trace=True)
    assert short[2] == long_[2] == OK and 1 < short[1]["iterations"] < 20 and long_[1]["iterations"] == short[1]["iterations"]
    assert same_bits(short[0], long_[0]) and all(np.array_equal(np.asarray(short[1][k]), np.asarray(long_[1][k])) for k in short[1])
    assert len(short[3]) == len(long_[3]) and all(same_bits(a["pose"], b["pose"]) and u64(a["cost"]) == u64(b["cost"]) for a, b in zip(short[3], long_[3]))
    follow("%s, to the stop" % storage, vol, pts, K.START, short[1], short[2], short[3], n_iterations=20)


def new_volume(storage):
    return SC.HVolume(**K.OPTS) if storage == "hashed" else SC.Volume(K.DIMS, **K.OPTS)


def create(ctx, storage):
    if storage == "hashed":
        ctx.tsdf_create_hashed(block_capacity=64, **K.OPTS)
    else:
        ctx.tsdf_create(dims=K.DIMS, **K.OPTS)


def volume_equals(ctx, vol, what):
    if isinstance(vol, HR.HVolume):
        S.tsdf_blocks_equal_restatement(ctx, vol, what)
    else:
        T, W = ctx.tsdf_volume()
        assert same_bits(T, vol.tsdf) and same_bits(W, vol.weight), what


def follow_track(what, ctx, storage, scans, start, poses, recs, infos, status, **opt):
    """The loop's outputs against the restatement led along the DEVICE's poses: scan k's record within POSE_TOL per step of the
    restatement's alignment from the device's previous pose on the restatement's model; that model then takes the scan at the device's
    pose, so it equals the device's bit for bit at the end, and every fuse info is equal."""
    vol = new_volume(storage)
    assert infos[0] == CR.integrate(vol, scans[0], start) and same_bits(poses[0], np.asarray(start, f32))
    first = OK
    for k in range(1, len(scans)):
        rpose, rrec, _ = SC.align(vol, scans[k], poses[k - 1], **opt)
        r = recs[k - 1]
        diff = float(np.abs(r["pose"] - rpose).max())
        print("%s, scan %d: status %d, %d iterations (restatement %d), %d valid of %d, |pose - restatement| = %.3g" %
              (what, k, r["status"], r["iterations"], rrec["iterations"], r["n_valid_first"], r["n_depth"], diff))
        assert r["status"] == rrec["status"] and (r["n_depth"], r["n_valid_first"]) == (rrec["n_depth"], rrec["n_valid_first"]), (what, k)
        assert same_bits(r["pose"], poses[k]) and diff <= S.POSE_TOL * max(r["iterations"], rrec["iterations"]), (what, k, diff)
        if r["status"] == OK:
            assert infos[k] == CR.integrate(vol, scans[k], poses[k]), (what, k)
        else:
            assert infos[k] == SC.ZERO_INFO and same_bits(poses[k], poses[k - 1]), (what, k)
            first = first or r["status"]
    assert status == first
    volume_equals(ctx, vol, what)
    return vol


@pytest.mark.parametrize("storage", STORAGES)
def test_the_loop(gpu_ctx_factory, storage):
    """Three small scans: records, poses, infos and the volume against the restatement; and against the restatement's own `track`, whose
    model the device's equals bit for bit where the poses agree bit for bit."""
    ctx = gpu_ctx_factory()
    scans = K.track_scans()
    create(ctx, storage)
    out = ctx.track_scans_sdf(scans, K.TRACK_POSES[0], n_iterations=10)
    follow_track(storage + " loop", ctx, storage, scans, K.TRACK_POSES[0], *out, n_iterations=10)
    assert out[3] == OK and len(out[0]) == 3 and len(out[1]) == 2 and len(out[2]) == 3
    for k in (1, 2):
        rot, trans = OF.pose_error(out[0][k], K.TRACK_POSES[k])
        print("scan %d: %.4f rad, %.4f m from its true pose" % (k, rot, trans))
        assert rot < 0.02 and trans < 0.5 * K.OPTS["voxel_size"]
    rv = new_volume(storage)
    rposes, rrecs, rinfos, rstatus = SC.track(rv, scans, K.TRACK_POSES[0], n_iterations=10)
    if all(same_bits(a, b) for a, b in zip(out[0], rposes)):
        volume_equals(ctx, rv, storage + " loop, the restatement's own track")
        assert out[2] == rinfos
    steps = 0
    for k, (r, rr) in enumerate(zip(out[1], rrecs)):
        steps += max(r["iterations"], rr["iterations"])
        assert r["status"] == rr["status"] == OK and float(np.abs(r["pose"] - rr["pose"]).max()) <= S.POSE_TOL * steps, (k, steps)
    # a scan that fails in the middle is skipped and carried; a single scan is only fused
    create(ctx, storage)
    away = (K.cloud(400, seed=3) + f32(40.0)).astype(f32)
    out = ctx.track_scans_sdf([scans[0], away, (scans[2], None)], K.TRACK_POSES[0], n_iterations=10)
    assert out[3] == ERR_NO_CORRESPONDENCES and out[1][0]["status"] == ERR_NO_CORRESPONDENCES and out[1][1]["status"] == OK
    assert "icp_track_scans_sdf" in ctx.lib.icp_last_error(ctx.h).decode()
    follow_track(storage + " loop with a failed scan", ctx, storage, [scans[0], away, scans[2]], K.TRACK_POSES[0], *out, n_iterations=10)
    create(ctx, storage)
    out = ctx.track_scans_sdf([scans[1]], K.TRACK_POSES[1])
    assert out[3] == OK and out[1] == [] and len(out[0]) == 1
    follow_track(storage + " loop of one scan", ctx, storage, [scans[1]], K.TRACK_POSES[1], *out)


def test_after_evict_and_insert(gpu_ctx_factory):
    """After an evict and an insert (the pool compacted, then refilled) the alignment equals that on a fresh volume uploaded with the same blocks."""
    a, b = upload(gpu_ctx_factory(), K.model(True)), gpu_ctx_factory()
    einfo, ec, et, ew = a.tsdf_evict_blocks((0.0, 0.0, 2.0), 1.5)
    assert 0 < einfo["n_evicted"] < len(K.model(True).blocks)
    a.tsdf_insert_blocks(ec, et, ew)
    _, coords, t, w = a.tsdf_blocks()
    b.tsdf_create_hashed(block_capacity=1 << 10, **K.OPTS)
    b.tsdf_upload_blocks(coords, t, w)
    pts = K.cloud(3000, seed=5)
    got = []
    for ctx in (a, b):
        ctx.set_source(pts)
        got.append((ctx.tsdf_cloud_system("source", K.START), ctx.tsdf_align_cloud("source", K.START, trace=True)))
    (sa, ca), (sb, cb) = got[0][0], got[1][0]
    assert tuple(ca) == tuple(cb) and np.array_equal(u64(sa), u64(sb))
    ra, rb = got[0][1], got[1][1]
    assert ra[2] == rb[2] == OK and same_bits(ra[0], rb[0]) and ra[1]["iterations"] == rb[1]["iterations"] and u64(ra[1]["cost_last"]) == u64(rb[1]["cost_last"])
    check_system("after evict and insert", a, K.model(True), pts, K.START)


@pytest.mark.parametrize("storage", STORAGES)
def test_refusals_leave_the_volume_as_it_was(gpu_ctx_factory, storage):
    from icp_amd import binding
    hashed = storage == "hashed"
    bare = gpu_ctx_factory()
    lib = bare.lib
    p = binding.pose_to_c(K.START); o = binding.sdf_options()
    sums = np.zeros(28); cnt = (ctypes.c_int32 * 2)(); rec = binding.IcpSdfFrame()
    msg = lambda c: lib.icp_last_error(c.h).decode()
    system = lambda c, which, pose, opt, s=sums, n=cnt: lib.icp_tsdf_cloud_system(c.h, which, binding._ptr(pose), ctypes.byref(opt) if opt is not None else None, binding._ptr(s), n)
    align = lambda c, which, pose, opt: lib.icp_tsdf_align_cloud(c.h, which, ctypes.byref(opt) if opt is not None else None, binding._ptr(pose), ctypes.byref(rec), None)
    bare.set_source(K.cloud(50))
    assert system(bare, 1, p, o) == ERR_INVALID_ARG and "icp_tsdf_cloud_system" in msg(bare) and "no volume" in msg(bare)
    assert align(bare, 1, p, o) == ERR_INVALID_ARG and "icp_tsdf_align_cloud" in msg(bare) and "no volume" in msg(bare)
    ctx = upload(gpu_ctx_factory(), K.model(hashed))
    ctx.set_source(K.cloud(300, seed=12))
    before = state(ctx, hashed)
    nan = p.copy(); nan[13] = np.nan
    inf = p.copy(); inf[0] = np.inf
    for name, call in (("icp_tsdf_cloud_system", system), ("icp_tsdf_align_cloud", align)):
        for which in (2, -1):
            assert call(ctx, which, p, o) == ERR_INVALID_ARG and name in msg(ctx) and "which" in msg(ctx)
        assert call(ctx, 1, None, o) == ERR_INVALID_ARG and name in msg(ctx) and "pose" in msg(ctx)
        assert call(ctx, 1, nan, o) == ERR_INVALID_ARG and call(ctx, 1, inf, o) == ERR_INVALID_ARG and "finite" in msg(ctx)
        assert call(ctx, 1, p, None) == ERR_INVALID_ARG and "options" in msg(ctx)
        for bad in (dict(stride=2), dict(stride=0), dict(n_iterations=0), dict(n_iterations=1001), dict(min_valid=5), dict(huber=-1.0), dict(stop_rotation=-1.0)):
            assert call(ctx, 1, p, binding.sdf_options(**bad)) == ERR_INVALID_ARG and name in msg(ctx), bad
        assert call(ctx, 1, p, binding.sdf_options(stride=2)) == ERR_INVALID_ARG and "stride" in msg(ctx)
        assert call(ctx, 0, p, o) == ERR_NO_TARGET and name in msg(ctx) and "target" in msg(ctx)
    assert system(ctx, 1, p, o, None, cnt) == ERR_INVALID_ARG and "null output" in msg(ctx)
    assert lib.icp_tsdf_cloud_system(ctx.h, 1, binding._ptr(p), ctypes.byref(o), binding._ptr(sums), None) == ERR_INVALID_ARG
    fresh = upload(gpu_ctx_factory(), K.model(hashed))
    assert align(fresh, 1, p, o) == ERR_NO_SOURCE and "icp_tsdf_align_cloud" in msg(fresh) and "source" in msg(fresh)
    # the loop
    a, b = K.cloud(40, seed=1), K.cloud(50, seed=2)
    out = (binding.IcpSdfFrame * 2)()

    def track(scans, counts, n_scans, pose=p, opt=o, out=out):
        xp = None if scans is None else (ctypes.c_void_p * len(scans))(*[binding._ptr(s) for s in scans])
        cn = None if counts is None else (ctypes.c_int32 * len(counts))(*counts)
        return lib.icp_track_scans_sdf(ctx.h, xp, cn, n_scans, ctypes.byref(opt) if opt is not None else None, binding._ptr(pose), out, None)
    who = "icp_track_scans_sdf"
    assert track([a, b], [40, 50], 0) == ERR_INVALID_ARG and who in msg(ctx) and "n_scans" in msg(ctx)
    assert track(None, [40, 50], 2) == ERR_INVALID_ARG and track([a, b], None, 2) == ERR_INVALID_ARG
    assert track([a, None], [40, 50], 2) == ERR_INVALID_ARG and "scan" in msg(ctx)
    assert track([a, b], [40, 0], 2) == ERR_INVALID_ARG and "scan" in msg(ctx)
    assert track([a, b], [40, 50], 2, out=None) == ERR_INVALID_ARG and "null output" in msg(ctx)
    assert track([a, b], [40, 50], 2, pose=None) == ERR_INVALID_ARG and track([a, b], [40, 50], 2, pose=nan) == ERR_INVALID_ARG and "pose" in msg(ctx)
    assert track([a, b], [40, 50], 2, opt=None) == ERR_INVALID_ARG and track([a, b], [40, 50], 2, opt=binding.sdf_options(stride=3)) == ERR_INVALID_ARG and "stride" in msg(ctx)
    assert lib.icp_track_scans_sdf(bare.h, None, None, 1, ctypes.byref(o), binding._ptr(p), None, None) == ERR_INVALID_ARG and "no volume" in msg(bare)
    assert same_state(before, state(ctx, hashed), hashed)
    # and the context still works: the resident source is the one set above
    assert ctx.tsdf_align_cloud("source", K.START)[2] == OK


def test_outcome_on_twelve_scans(gpu_ctx_factory, tmp_path):
    """eth.track_tsdf on the twelve scans of tests/tsdf_cloud_outcome_fixture.py (10 cm voxels, truncation 0.4 m): every scan aligns, the
    worst ends within 0.02 rad and 0.05 m of its true pose, the model passes that fixture's assert_surface, and the records agree with the
    restatement's (tests/sdf_cloud_outcome_fixture.py) within POSE_TOL per step taken so far.  eth.reconstruct(tracker="sdf") meshes that
    one model; tracker="map" returns what the call without the argument returns."""
    from icp_amd import eth
    clouds, truth, normals = CF.scans()
    rvol, rposes, rrecs, rinfos, rstatus = OF.tracked()
    ctx = gpu_ctx_factory()
    kw = dict(voxel_size=CF.VOXEL, truncation=CF.TRUNCATION, origin=CF.ORIGIN, max_range=CF.MAX_RANGE, block_capacity=256)
    poses, recs, infos, status = eth.track_tsdf(ctx, clouds, truth[0], **kw, **OF.SDF_OPTIONS)
    OF.assert_outcome(poses, recs, status)
    steps = 0
    for k, (r, rr) in enumerate(zip(recs, rrecs)):
        steps += max(r["iterations"], rr["iterations"])
        diff = float(np.abs(r["pose"] - rr["pose"]).max())
        print("scan %d: %d iterations (restatement %d), |pose - restatement| = %.3g (bound %.3g)" % (k + 1, r["iterations"], rr["iterations"], diff, S.POSE_TOL * steps))
        assert diff <= S.POSE_TOL * steps, (k, diff)
    _, coords, t, w = ctx.tsdf_blocks()
    dvol = SC.HVolume(**CF.options())
    for c, tt, ww in zip(coords, t, w):
        dvol.blocks[tuple(int(x) for x in c)] = [tt, ww]
    CF.assert_surface(dvol)
    assert all(i["n_updated"] > 0 for i in infos) and infos[-1]["n_blocks"] == len(coords)
    # the whole chain on one model
    path = str(tmp_path / "room_sdf.ply")
    sposes, srecs, sstatus, mesh = eth.reconstruct(ctx, list(zip(clouds, normals)), truth[0], tsdf_voxel_size=CF.VOXEL, truncation=CF.TRUNCATION, mesh_path=path,
                                                   tracker="sdf", block_capacity=256, **OF.SDF_OPTIONS)
    assert sstatus == OK and len(mesh[0]) > 1000 and len(mesh[2]) > 1000 and all(same_bits(a, b) for a, b in zip(sposes, poses))
    print("reconstruct(tracker='sdf'): %d vertices, %d triangles" % (len(mesh[0]), len(mesh[2])))
    # tracker="map" is the call as it was
    ctx.set_gicp_options(1e-3, 0)
    args = dict(tsdf_voxel_size=CF.VOXEL, truncation=CF.TRUNCATION, voxel_size=0.25, hashed=True, n_iterations=30, min_valid=64)
    was = eth.reconstruct(ctx, list(zip(clouds, normals)), truth[0], **args)
    now = eth.reconstruct(ctx, list(zip(clouds, normals)), truth[0], tracker="map", **args)
    assert was[2] == now[2] and all(same_bits(a, b) for a, b in zip(was[0], now[0])) and len(was[1]) == len(now[1])
    assert all(same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(was[3], now[3]))
    mrot, mtrans = OF.worst(now[0])
    print("tracked against the voxel map (0.25 m cells): status %d, %d of %d scans aligned, worst scan %.4f rad and %.4f m from its true pose"
          % (now[2], sum(r["status"] == OK for r in now[1]), len(now[1]), mrot, mtrans))
    print("  per scan [rad / m]: " + ", ".join("%.4f / %.3f" % OF.pose_error(T, G) for T, G in zip(now[0], truth)))
    with pytest.raises(ValueError):
        eth.reconstruct(ctx, list(zip(clouds, normals)), truth[0], tracker="nonsense")
