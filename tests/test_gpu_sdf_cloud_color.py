"""A coloured laser scan aligned to the coloured TSDF volume with the photometric term on the device (icp_tsdf_cloud_system_color,
icp_tsdf_align_cloud_color, icp_track_scans_sdf_photometric) against the numpy restatement of the contract
(tests/sdf_cloud_color_restatement.py).  The three counts are compared exactly; every one of the 29 sums with the contract's bound,
n_valid 2^-52 sum |term| with sum |term| from the restatement (derived from the summation: the terms are the same doubles, only their order
differs); two runs bit for bit; every traced iteration's pose within support.POSE_TOL -- the tolerance of tests/test_gpu_sdf_cloud.py -- of
the restatement's step from the DEVICE's previous pose.  Sizes around a wave, a work-group's pass, one block's and two blocks' points, both
storages; the sizes at which k_sdf_solve_color's fold changes shape; the special points of tests/sdf_cloud_color_cases.py; dense against
hashed; cells across blocks -1 / 0 and in the last layer of a dense box; failed alignments; the loop; the refusals; and the outcome on the
flat textured wall of tests/sdf_cloud_color_outcome_fixture.py."""
import ctypes

import numpy as np
import pytest

import htsdf_color_restatement as HC
import htsdf_restatement as HR
import sdf_cloud_cases as K
import sdf_cloud_color_cases as CK
import sdf_cloud_color_outcome_fixture as OF
import sdf_cloud_color_restatement as R
import sdf_cloud_restatement as SC
import sdf_restatement as SR
import support as S
import tsdf_cloud_color_restatement as CC
from support import same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = 0, 1, 3, 4, 8
STEPS = 3
STORAGES = ("dense", "hashed")
W = CK.WEIGHT


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def upload(ctx, vol, color=True):
    """A restatement's volume, dense or hashed, with its colours (color=False: the geometry alone, into a volume without colours)."""
    opts = dict(origin=tuple(float(x) for x in vol.o), voxel_size=float(vol.s), truncation=float(vol.trunc), max_weight=float(vol.max_w), max_depth=float(vol.max_d))
    if isinstance(vol, HR.HVolume):
        ctx.tsdf_create_hashed(block_capacity=max(64, len(vol.blocks)), color=color, **opts)
        ctx.tsdf_upload_blocks(*vol.sorted_blocks(), *(HC.sorted_colors(vol) if color else ()))
    else:
        ctx.tsdf_create(dims=vol.dims, color=color, **opts)
        ctx.tsdf_upload(vol.tsdf, vol.weight)
        if color:
            ctx.tsdf_color_upload(vol.rgb, vol.wc)
    return ctx


def resident(ctx, which, pts, rgba):
    (ctx.set_source if which == "source" else ctx.set_target)(pts, None, rgba)


@pytest.fixture(scope="module")
def ctxs(gpu_ctx_factory):
    """One context per storage holding sdf_cloud_color_cases.colored_model(): the dense box, and the same voxels and colours in blocks."""
    return {"dense": upload(gpu_ctx_factory(), CK.colored_model(False)), "hashed": upload(gpu_ctx_factory(), CK.colored_model(True))}


def check_system(what, ctx, vol, pts, rgba, pose, which="source", huber=0.0, color_huber=0.0, ref=None):
    """Counts exactly; every sum within n_valid 2^-52 sum |term| of the restatement's; a second call the same bits."""
    rcounts, rsums, rabs = ref if ref is not None else R.system(vol, pts, rgba, pose, huber=huber, weight=W, color_huber=color_huber)
    sums, counts = ctx.tsdf_cloud_system(which, pose, huber=huber, color_weight=W, color_huber=color_huber)
    sums2, counts2 = ctx.tsdf_cloud_system(which, pose, huber=huber, color_weight=W, color_huber=color_huber)
    bound = rcounts[1] * 2.0 ** -52 * rabs
    err = np.abs(sums - rsums)
    print("%s: counts %s, worst |sum - restatement| / bound = %.3g" % (what, tuple(counts), (err / np.maximum(bound, 1e-300)).max()))
    assert sums.shape == (29,) and tuple(counts) == tuple(rcounts), (what, counts, rcounts)
    assert (err <= bound).all(), (what, err, bound)
    assert np.array_equal(u64(sums), u64(sums2)) and tuple(counts2) == tuple(counts), what
    return sums, counts


def follow(what, vol, pts, rgba, start, rec, rc, trace, color_huber=0.0, **opt):
    """Every iteration's pose within S.POSE_TOL of the restatement's step from the DEVICE's previous pose, n_valid and n_color exactly, both
    costs within the summation bound; a step the restatement fails is failed on the device, with the pose carried."""
    o = SC.options(**opt)
    prev = np.asarray(start, f32)
    first = None
    assert len(trace) == rec["iterations"] >= 1
    for i, t in enumerate(trace):
        counts, sums, sabs = R.system(vol, pts, rgba, prev, weight=W, color_huber=color_huber, **o)
        first = counts if first is None else first
        want, x = (None, None) if counts[0] == 0 else SR.step(sums, counts, prev, **o)
        bound = counts[1] * 2.0 ** -52 * sabs
        assert (t["n_valid"], t["n_color"]) == counts[1:], (what, i, t["n_valid"], t["n_color"], counts)
        assert abs(t["cost"] - sums[27]) <= bound[27] and abs(t["cost_color"] - sums[28]) <= bound[28], (what, i)
        if want is None:
            status = ERR_NO_SOURCE if counts[0] == 0 else ERR_NO_CORRESPONDENCES
            assert t["status"] == status == rec["status"] == rc and i == len(trace) - 1, (what, i, t["status"])
            assert same_bits(t["pose"], prev) and same_bits(rec["pose"], np.asarray(start, f32)), (what, i)
            break
        diff = float(np.abs(t["pose"] - want).max())
        print("%s, step %d: %d coloured of %d valid of %d, cost %.6g (colour %.6g), |pose - restatement| = %.3g" % (what, i, counts[2], counts[1], counts[0], t["cost"], t["cost_color"], diff))
        assert t["status"] == OK and diff <= S.POSE_TOL, (what, i, diff)
        prev = t["pose"]
        if i == len(trace) - 1:
            assert rc == OK and rec["status"] == OK and same_bits(rec["pose"], t["pose"])
            assert SR.stopped(x, **o) or i == o["n_iterations"] - 1, (what, i)
    assert (rec["n_depth"], rec["n_valid_first"], rec["n_valid_last"]) == (first[0], trace[0]["n_valid"], trace[-1]["n_valid"])
    assert (rec["n_color_first"], rec["n_color_last"]) == (trace[0]["n_color"], trace[-1]["n_color"])
    assert u64(rec["cost_first"]) == u64(trace[0]["cost"]) and u64(rec["cost_last"]) == u64(trace[-1]["cost"])
    assert u64(rec["cost_color_first"]) == u64(trace[0]["cost_color"]) and u64(rec["cost_color_last"]) == u64(trace[-1]["cost_color"])


@pytest.mark.parametrize("n", CK.SIZES)
@pytest.mark.parametrize("storage", STORAGES)
def test_sizes(ctxs, storage, n):
    """The sums and three traced steps at every size, the cloud as the source and as the target (whose planes are padded to a wave); a
    permuted upload stays within the bound of the same reference."""
    ctx, vol = ctxs[storage], CK.colored_model(storage == "hashed")
    pts = K.cloud(n, seed=100 + n)
    rgba = CK.wall_colors(pts, seed=n)
    ref = R.system(vol, pts, rgba, K.START, weight=W)
    opt = dict(n_iterations=STEPS, min_valid=6, stop_rotation=0.0, stop_translation=0.0)
    for which in ("source", "target"):
        resident(ctx, which, pts, rgba)
        what = "%s, %d points as the %s" % (storage, n, which)
        check_system(what, ctx, vol, pts, rgba, K.START, which, ref=ref)
        pose, rec, rc, trace = ctx.tsdf_align_cloud(which, K.START, trace=True, color_weight=W, **opt)
        follow(what, vol, pts, rgba, K.START, rec, rc, trace, **opt)
        assert same_bits(pose, rec["pose"])
    if n >= 255:
        assert ref[0][2] >= 64 and rec["iterations"] == STEPS and rc == OK
    perm = np.random.default_rng(n).permutation(n)
    resident(ctx, "source", pts[perm], rgba[perm])
    check_system("%s, %d points, permuted" % (storage, n), ctx, vol, pts, rgba, K.START, ref=ref)


@pytest.mark.parametrize("blocks", CK.FOLD_BLOCKS)
@pytest.mark.parametrize("storage", STORAGES)
def test_fold_sizes(ctxs, storage, blocks):
    """The coloured accumulate over 1, 64, 65, 256, 257 and 513 blocks: the sizes at which k_sdf_solve_color's fold changes shape.  The
    dense and the hashed model hold the same fields (tests/test_sdf_cloud_color_host.py), so one reference serves both."""
    ctx = ctxs[storage]
    n = blocks * CK.PER_BLOCK
    pts, rgba = K.fold_cloud()[:n], CK.fold_colors()[:n]
    ctx.set_source(pts, None, rgba)
    ref = CK.fold_reference(blocks)
    assert ref[0][0] == n and ref[0][2] > 0.5 * n
    check_system("%s, %d blocks" % (storage, blocks), ctx, None, pts, rgba, K.START, ref=ref)


@pytest.mark.parametrize("storage", STORAGES)
def test_special_points_hubers_and_orders(gpu_ctx_factory, storage):
    """The special points (one Wc == 0 corner, an inf in the colour array, black, white, the fourth-byte twins, coloured points without a
    valid cell, and K.special()'s own) are counted and summed as the restatement does; flipping every fourth byte leaves the bits; both
    Huber bounds on and off, the cloud reversed and shuffled."""
    vol = CK.special_model(storage == "hashed")
    ctx = upload(gpu_ctx_factory(), vol)
    sp, rgba, names, _ = CK.special()
    ctx.set_source(sp, None, rgba)
    sums, counts = check_system("%s, special points" % storage, ctx, vol, sp, rgba, K.START)
    assert counts[0] == len(sp) - 3 and counts[2] < counts[1] < counts[0]
    flipped = rgba.copy(); flipped[:, 3] ^= 0xFF
    ctx.set_source(sp, None, flipped)
    assert np.array_equal(u64(ctx.tsdf_cloud_system("source", K.START, color_weight=W)[0]), u64(sums))
    # each special point alone, with eight plain wall points around it so that the sums are not empty
    for name in ("wc_zero", "s_inf", "black", "white", "alpha_00", "alpha_ff", "free", "unobserved"):
        idx = np.r_[0:8, names[name]]
        ctx.set_source(sp[idx], None, rgba[idx])
        check_system("%s, %s" % (storage, name), ctx, vol, sp[idx], rgba[idx], K.START)
    pts = K.cloud(3000, seed=5)
    col = CK.wall_colors(pts, seed=5)
    col[::7, :3] = 255 - col[::7, :3]                    # (some large colour residuals for the colour Huber to bound)
    perm = np.random.default_rng(9).permutation(len(pts))
    for huber, color_huber in ((0.0, 0.0), (0.02, 0.0), (0.0, 0.05), (0.02, 0.05)):
        ref = R.system(vol, pts, col, K.START, huber=huber, weight=W, color_huber=color_huber)
        got = []
        for what, o in (("as uploaded", slice(None)), ("reversed", slice(None, None, -1)), ("shuffled", perm)):
            ctx.set_source(np.ascontiguousarray(pts[o]), None, np.ascontiguousarray(col[o]))
            got.append(check_system("%s, huber %g, colour huber %g, %s" % (storage, huber, color_huber, what), ctx, vol, pts, col, K.START, huber=huber,
                                    color_huber=color_huber, ref=ref))
        assert all(tuple(g[1]) == tuple(got[0][1]) for g in got)
    plain, bounded = R.system(vol, pts, col, K.START, weight=W), R.system(vol, pts, col, K.START, weight=W, color_huber=0.05)
    assert bounded[1][28] < plain[1][28]


def test_dense_equals_hashed(ctxs):
    """The same field and the same colours in both storages: the counts are equal, the sums within the bound."""
    pts = K.cloud(3000, seed=5)
    rgba = CK.wall_colors(pts, seed=5)
    ref = R.system(CK.colored_model(), pts, rgba, K.START, weight=W)
    got = []
    for storage in STORAGES:
        ctxs[storage].set_source(pts, None, rgba)
        got.append(ctxs[storage].tsdf_cloud_system("source", K.START, color_weight=W))
    assert tuple(got[0][1]) == tuple(got[1][1]) == tuple(ref[0])
    assert (np.abs(got[0][0] - got[1][0]) <= ref[0][1] * 2.0 ** -52 * ref[2]).all()


def test_block_straddle_and_box_faces(gpu_ctx_factory):
    """Hashed: cells whose corners lie in blocks -1 and 0 on one, two and three axes, interior cells, and cells whose neighbouring block
    does not exist, against the restatement and against the dense call on the box that covers the eight blocks (equal counts; that box has
    another origin, so its fp32 cell fractions differ and its sums are compared with its own restatement).  Dense: the first and the last
    cell of each axis, and the cells one step outside them."""
    cover = upload(gpu_ctx_factory(), CK.plane_cover())
    for name, vol, (inside, outside) in (("hashed", CK.plane_hashed(), K.straddle_cells()), ("dense", CK.plane_dense(), K.face_cells())):
        ctx = upload(gpu_ctx_factory(), vol)
        pin, pout = K.cell_points(vol, inside), K.cell_points(vol, outside, seed=1)
        pts = np.concatenate([pin, pout])
        rgba = CK.wall_colors(pts, seed=3)
        ctx.set_source(pts, None, rgba)
        sums, counts = check_system(name + ", crafted cells", ctx, vol, pts, rgba, K.EYE)
        assert tuple(counts) == (len(pts), len(pin), len(pin))
        ctx.set_source(pout, None, rgba[len(pin):])
        assert tuple(ctx.tsdf_cloud_system("source", K.EYE, color_weight=W)[1]) == (len(pout), 0, 0)
        tilt = S.pose_of((0.004, -0.003, 0.002), (0.004, -0.003, 0.002))
        ctx.set_source(pts, None, rgba)
        check_system(name + ", crafted cells, tilted", ctx, vol, pts, rgba, tilt)
        if name == "hashed":
            cover.set_source(pin, None, rgba[:len(pin)])
            csums, ccounts = check_system("the covering box", cover, CK.plane_cover(), pin, rgba[:len(pin)], K.EYE)
            ctx.set_source(pin, None, rgba[:len(pin)])
            hsums, hcounts = ctx.tsdf_cloud_system("source", K.EYE, color_weight=W)
            assert tuple(ccounts) == tuple(hcounts) == (len(pin),) * 3


@pytest.mark.parametrize("storage", STORAGES)
def test_align_and_its_failures(ctxs, storage):
    """From START to the stop against the coloured model, every iteration followed; a cloud without a valid point fails with
    NO_CORRESPONDENCES and carries the pose; an all-NaN cloud fails with NO_SOURCE; min_valid == n_valid takes the step, n_valid + 1 fails it."""
    ctx, vol = ctxs[storage], CK.colored_model(storage == "hashed")
    pts = K.cloud(3000, seed=5)
    rgba = CK.wall_colors(pts, seed=5)
    ctx.set_source(pts, None, rgba)
    pose, rec, rc, trace = ctx.tsdf_align_cloud("source", K.START, trace=True, color_weight=W)
    follow("%s, to the stop" % storage, vol, pts, rgba, K.START, rec, rc, trace, n_iterations=20)
    assert rc == OK and 1 < rec["iterations"] < 20 and np.abs(pose - K.EYE).max() < 0.5 * np.abs(K.START - K.EYE).max()
    short = ctx.tsdf_align_cloud("source", K.START, color_weight=W)
    assert same_bits(short[0], pose) and same_records([short[1]], [rec])
    # the geometric call on the same context is the call it was: the 28 sums, the geometric record
    gs, gc = ctx.tsdf_cloud_system("source", K.START)
    assert gs.shape == (28,) and len(gc) == 2 and "n_color_first" not in ctx.tsdf_align_cloud("source", K.START)[1]
    assert gs.shape == ctx.tsdf_cloud_system("source", K.START, color_weight=0.0)[0].shape
    away = (K.cloud(500, seed=3) + f32(40.0)).astype(f32)
    ctx.set_source(away, None, CK.wall_colors(away))
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START, color_weight=W)
    assert rc == ERR_NO_CORRESPONDENCES == rec["status"] and same_bits(pose, K.START) and (rec["n_depth"], rec["n_valid_first"], rec["n_color_first"], rec["iterations"]) == (500, 0, 0, 1)
    msg = ctx.lib.icp_last_error(ctx.h).decode()
    assert "icp_tsdf_align_cloud_color" in msg and "valid points" in msg
    ctx.set_source(np.full((130, 3), np.nan, f32), None, np.zeros((130, 4), np.uint8))
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START, color_weight=W)
    assert rc == ERR_NO_SOURCE == rec["status"] and same_bits(pose, K.START) and rec["n_depth"] == 0
    assert tuple(ctx.tsdf_cloud_system("source", K.START, color_weight=W)[1]) == (0, 0, 0)
    pts = K.cloud(300, seed=12)
    n_valid = R.system(vol, pts, CK.wall_colors(pts), K.START, weight=W)[0][1]
    assert 64 < n_valid < 300
    ctx.set_source(pts, None, CK.wall_colors(pts))
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START, n_iterations=1, min_valid=n_valid, color_weight=W)
    assert rc == OK and rec["n_valid_first"] == n_valid and not same_bits(pose, K.START)
    pose, rec, rc = ctx.tsdf_align_cloud("source", K.START, n_iterations=1, min_valid=n_valid + 1, color_weight=W)
    assert rc == ERR_NO_CORRESPONDENCES and rec["n_valid_first"] == n_valid and same_bits(pose, K.START)


def new_volume(storage):
    return CC.add_color(SC.HVolume(**K.OPTS) if storage == "hashed" else SC.Volume(K.DIMS, **K.OPTS))


def create(ctx, storage):
    if storage == "hashed":
        ctx.tsdf_create_hashed(block_capacity=64, color=True, **K.OPTS)
    else:
        ctx.tsdf_create(dims=K.DIMS, color=True, **K.OPTS)


def same_records(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


@pytest.mark.parametrize("storage", STORAGES)
def test_the_loop(gpu_ctx_factory, storage):
    """track_scans_sdf(colors=..., color_weight=0.1) on four small coloured scans: the restatement led along the DEVICE's poses -- scan k's
    record within POSE_TOL per step of the restatement's alignment from the device's previous pose on the restatement's model, which then
    takes the scan at the device's pose, so infos, n_colored, geometry and colours are equal at the end.  With color_weight=0 the call
    returns what track_scans_sdf(colors=...) returns, bit for bit."""
    scans, cols, truth = CK.track_scans()
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    create(ctx, storage)
    opt = dict(n_iterations=10)
    poses, recs, infos, status, ncs = ctx.track_scans_sdf(scans, truth[0], colors=cols, color_weight=W, **opt)
    assert status == OK and len(poses) == 4 and len(recs) == 3 and all("n_color_first" in r for r in recs)
    vol = new_volume(storage)
    want = [CC.integrate(vol, scans[0], cols[0], truth[0])]
    assert same_bits(poses[0], truth[0])
    for k in range(1, len(scans)):
        rpose, rrec, _ = R.align(vol, scans[k], cols[k], poses[k - 1], weight=W, **opt)
        r = recs[k - 1]
        diff = float(np.abs(r["pose"] - rpose).max())
        print("%s loop, scan %d: %d iterations (restatement %d), %d coloured of %d valid, |pose - restatement| = %.3g" %
              (storage, k, r["iterations"], rrec["iterations"], r["n_color_first"], r["n_valid_first"], diff))
        assert r["status"] == rrec["status"] == OK and (r["n_depth"], r["n_valid_first"], r["n_color_first"]) == (rrec["n_depth"], rrec["n_valid_first"], rrec["n_color_first"])
        assert r["n_color_first"] > 64 and same_bits(r["pose"], poses[k]) and diff <= S.POSE_TOL * max(r["iterations"], rrec["iterations"]), (k, diff)
        want.append(CC.integrate(vol, scans[k], cols[k], poses[k]))
    assert [w[0] for w in want] == infos and [w[2] for w in want] == ncs and all(n > 0 for n in ncs)
    if storage == "hashed":
        S.tsdf_blocks_equal_restatement(ctx, vol, storage + " loop")
        got = ctx.tsdf_blocks(colors=True)[4:]
    else:
        T, Wt = ctx.tsdf_volume()
        assert same_bits(T, vol.tsdf) and same_bits(Wt, vol.weight)
        got = ctx.tsdf_color_volume()
    assert all(same_bits(a, b) for a, b in zip(got, CC.colors_of(vol)))
    # a weight of zero is the call as it was
    create(ctx, storage); create(twin, storage)
    zero = ctx.track_scans_sdf(scans, truth[0], colors=cols, color_weight=0.0, color_huber=0.0, **opt)
    was = twin.track_scans_sdf(scans, truth[0], colors=cols, **opt)
    assert len(zero) == len(was) == 5 and zero[3] == was[3] and zero[2] == was[2] and zero[4] == was[4]
    assert all(same_bits(a, b) for a, b in zip(zero[0], was[0])) and same_records(zero[1], was[1]) and "n_color_first" not in zero[1][0]
    # a scan that fails in the middle is skipped and carries the pose
    create(ctx, storage)
    far = [scans[0], (scans[1] + f32(50.0)).astype(f32), scans[2]]
    out = ctx.track_scans_sdf(far, truth[0], colors=cols[:3], color_weight=W, **opt)
    assert out[3] == ERR_NO_CORRESPONDENCES == out[1][0]["status"] and out[1][1]["status"] == OK and out[4][1] == 0 and out[2][1]["n_updated"] == 0
    assert same_bits(out[0][1], out[0][0]) and "icp_track_scans_sdf_photometric" in ctx.lib.icp_last_error(ctx.h).decode()


@pytest.mark.parametrize("storage", STORAGES)
def test_refusals(gpu_ctx_factory, storage):
    """Every refusal of the three calls names the call; the context works afterwards."""
    from icp_amd import binding
    hashed = storage == "hashed"
    ctx = gpu_ctx_factory()
    lib = ctx.lib
    p = binding.pose_to_c(K.START); o = binding.sdf_options(); co = binding.sdf_color_options(weight=W)
    sums = np.zeros(29); cnt = (ctypes.c_int32 * 3)(); rec = binding.IcpSdfColorFrame()
    msg = lambda: lib.icp_last_error(ctx.h).decode()
    ref = lambda x: ctypes.byref(x) if x is not None else None
    system = lambda which=1, pose=p, opt=o, copt=co, s=sums, n=cnt: lib.icp_tsdf_cloud_system_color(ctx.h, which, binding._ptr(pose), ref(opt), ref(copt), binding._ptr(s), n)
    align = lambda which=1, pose=p, opt=o, copt=co: lib.icp_tsdf_align_cloud_color(ctx.h, which, ref(opt), ref(copt), binding._ptr(pose), ctypes.byref(rec), None)
    pts = K.cloud(300, seed=12)
    rgba = CK.wall_colors(pts)
    calls = (("icp_tsdf_cloud_system_color", system), ("icp_tsdf_align_cloud_color", align))
    # no volume; a volume without colours
    ctx.set_source(pts, None, rgba)
    for name, call in calls:
        assert call() == ERR_INVALID_ARG and name in msg() and "no volume" in msg()
    upload(ctx, K.model(hashed), color=False)
    for name, call in calls:
        assert call() == ERR_INVALID_ARG and name in msg() and "no colours" in msg() and "volume" in msg()
    with pytest.raises(binding.IcpError):
        ctx.tsdf_cloud_system("source", K.START, color_weight=W)
    assert ctx.tsdf_cloud_system("source", K.START)[1][1] > 64      # (the geometric call takes that volume)
    # a coloured volume: the call's own checks in sdf_cloud_check's order, then the colour ones
    upload(ctx, CK.colored_model(hashed))
    nan = p.copy(); nan[13] = np.nan
    for name, call in calls:
        for which in (2, -1):
            assert call(which) == ERR_INVALID_ARG and name in msg() and "which" in msg()
        assert call(pose=None) == ERR_INVALID_ARG and "pose" in msg() and call(pose=nan) == ERR_INVALID_ARG and "finite" in msg()
        assert call(opt=None) == ERR_INVALID_ARG and "options" in msg()
        for bad in (dict(stride=2), dict(stride=0), dict(n_iterations=0), dict(min_valid=5), dict(huber=-1.0)):
            assert call(opt=binding.sdf_options(**bad)) == ERR_INVALID_ARG and name in msg(), bad
        assert call(opt=binding.sdf_options(stride=2)) == ERR_INVALID_ARG and "stride" in msg()
        assert call(0) == ERR_NO_TARGET and name in msg()
        assert call(copt=None) == ERR_INVALID_ARG and name in msg() and "colour options" in msg()
        for weight in (0.0, -0.1, float("nan"), float("inf")):
            assert call(copt=binding.IcpSdfColorOptions(weight, 0.0)) == ERR_INVALID_ARG and name in msg() and "weight" in msg(), weight
        assert call(copt=binding.IcpSdfColorOptions(W, -1.0)) == ERR_INVALID_ARG and "huber" in msg()
    assert system(s=None) == ERR_INVALID_ARG and "null output" in msg()
    assert lib.icp_tsdf_cloud_system_color(ctx.h, 1, binding._ptr(p), ref(o), ref(co), binding._ptr(sums), None) == ERR_INVALID_ARG and "null output" in msg()
    ctx.set_source(pts)                                  # a cloud without colours
    for name, call in calls:
        assert call() == ERR_INVALID_ARG and name in msg() and "cloud has no colours" in msg()
    ctx.set_source(pts, None, rgba)
    assert system() == OK and align() == OK and rec.n_color_first > 64
    # the loop
    who = "icp_track_scans_sdf_photometric"
    a, b = K.cloud(40, seed=1), K.cloud(50, seed=2)
    ca, cb = CK.wall_colors(a), CK.wall_colors(b)
    out = (binding.IcpSdfColorFrame * 2)()

    def track(scans, colors, counts, n_scans=2, pose=p, opt=o, copt=co, out=out):
        arr = lambda xs: None if xs is None else (ctypes.c_void_p * len(xs))(*[None if x is None else binding._ptr(x) for x in xs])
        cn = None if counts is None else (ctypes.c_int32 * len(counts))(*counts)
        return lib.icp_track_scans_sdf_photometric(ctx.h, arr(scans), arr(colors), cn, n_scans, ref(opt), ref(copt), binding._ptr(pose), out, None, None)
    assert track([a, b], [ca, cb], [40, 50], 0) == ERR_INVALID_ARG and who in msg() and "n_scans" in msg()
    assert track(None, [ca, cb], [40, 50]) == ERR_INVALID_ARG and track([a, b], [ca, cb], None) == ERR_INVALID_ARG
    assert track([a, None], [ca, cb], [40, 50]) == ERR_INVALID_ARG and "scan" in msg()
    assert track([a, b], None, [40, 50]) == ERR_INVALID_ARG and who in msg() and "null colours" in msg()
    assert track([a, b], [ca, None], [40, 50]) == ERR_INVALID_ARG and who in msg() and "null colours" in msg()
    assert track([a, b], [ca, cb], [40, 50], out=None) == ERR_INVALID_ARG and "null output" in msg()
    assert track([a, b], [ca, cb], [40, 50], pose=nan) == ERR_INVALID_ARG and "pose" in msg()
    assert track([a, b], [ca, cb], [40, 50], opt=binding.sdf_options(stride=3)) == ERR_INVALID_ARG and "stride" in msg()
    assert track([a, b], [ca, cb], [40, 50], copt=None) == ERR_INVALID_ARG and who in msg() and "colour options" in msg()
    assert track([a, b], [ca, cb], [40, 50], copt=binding.IcpSdfColorOptions(0.0, 0.0)) == ERR_INVALID_ARG and "weight" in msg()
    # a scan of 2^24 + 1 points is refused before anything is read or uploaded (the arrays are untouched zero pages)
    n = (1 << 24) + 1
    big, cbig = np.zeros((n, 3), f32), np.zeros((n, 4), np.uint8)
    assert track([a, big], [ca, cbig], [40, n]) == ERR_INVALID_ARG and who in msg() and "2^24" in msg()
    del big, cbig
    upload(ctx, K.model(hashed), color=False)
    assert track([a, b], [ca, cb], [40, 50]) == ERR_INVALID_ARG and who in msg() and "no colours" in msg()
    # and the context still works
    upload(ctx, CK.colored_model(hashed))
    ctx.set_source(pts, None, rgba)
    assert ctx.tsdf_align_cloud("source", K.START, color_weight=W)[2] == OK


@pytest.mark.parametrize("storage", STORAGES)
def test_outcome_on_the_flat_textured_wall(gpu_ctx_factory, storage):
    """Nine scans sliding 2 cm each along a flat textured wall (tests/sdf_cloud_color_outcome_fixture.py), through eth.track_tsdf: the
    photometric loop's worst translation error is at most twice what the restatement's loop recorded in the golden file, all eight
    alignments report ICP_OK, and the geometric loop on the same scans ends more than half the travel away."""
    from icp_amd import eth
    scans, cols, truth = OF.fixture()
    g = OF.golden()
    ctx = gpu_ctx_factory()
    kw = dict(voxel_size=OF.VOXEL, truncation=OF.TRUNCATION, origin=OF.ORIGIN, max_range=OF.OPTS["max_depth"], block_capacity=256)
    kw.update(dict(hashed=True) if storage == "hashed" else dict(hashed=False, dims=OF.DIMS))
    poses, recs, infos, status, ncs = eth.track_tsdf(ctx, scans, truth[0], colors=cols, color_weight=OF.COLOR_OPTIONS["weight"], color_huber=OF.COLOR_OPTIONS["huber"],
                                                     **kw, **OF.OPTIONS)
    ec = OF.translation_errors(poses, truth)
    gposes = eth.track_tsdf(ctx, scans, truth[0], colors=cols, **kw, **OF.OPTIONS)[0]
    eg = OF.translation_errors(gposes, truth)
    print("%s: photometric loop worst %.4f m (restatement %.4f m), geometric loop last %.4f m, of %.3f m of travel" %
          (storage, max(ec), g["colored_worst_translation_m"], eg[-1], OF.TRAVEL))
    print("  photometric per scan:", " ".join("%.4f" % e for e in ec))
    assert status == OK and len(recs) == 8 and all(r["status"] == OK for r in recs) and all(n > 0 for n in ncs)
    assert max(ec) <= 2 * g["colored_worst_translation_m"]
    assert eg[-1] > OF.TRAVEL / 2
