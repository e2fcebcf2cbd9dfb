"""Free space carved by the cloud fuses on the device (icp_set_tsdf_carve_options) against the numpy restatement
of the contract (tests/tsdf_carve_restatement.py), BIT FOR BIT: block coordinates, tsdf, weight, every field of the fuse info and of the
carve stats, on both storages.  The crafted cases of tests/tsdf_carve_cases.py (sizes around a wave and a work-group, the dyadic rays
counted by hand, the join of carve walk and band, hashed residency, the dense box, exact ones, the mixed voxel, lanes for the wave
combining); the off state; the order of the points; dense against hashed; depth frames, colours, evict and insert around a carved
cloud; the tracking loop; the refusals; and the outcome: a box that stood in four scans and left, carved out of the model and the mesh."""
import ctypes

import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_restatement as HR
import sdf_cloud_cases as SK
import sdf_cloud_restatement as SC
import support as S
import tsdf_carve_cases as K
import tsdf_carve_outcome_fixture as OF
import tsdf_carve_restatement as CV
import tsdf_cloud_outcome_fixture as CF
import tsdf_cloud_restatement as CR
from support import same_bits, pose_of
from tsdf_cloud_cases import cloud, OPTS, TILTED, EYE

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, ERR_INVALID_ARG = 0, 1
INF = float("inf")


def create(ctx, c):
    if c["dims"] is None:
        ctx.tsdf_create_hashed(block_capacity=c["capacity"], **c["opts"])
        if c["alloc"] is not None:
            ctx.tsdf_allocate_blocks(c["alloc"])
    else:
        ctx.tsdf_create(dims=c["dims"], **c["opts"])


def fuse(ctx, pts, pose, origin=None, which="source"):
    (ctx.set_source if which == "source" else ctx.set_target)(pts)
    info = ctx.tsdf_integrate_cloud(which, pose=pose, sensor_origin=origin)
    st = ctx.tsdf_carve_stats()
    return info, dict(n_steps=st["n_steps"], n_carved=st["n_carved"]), st["n_carved_total"]


def run(ctx, c, carve=None, order=None):
    """The case on the device under `carve` (None: its own; False: the options are never touched).  -> (infos, stats)"""
    create(ctx, c)
    if carve is not False:
        ctx.set_tsdf_carve(**(c["carve"] if carve is None else carve))
    infos, stats, total = [], [], 0
    for pts, pose, origin, which in c["steps"]:
        p = K.device_cloud(c, pts)
        info, st, tot = fuse(ctx, p if order is None else order(p), pose, origin, which)
        total += st["n_carved"]
        assert tot == total
        infos.append(info); stats.append(st)
    return infos, stats


def state(ctx, c):
    return ctx.tsdf_blocks()[1:] if c["dims"] is None else ctx.tsdf_volume()


def same_state(a, b):
    return len(a) == len(b) and all(same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a, b))


def volume_equals(ctx, vol, what):
    if isinstance(vol, HR.HVolume):
        S.tsdf_blocks_equal_restatement(ctx, vol, what)
    else:
        T, W = ctx.tsdf_volume()
        assert same_bits(T, vol.tsdf) and same_bits(W, vol.weight), what


@pytest.mark.parametrize("name", list(K.CASES))
def test_device_equals_restatement(gpu_ctx_factory, name):
    """Every crafted case: infos, carve stats and the volume, bit for bit; the figures counted by hand."""
    c = K.CASES[name]
    winfos, wstats, vol = K.reference(name)
    ctx = gpu_ctx_factory()
    infos, stats = run(ctx, c)
    print("%s: %s %s" % (name, infos[-1], stats[-1]))
    assert infos == winfos and stats == wstats, (name, infos, winfos, stats, wstats)
    volume_equals(ctx, vol, name)
    for key, v in c["expect"].items():
        assert dict(infos[-1], **stats[-1])[key] == v, (name, key)
    if c["alloc"] is not None and not name.startswith("residency/beyond"):
        # carving allocates nothing: the blocks are the allocated ones plus the touch's set
        touched = CV.walk(K.new_volume(c), c["steps"][0][0], c["steps"][0][1], c["steps"][0][2])["touched"]
        assert infos[0]["n_blocks"] == len(set(map(tuple, c["alloc"].tolist())) | set(map(tuple, touched.tolist())))
    if name in ("exact_ones", "mixed_voxel"):
        T, W = ctx.tsdf_volume()
        row = lambda a: a[12, 2, 2:22]                 # the ray's voxels: the sensor on (2, 2, 12), along +x
        if name == "exact_ones":
            assert (row(T)[1:13] == f32(1.0)).all() and (row(W)[1:13] == f32(1.0)).all() and row(W)[0] == 0
        else:
            # voxels 1 .. 5: both rays f = 1; 8: 0 and 1; 11: -1 and 1; 12: carved by PASS alone
            assert (row(T)[1:6] == f32(1.0)).all() and row(T)[8] == f32(0.5) and row(T)[11] == f32(0.0) and row(T)[12] == f32(1.0) and (row(W)[1:20] == 1).all()
    if name.startswith("lanes/pile"):
        assert stats[0]["n_carved"] % K.CC.PILE_N == 0 and stats[0]["n_carved"] > 0


@pytest.mark.parametrize("name", ["n257/hashed", "n257/dense", "lanes/runs/hashed"])
def test_off_state(gpu_ctx_factory, name):
    """With distance 0, and after on-then-off, the call equals the same call on a fresh context that never had the option set -- and
    tsdf_cloud_restatement, the contract of the call without carving."""
    c = K.CASES[name]
    never, zero, toggled = gpu_ctx_factory(), gpu_ctx_factory(), gpu_ctx_factory()
    a = run(never, c, carve=False)
    b = run(zero, c, carve=dict(distance=0.0, min_range=0.7))
    run(toggled, c)                                    # carved once ...
    toggled.set_tsdf_carve(0.0)
    d = run(toggled, c, carve=False)                   # ... then a new volume with the option off again
    assert toggled.tsdf_carve_options().distance == 0.0 and toggled.tsdf_carve_stats() == dict(n_steps=0, n_carved=0, n_carved_total=0)
    assert a == b == d and all(st == dict(n_steps=0, n_carved=0) for st in a[1])
    assert same_state(state(never, c), state(zero, c)) and same_state(state(never, c), state(toggled, c))
    vol = K.new_volume(c)
    assert a[0] == [CR.integrate(vol, p, T, e) for p, T, e, _ in c["steps"]]
    volume_equals(never, vol, name)


@pytest.mark.parametrize("name", ["n3000/hashed", "n3000/dense"])
def test_the_timing_hook_fuses_twice(gpu_ctx_factory, name):
    """icp_debug_tsdf_carve_time (tools/time_tsdf_carve.py) is the call and one more touch, carving accumulate and fold: the volume and
    the stats are the restatement's after two fuses; refused while carving is off."""
    from icp_amd import binding
    c = K.CASES[name]
    pts, pose, origin, _ = c["steps"][0]
    vol = K.new_volume(c)
    want = [CV.integrate(vol, pts, pose, origin, **c["carve"]) for _ in range(2)]
    ctx = gpu_ctx_factory()
    e = None if origin is None else np.asarray(origin, f32)
    create(ctx, c)
    ctx.set_tsdf_carve(**c["carve"])
    ctx.set_source(pts)
    ms = (ctypes.c_float * 3)()
    assert ctx.lib.icp_debug_tsdf_carve_time(ctx.h, 1, binding._ptr(binding.pose_to_c(pose)), binding._ptr(e), ms) == OK
    st = ctx.tsdf_carve_stats()
    assert (st["n_steps"], st["n_carved"], st["n_carved_total"]) == (want[1][1]["n_steps"], want[1][1]["n_carved"], want[0][1]["n_carved"] + want[1][1]["n_carved"])
    volume_equals(ctx, vol, name)
    ctx.set_tsdf_carve(0.0)
    assert ctx.lib.icp_debug_tsdf_carve_time(ctx.h, 1, binding._ptr(binding.pose_to_c(pose)), binding._ptr(e), ms) == ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["n3000/hashed", "n3000/dense", "lanes/runs/dense"])
def test_order_of_the_points(gpu_ctx_factory, name):
    """Reversed and shuffled uploads give identical volumes, infos and stats."""
    c = K.CASES[name]
    ctx = gpu_ctx_factory()
    perm = np.random.default_rng(5)
    got = []
    for order in (None, lambda p: p[::-1].copy(), lambda p: p[perm.permutation(len(p))]):
        res = run(ctx, c, order=order)
        got.append((res, state(ctx, c)))
    for res, st in got[1:]:
        assert res == got[0][0] and same_state(st, got[0][1])
    assert got[0][0][1][0]["n_carved"] > 0


def test_dense_against_hashed(gpu_ctx_factory):
    """Blocks allocated over a box: at every voxel of the hashed volume's resident blocks inside the box the dense volume holds the same
    bits -- carving on a hashed volume is carving on a dense one, restricted to the storage that exists."""
    from icp_amd import binding
    opts = dict(OPTS, origin=(-1.8, -1.8, -0.5))
    dims = (48, 48, 48)
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    box = K.block_box((0, 0, 0), (5, 5, 5))
    h.tsdf_create_hashed(block_capacity=256, **opts); h.tsdf_allocate_blocks(box)
    d.tsdf_create(dims=dims, **opts)
    hv = HR.HVolume(**opts); hv.allocate(box); dv = CR.DVolume(dims, **opts)
    for ctx in (h, d):
        ctx.set_tsdf_carve(INF, 0.2)
    for k, pose in enumerate([EYE, TILTED, pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05))]):
        pts = cloud(1500, seed=20 + k)
        ih, idn = fuse(h, pts, pose), fuse(d, pts, pose)
        assert ih[:2] == CV.integrate(hv, pts, pose, None, INF, 0.2) and idn[:2] == CV.integrate(dv, pts, pose, None, INF, 0.2)
        assert ih[1]["n_carved"] > 0 and idn[1]["n_carved"] > 0
    _, coords, t, w = h.tsdf_blocks()
    inside = ((coords >= 0) & (coords <= 5)).all(1)
    assert inside.sum() == 216 and len(coords) > 216          # the touch went beyond the box: those blocks have no dense counterpart
    T, Wt = binding.tsdf_blocks_to_dense(coords[inside], t[inside], w[inside], (0, 0, 0), dims)
    Td, Wd = d.tsdf_volume()
    assert same_bits(T, Td) and same_bits(Wt, Wd) and Wd.max() == 3
    volume_equals(h, hv, "hashed"); volume_equals(d, dv, "dense")


def test_depth_frames_colours_evict_and_insert(gpu_ctx_factory):
    """A depth frame, a carved cloud, a depth frame on one volume; a coloured volume's colours unchanged; and after an evict and an insert
    the carved fuse equals that on a fresh volume uploaded with the same blocks."""
    ctx = gpu_ctx_factory()
    cam, rcam = HC.camera()
    ctx.tsdf_create_hashed(color=True, **HC.STRADDLE)
    hv = HR.HVolume(**HC.STRADDLE)
    ctx.set_tsdf_carve(INF, 0.1)
    rgbx = np.random.default_rng(3).integers(0, 256, (HC.H, HC.W, 4), dtype=np.uint8)
    n, nc = ctx.tsdf_integrate(HC.crafted_frame(), cam, HC.TILTED, rgbx=rgbx)
    assert n == HR.integrate(hv, HC.crafted_frame(), rcam, HC.TILTED) and nc > 0
    _, c0, t0, w0, rgb0, cw0 = ctx.tsdf_blocks(colors=True)
    near = (cloud(2000, seed=32) * f32(0.7)).astype(f32)
    got = fuse(ctx, near, HC.POSES[2])
    assert got[:2] == CV.integrate(hv, near, HC.POSES[2], None, INF, 0.1) and got[1]["n_carved"] > 0      # the frame's blocks lie in front of the cloud's band
    S.tsdf_blocks_equal_restatement(ctx, hv, "cloud after frame")
    _, c1, t1, w1, rgb1, cw1 = ctx.tsdf_blocks(colors=True)
    key = lambda c: (c[:, 2].astype(np.int64) << 42) + (c[:, 1].astype(np.int64) << 21) + c[:, 0]
    at = np.searchsorted(key(c1), key(c0))
    assert np.array_equal(c1[at], c0) and same_bits(rgb1[at], rgb0) and same_bits(cw1[at], cw0) and cw0.max() > 0
    new = np.ones(len(c1), bool); new[at] = False
    assert not rgb1[new].any() and not cw1[new].any()
    assert ctx.tsdf_integrate(HC.frames()[1], cam, EYE) == HR.integrate(hv, HC.frames()[1], rcam, EYE)
    S.tsdf_blocks_equal_restatement(ctx, hv, "frame after cloud after frame")
    # evict and insert
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    first, second = cloud(2000, seed=41), cloud(2000, seed=42)
    a.tsdf_create_hashed(block_capacity=16, **OPTS)
    a.tsdf_allocate_blocks(K.WALL_BLOCKS)
    hv = HR.HVolume(**OPTS); hv.allocate(K.WALL_BLOCKS)
    a.set_tsdf_carve(INF); b.set_tsdf_carve(INF)
    assert fuse(a, first, TILTED)[:2] == CV.integrate(hv, first, TILTED, None, INF)
    einfo, ec, et, ew = a.tsdf_evict_blocks((0.0, 0.0, 2.0), 1.5)
    assert 0 < einfo["n_evicted"] < len(hv.blocks)
    a.tsdf_insert_blocks(ec, et, ew)
    _, coords, t, w = a.tsdf_blocks()
    b.tsdf_create_hashed(block_capacity=1 << 10, **OPTS)
    b.tsdf_upload_blocks(coords, t, w)
    pose = pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05))
    ia, ib = fuse(a, second, pose), fuse(b, second, pose)
    assert ia[:2] == ib[:2] == CV.integrate(hv, second, pose, None, INF)
    assert same_state(a.tsdf_blocks()[1:], b.tsdf_blocks()[1:])
    S.tsdf_blocks_equal_restatement(a, hv, "after evict and insert")


@pytest.mark.parametrize("storage", ["dense", "hashed"])
def test_the_loop(gpu_ctx_factory, storage):
    """icp_track_scans_sdf with carving on, as tests/test_gpu_sdf_cloud.py checks it without: every record within POSE_TOL per step of the
    restatement's alignment from the DEVICE's previous pose, then the restatement's model led along the device's poses -- every fuse
    carving -- and compared bit for bit, infos and carve stats included; eth.track_tsdf(carve=...) is the same call and puts the options
    back."""
    from icp_amd import eth
    ctx = gpu_ctx_factory()
    scans = SK.track_scans()
    carve = dict(distance=1.5, min_range=0.3)
    vol = SC.HVolume(**SK.OPTS) if storage == "hashed" else SC.Volume(SK.DIMS, **SK.OPTS)
    kw = dict(voxel_size=SK.OPTS["voxel_size"], truncation=SK.OPTS["truncation"], origin=SK.OPTS["origin"], max_range=SK.OPTS["max_depth"], block_capacity=64)
    kw.update(dict(hashed=True) if storage == "hashed" else dict(hashed=False, dims=SK.DIMS))
    poses, recs, infos, status = eth.track_tsdf(ctx, scans, SK.TRACK_POSES[0], carve=carve, n_iterations=10, **kw)
    assert ctx.tsdf_carve_options().distance == 0.0 and status == OK
    first = CV.integrate(vol, scans[0], SK.TRACK_POSES[0], None, **carve)
    assert infos[0] == first[0] and same_bits(poses[0], np.asarray(SK.TRACK_POSES[0], f32))
    total = first[1]["n_carved"]
    for k in range(1, len(scans)):
        rpose, rrec, _ = SC.align(vol, scans[k], poses[k - 1], n_iterations=10)
        r = recs[k - 1]
        diff = float(np.abs(r["pose"] - rpose).max())
        print("%s, scan %d: %d iterations (restatement %d), %d valid of %d, |pose - restatement| = %.3g" % (storage, k, r["iterations"], rrec["iterations"], r["n_valid_first"], r["n_depth"], diff))
        assert r["status"] == rrec["status"] == OK and (r["n_depth"], r["n_valid_first"]) == (rrec["n_depth"], rrec["n_valid_first"])
        assert same_bits(r["pose"], poses[k]) and diff <= S.POSE_TOL * max(r["iterations"], rrec["iterations"])
        info, last = CV.integrate(vol, scans[k], poses[k], None, **carve)
        assert infos[k] == info and last["n_carved"] > 0
        total += last["n_carved"]
    volume_equals(ctx, vol, storage + " loop")
    # the restatement's own loop: where its poses agree with the device's bit for bit, so do model and infos
    rv = SC.HVolume(**SK.OPTS) if storage == "hashed" else SC.Volume(SK.DIMS, **SK.OPTS)
    rposes, rrecs, rinfos, rstatus, rstats = CV.track(rv, scans, SK.TRACK_POSES[0], n_iterations=10, **carve)
    assert rstatus == OK and all(float(np.abs(a - b).max()) <= S.POSE_TOL * 20 for a, b in zip(poses, rposes))
    if all(same_bits(a, b) for a, b in zip(poses, rposes)):
        volume_equals(ctx, rv, storage + " loop, the restatement's own track")
        assert infos == rinfos and rstats[-1] == last
    # the C call with the options set on the context: the stats are the last fuse's, the total the loop's
    ctx.set_tsdf_carve(**carve)
    if storage == "hashed":
        ctx.tsdf_create_hashed(block_capacity=64, **SK.OPTS)
    else:
        ctx.tsdf_create(dims=SK.DIMS, **SK.OPTS)
    out = ctx.track_scans_sdf(scans, SK.TRACK_POSES[0], n_iterations=10)
    assert all(same_bits(a, b) for a, b in zip(out[0], poses)) and out[2] == infos
    st = ctx.tsdf_carve_stats()
    assert st == dict(n_steps=15, n_carved=last["n_carved"], n_carved_total=total)
    volume_equals(ctx, vol, storage + " loop again")


def test_refusals_leave_volume_and_options_as_they_were(gpu_ctx_factory):
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    lib = ctx.lib
    p = binding.pose_to_c(TILTED)
    msg = lambda: lib.icp_last_error(ctx.h).decode()
    ctx.set_source(cloud(50))
    for hashed in (True, False):
        if hashed:
            ctx.tsdf_create_hashed(**OPTS); ctx.tsdf_allocate_blocks(K.WALL_BLOCKS)
        else:
            ctx.tsdf_create(dims=(40, 40, 40), **dict(OPTS, origin=(-1.8, -1.8, 0.0)))
        ctx.set_tsdf_carve(2.0, 0.25)
        assert ctx.tsdf_integrate_cloud("source", pose=TILTED)["n_updated"] > 0 and ctx.tsdf_carve_stats()["n_carved"] > 0
        get = lambda: ctx.tsdf_blocks() if hashed else ctx.tsdf_volume()
        before, stats = get(), ctx.tsdf_carve_stats()
        for bad in (binding.IcpTsdfCarveOptions(-1.0, 0.0), binding.IcpTsdfCarveOptions(np.nan, 0.0), binding.IcpTsdfCarveOptions(1.0, -0.5),
                    binding.IcpTsdfCarveOptions(1.0, INF), binding.IcpTsdfCarveOptions(1.0, np.nan)):
            assert lib.icp_set_tsdf_carve_options(ctx.h, ctypes.byref(bad)) == ERR_INVALID_ARG and "icp_set_tsdf_carve_options" in msg()
        o = ctx.tsdf_carve_options()
        assert (o.distance, o.min_range) == (2.0, 0.25) and ctx.tsdf_carve_stats() == stats
        bad = p.copy(); bad[13] = np.nan
        assert lib.icp_tsdf_integrate_cloud(ctx.h, 1, binding._ptr(bad), None, None) == ERR_INVALID_ARG
        assert lib.icp_tsdf_integrate_cloud(ctx.h, 2, binding._ptr(p), None, None) == ERR_INVALID_ARG
        assert lib.icp_tsdf_integrate_cloud(ctx.h, 0, binding._ptr(p), None, None) == 3          # no target
        after = get()
        if hashed:
            assert before[0] == after[0] and same_state(before[1:], after[1:])
        else:
            assert same_state(before, after)
        assert ctx.tsdf_carve_stats() == stats
    # J beyond the cap: a volume whose max_depth / voxel_size exceeds 65536, carved all the way
    far = dict(OPTS, voxel_size=0.001, truncation=0.004, max_depth=65.537)
    ctx.tsdf_create_hashed(**far)
    ctx.set_tsdf_carve(INF)
    info = binding.IcpTsdfCloudInfo()
    assert lib.icp_tsdf_integrate_cloud(ctx.h, 1, binding._ptr(p), None, ctypes.byref(info)) == ERR_INVALID_ARG and "65536" in msg() and "icp_tsdf_integrate_cloud" in msg()
    assert ctx.tsdf_blocks()[0]["n_blocks"] == 0 and info.n_points == 0 and ctx.tsdf_carve_options().distance == INF
    scan = np.ascontiguousarray(cloud(50)); xp = (ctypes.c_void_p * 1)(binding._ptr(scan)); cn = (ctypes.c_int32 * 1)(50)
    o = binding.sdf_options()
    assert lib.icp_track_scans_sdf(ctx.h, xp, cn, 1, ctypes.byref(o), binding._ptr(p.copy()), None, None) == ERR_INVALID_ARG and "65536" in msg()
    assert ctx.tsdf_blocks()[0]["n_blocks"] == 0
    ctx.set_tsdf_carve(65.5)                           # under the cap: accepted, and short rays do not idle through it
    j = CV.carve_steps(HR.HVolume(**far), 65.5)
    assert ctx.tsdf_integrate_cloud("source", pose=TILTED)["n_rays"] == 50 and ctx.tsdf_carve_stats()["n_steps"] == j and 65000 < j <= 65536
    # the options survive a reset, a new volume and new clouds
    ctx.set_tsdf_carve(1.25, 0.5)
    ctx.tsdf_reset(); ctx.tsdf_create_hashed(**OPTS); ctx.set_source(cloud(10)); ctx.set_target(cloud(10))
    o = ctx.tsdf_carve_options()
    assert (o.distance, o.min_range) == (1.25, 0.5)
    assert lib.icp_set_tsdf_carve_options(ctx.h, None) == OK and ctx.tsdf_carve_options().distance == 0.0


def test_outcome_box_carved_out_of_model_and_mesh(gpu_ctx_factory):
    """The twelve scans with a box in the first four: eth.fuse_scans(carve=...) equals the fixture's carved model bit for bit (whose
    conditions are asserted on the CPU), its mesh has no vertex inside the box shrunk by one voxel, and without carving it has some."""
    from icp_amd import eth
    clouds, poses, _ = OF.scans()
    ctx = gpu_ctx_factory()
    kw = dict(voxel_size=CF.VOXEL, truncation=CF.TRUNCATION, origin=CF.ORIGIN, max_range=CF.MAX_RANGE, block_capacity=256)
    counts = {}
    for carved in (False, True):
        vol, want, _ = OF.model(carved)
        infos = eth.fuse_scans(ctx, clouds, poses, carve=OF.CARVE if carved else None, **kw)
        assert infos == want and ctx.tsdf_carve_options().distance == 0.0
        S.tsdf_blocks_equal_restatement(ctx, vol, "outcome, carved %s" % carved)
        v, _, t = ctx.tsdf_mesh_hashed()
        counts[carved] = OF.vertices_in_box(v)
        print("carved %s: %d vertices, %d triangles, %d vertices inside the shrunk box" % (carved, len(v), len(t), counts[carved]))
    assert counts[True] == 0 and counts[False] > 0
