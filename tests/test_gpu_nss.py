"""Normal-space sampling (params.selection = 2, dev_nss.hpp) on the device against the numpy restatement tests/nss_restatement.py: buckets
and index lists exactly, teacher-forced iterations against the oracle on the device's own lists, the held form, every loop that takes a
selection, the paths that must stay untouched, refusals, and the incised plane the feature exists for."""
import functools
import numpy as np
import pytest

import nss_restatement as nss
import support as S
from support import bits, load

pytestmark = pytest.mark.gpu
f32 = np.float32
POSE_TOL = 1e-5
LONG_SEGMENT = 16384          # NSS_LONG (dev_nss.hpp): a bucket with more candidates than this is selected by several blocks of 4096


# this file's defaults: 4 iterations, normal-space sampling of half the points
configure = functools.partial(S.configure, n_iterations=4, selection=2, proba=0.5)


def factors_of(ctx):
    from icp_amd import binding
    return binding.schedule(ctx.params, ctx.n_src)


def check_lists(ctx, pts, nrm, proba, seed, grid, resample, label):
    """Every iteration's query set of the run that just ended, against the restatement; returns the lists."""
    ref = nss.run_lists(pts, nrm, factors_of(ctx), proba, seed, grid=grid, resample=resample)
    for i, r in enumerate(ref):
        dev = ctx.selection(i)
        assert np.array_equal(dev, r), (label, i, len(dev), len(r))
    return ref


def sized_cloud(bunny, n):
    """The first n bunny source points; past the bunny's 1054, jittered copies of it (seeded)."""
    pts, nrm = bunny["src_pts"], bunny["src_nrm"]
    if n <= len(pts):
        return pts[:n].copy(), nrm[:n].copy()
    rng = np.random.default_rng(n)
    reps = -(-n // len(pts))
    p = np.tile(pts, (reps, 1))[:n] + rng.normal(0, 1e-4, (n, 3)).astype(f32)
    q = np.tile(nrm, (reps, 1))[:n] + rng.normal(0, 0.05, (n, 3)).astype(f32)
    return p.astype(f32), q.astype(f32)


# ------------------------------------------------------------------------------------------------ buckets
def handmade_normals():
    s = np.float32(1e-40)                                    # subnormal
    rows = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
            (1, 1, 0), (-1, 1, 0), (1, -1, 0), (0, 1, 1), (0, -1, 1), (1, 0, 1), (-1, 0, -1),             # |x| = |y| ties and their kin
            (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1), (0.5, 0.5, 0.5),                             # |x| = |y| = |z|
            (1, 1, 0.3), (1, -1, 0.3), (2, 0.3, -2), (0.3, 3, 3),                                          # u or v exactly +-1
            (1, 0, 0.2), (1, 0.2, 0), (0.2, 0, -1),                                                        # u or v exactly 0
            (-0.0, 0, 1), (1, -0.0, -0.0), (-0.0, -1, 0.0), (-0.0, -0.0, -0.0),                            # -0.0 components (the last: zero normal)
            (s, 0, 0), (s, s, -s), (0, -3 * s, s), (2 * s, s, 0),                                          # subnormal normals
            (np.nan, 0, 1), (0, np.inf, 0), (1, 0, -np.inf), (0, 0, 0),                                    # NaN, Inf, zero
            (0.2, -0.33, 0.6), (1e-3, 1, 1e-3), (0.6, 0.2, 0.2000001), (-0.7, 0.7000001, 0.1)]
    return np.array(rows, dtype=f32)


@pytest.mark.parametrize("grid", [3, 5, 7])
def test_buckets_equal_restatement(gpu_ctx_factory, bunny, grid):
    ctx = gpu_ctx_factory()
    ctx.set_nss_options(grid, True)
    ctx.set_source(bunny["src_pts"], bunny["src_nrm"])
    assert np.array_equal(ctx.normal_buckets(), nss.buckets(bunny["src_pts"], bunny["src_nrm"], grid))
    nrm = handmade_normals()
    pts = np.arange(3 * (len(nrm) + 3), dtype=f32).reshape(-1, 3) * f32(0.01)
    nrm = np.concatenate([nrm, [[0, 0, 1], [0, 1, 0], [1, 0, 0]]]).astype(f32)
    pts[-3, 0] = np.nan; pts[-2, 1] = np.inf; pts[-1, 2] = -np.inf                                          # non-finite points
    ctx.set_source(pts, nrm)
    dev, ref = ctx.normal_buckets(), nss.buckets(pts, nrm, grid)
    assert np.array_equal(dev, ref), np.nonzero(dev != ref)[0]
    assert (ref[-3:] == nss.NONE).all() and (ref != nss.NONE).sum() >= len(nrm) - 10
    for other in (3, 5, 7):                                   # the cache follows the grid
        ctx.set_nss_options(other, True)
        assert np.array_equal(ctx.normal_buckets(), nss.buckets(pts, nrm, other))


# ------------------------------------------------------------------------------------------------ lists
@pytest.mark.parametrize("resample", [1, 0])
@pytest.mark.parametrize("multires", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1054, 4097])
def test_lists_equal_restatement(gpu_ctx_factory, bunny, n, multires, resample):
    ctx = gpu_ctx_factory()
    pts, nrm = sized_cloud(bunny, n)
    if n > 300:
        nrm[3] = 0; nrm[100, 2] = np.nan; pts[200, 0] = np.inf                                              # points without a bucket
    ctx.set_target(bunny["tgt_pts"], bunny["tgt_nrm"])
    ctx.set_source(pts, nrm)
    ctx.set_nss_options(5, bool(resample))
    for k, proba in enumerate((0.0, 1e-9, 0.25, 0.5, 1.0)):
        configure(ctx, knn_backend=k & 1, n_iterations=3, multires=multires, proba=proba, seed=11 + k)
        _, recs, rc = ctx.run(np.eye(4, dtype=f32), check=False)
        lists = check_lists(ctx, pts, nrm, proba, 11 + k, 5, bool(resample), (n, multires, resample, proba))
        assert [r["n_src"] for r in recs] == [len(l) for l in lists]
        if proba == 0.0:
            assert rc == 8 and all(r["status"] == 8 for r in recs)
        if proba == 1e-9:
            assert all(len(l) == 1 for l in lists)


def test_one_bucket_takes_the_multi_block_select(gpu_ctx_factory):
    """20 481 points whose normals all fall in one bucket: more than NSS_LONG = 16 384, so the full level's select runs in 6 blocks of
    4096 on the global histogram; the multires levels below (10 241, 5 121, ...) take the one-block select on the same data."""
    n = LONG_SEGMENT + 4097
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(0, 1, (n, 2)), rng.normal(0, 1e-3, (n, 1))], axis=1).astype(f32)
    nrm = (np.array([0, 0, 1]) + rng.normal(0, 0.02, (n, 3))).astype(f32)
    assert len(np.unique(nss.buckets(pts, nrm, 5))) == 1
    ctx = gpu_ctx_factory()
    ctx.set_target(pts[::4], nrm[::4]); ctx.set_source(pts, nrm)
    for multires, resample, proba in ((0, 1, 0.25), (1, 1, 0.9), (0, 0, 0.01), (1, 0, 0.5)):
        ctx.set_nss_options(5, bool(resample))
        configure(ctx, n_iterations=2, multires=multires, proba=proba, seed=5, max_distance=0.01)
        ctx.run(np.eye(4, dtype=f32), check=False)
        check_lists(ctx, pts, nrm, proba, 5, 5, bool(resample), (multires, resample, proba))
    # two long segments and a short one on one level: the long-segment list and its chunk offsets
    nrm2 = np.concatenate([(np.array([1, 0, 0]) + rng.normal(0, 0.02, (n, 3))).astype(f32), nrm, nrm]); nrm2[-500:] = [0, -1, 0]
    pts2 = np.tile(pts, (3, 1))
    ctx.set_source(pts2, nrm2)
    cnt = np.bincount(nss.buckets(pts2, nrm2, 5), minlength=150)
    assert (cnt > LONG_SEGMENT).sum() == 2 and ((cnt > 0) & (cnt <= LONG_SEGMENT)).sum() >= 1
    ctx.set_nss_options(5, True)
    configure(ctx, n_iterations=2, proba=0.6, seed=9, max_distance=0.01)
    ctx.run(np.eye(4, dtype=f32), check=False)
    check_lists(ctx, pts2, nrm2, 0.6, 9, 5, True, "two long")


def test_one_point_per_bucket(gpu_ctx_factory, bunny):
    g = 7
    c = (np.arange(g) + 0.5) * 2 / g - 1                       # cell centres
    u, v = [a.ravel() for a in np.meshgrid(c, c)]
    one = np.ones_like(u)
    nrm = np.concatenate([np.stack(t, axis=1) for t in ((one, u, v), (-one, u, v), (u, one, v), (u, -one, v), (u, v, one), (u, v, -one))]).astype(f32)
    assert len(np.unique(nss.buckets(np.zeros_like(nrm), nrm, g))) == 6 * g * g
    pts = np.resize(bunny["src_pts"], (len(nrm), 3)).astype(f32)
    ctx = gpu_ctx_factory()
    ctx.set_target(bunny["tgt_pts"], bunny["tgt_nrm"]); ctx.set_source(pts, nrm)
    ctx.set_nss_options(g, True)
    for proba in (0.5, 0.1, 1.0):                               # cap 1, every bucket capped, the excess rule decides
        configure(ctx, n_iterations=3, proba=proba, seed=2)
        ctx.run(np.eye(4, dtype=f32), check=False)
        lists = check_lists(ctx, pts, nrm, proba, 2, g, True, proba)
        assert len(lists[0]) == int(np.ceil(proba * 294))


def test_getter_on_random_sampling(gpu_ctx_factory, bunny):
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    for multires in (0, 1):
        configure(ctx, selection=1, n_iterations=3, multires=multires, proba=0.3, seed=77)
        _, recs, _ = ctx.run(np.eye(4, dtype=f32), check=False)
        for i, f in enumerate(factors_of(ctx)):
            base = nss.base_set(bunny["src_pts"], bunny["src_nrm"], f)
            keep = base[nss.select_hash(77, i, base) < np.uint32(int(float(f32(0.3)) * 4294967296.0))]
            assert np.array_equal(ctx.selection(i), keep.astype(np.int32)) and recs[i]["n_src"] == len(keep)


# ------------------------------------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("resample", [1, 0])
@pytest.mark.parametrize("multires", [0, 1])
@pytest.mark.parametrize("knn_backend", [0, 1])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_teacher_forced_parity(gpu_ctx_factory, orc, bunny, metric, knn_backend, multires, resample):
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    ctx.set_nss_options(5, bool(resample))
    configure(ctx, metric=metric, knn_backend=knn_backend, n_iterations=4, multires=multires, proba=0.5, seed=3)
    pose, recs, rc = ctx.run(np.eye(4, dtype=f32))
    lists = check_lists(ctx, bunny["src_pts"], bunny["src_nrm"], 0.5, 3, 5, bool(resample), "parity")
    prm = orc.make_params(metric=metric, n_iterations=1, max_distance=0.0003, solver_mode=1)
    before = np.eye(4, dtype=f32)
    for i, (L, r) in enumerate(zip(lists, recs)):
        po, _, nv, _, _ = orc.iterate(prm, bunny["src_pts"][L], bunny["src_nrm"][L], bunny["src_rgba"][L], bunny["tgt_pts"], bunny["tgt_nrm"], bunny["tgt_rgba"], before)
        assert r["status"] == 0 and r["n_src"] == len(L) and r["n_valid"] == nv, (i, r["n_src"], r["n_valid"], nv)
        assert np.abs(r["pose"] - po).max() < POSE_TOL, (i, np.abs(r["pose"] - po).max())
        before = r["pose"]
    assert np.array_equal(pose, recs[-1]["pose"])


def test_held_mode_takes_the_fast_form(gpu_ctx_factory, bunny):
    from icp_amd import binding
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c, backend in ((a, 1), (b, 0)):
        load(c, bunny)
        c.set_nss_options(5, False)
        configure(c, knn_backend=backend, n_iterations=6, multires=1, proba=0.5, seed=4)
    merged, fell_back = binding.C.c_int32(0), binding.C.c_int32(0)
    pa, ra, _ = a.run(np.eye(4, dtype=f32))
    pb, rb, _ = b.run(np.eye(4, dtype=f32))
    fac = factors_of(a)
    lists = check_lists(a, bunny["src_pts"], bunny["src_nrm"], 0.5, 4, 5, False, "held")
    for i in range(len(fac)):                                  # one list per level, its size constant
        first = fac.index(fac[i])
        assert ra[i]["n_src"] == ra[first]["n_src"] == len(lists[first]) and np.array_equal(a.selection(i), a.selection(first))
        assert ra[i]["n_src"] == rb[i]["n_src"] and ra[i]["n_valid"] == rb[i]["n_valid"]
        assert np.abs(ra[i]["pose"] - rb[i]["pose"]).max() < POSE_TOL, i
    assert a.lib.icp_debug_counters(a.h, binding.C.byref(merged), binding.C.byref(fell_back)) == 0
    assert merged.value == 1 and fell_back.value == 0         # the point-to-plane run went through the merged ring launches
    # the seeded search on the held level's cloud: a context whose source is source[L], launched pose by pose as the loop runs it,
    # against brute force at the last pose
    L = lists[-1]
    sub = dict(bunny, src_pts=bunny["src_pts"][L], src_nrm=bunny["src_nrm"][L], src_rgba=bunny["src_rgba"][L])
    c, d = gpu_ctx_factory(), gpu_ctx_factory()
    for x, backend in ((c, 1), (d, 0)):
        load(x, sub)
        configure(x, knn_backend=backend, selection=0, n_iterations=6)
    n1 = fac.count(1)
    poses = [ra[len(fac) - n1 - 1 + k]["pose"] if len(fac) - n1 - 1 + k >= 0 else np.eye(4, dtype=f32) for k in range(n1)]      # the pose before each full-level iteration
    ms, _ = c.match_seeded(poses)
    mb, _, _ = d.correspond(poses[-1])
    assert np.array_equal(ms["idx"], mb["idx"]) and np.array_equal(bits(ms["weight"]), bits(mb["weight"]))


# ------------------------------------------------------------------------------------------------ every loop
def test_multistart_follows_icp_run(gpu_ctx_factory, bunny):
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    rng = np.random.default_rng(1)
    starts = [np.eye(4, dtype=f32)]
    for _ in range(2):
        T = np.eye(4, dtype=f32); T[:3, 3] = rng.normal(0, 0.002, 3); starts.append(T)
    for resample in (True, False):
        ctx.set_nss_options(5, resample)
        configure(ctx, n_iterations=4, multires=1, proba=0.5, seed=6)
        res, stats, _ = ctx.run_multistart(starts, max_stats=16)
        M = [len(ctx.selection(i)) for i in range(len(stats[0]))]
        for k, T in enumerate(starts):
            pose, recs, rc = ctx.run(T, check=False)
            assert res[k]["status"] == rc == 0 and np.array_equal(bits(res[k]["pose"]), bits(pose)), (resample, k)
            assert [r["n_src"] for r in recs] == M == [s["n_src"] for s in stats[k]]
            for x, y in zip(stats[k], recs):
                assert np.array_equal(bits(x["pose"]), bits(y["pose"])) and x["n_valid"] == y["n_valid"]


def test_batch_run_equals_per_pair_runs(gpu_ctx_factory, bunny):
    from icp_amd import binding
    other = dict(bunny, src_pts=bunny["src_pts"][::-1].copy(), src_nrm=bunny["src_nrm"][::-1].copy(), src_rgba=bunny["src_rgba"][::-1].copy())
    pairs = [bunny, other, bunny]
    ctxs = [gpu_ctx_factory(), gpu_ctx_factory()]
    ref = gpu_ctx_factory()
    for c in ctxs + [ref]:
        c.set_nss_options(3, False)
        configure(c, n_iterations=4, proba=0.25, seed=8)
    poses, status, rc = binding.batch_run(ctxs, pairs)
    assert rc == 0
    for i, d in enumerate(pairs):
        load(ref, d)
        pose, recs, st = ref.run(np.eye(4, dtype=f32), check=False)
        assert st == status[i] == 0 and recs[0]["n_src"] == 264
        assert np.array_equal(bits(binding.pose_to_c(pose)), poses[i].view(np.uint32)), i


def test_track_depth_frames_equals_frame_by_frame(gpu_ctx_factory):
    from icp_amd import binding, synth
    W, H = 160, 120
    K = np.array([[525.0 / 4, 0, 319.5 / 4], [0, 525.0 / 4, 239.5 / 4], [0, 0, 1]], f32)
    depth, rgbx = [], []
    for k in range(3):
        pts, _, rgba = synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), W, H, 0x7A11 + k)
        depth.append(pts[:, 2].reshape(H, W).copy()); rgbx.append(rgba)
    depth, rgbx = np.stack(depth), np.stack(rgbx)
    cam = binding.depth_camera(K, W, H)
    to, so = binding.depth_options(False, 1), binding.depth_options(False, 2)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.set_nss_options(5, True)
        configure(c, n_iterations=5, proba=0.2, seed=12, max_distance=0.1)
    _, recs, rc = a.track_depth_frames(depth, rgbx, cam, to, so)
    b.set_target_depth(depth[0], rgbx[0], cam, to)
    pose = np.eye(4, dtype=f32)
    for k in range(1, 3):
        b.set_source_depth(depth[k], rgbx[k], cam, so)
        pose, its, st = b.run(pose, check=False)
        assert recs[k - 1]["status"] == st == 0
        assert np.array_equal(bits(recs[k - 1]["pose"]), bits(pose)), k
        M = nss.sample_size(0.2, int((b.normal_buckets() != nss.NONE).sum()))
        assert M > 0 and all(r["n_src"] == M for r in its)
    for i in range(5):                                         # the tracker's last frame and the last run by hand made the same draws
        assert np.array_equal(a.selection(i), b.selection(i))


@pytest.mark.parametrize("form", ["gicp", "colored", "robust", "lm"])
@pytest.mark.parametrize("resample", [1, 0])
def test_other_metrics_and_modes(gpu_ctx_factory, bunny, form, resample):
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    ctx.set_nss_options(5, bool(resample))
    configure(ctx, metric={"gicp": 3, "colored": 4}.get(form, 1), n_iterations=4, proba=0.25, seed=21, knn_backend=1)
    if form == "robust":
        ctx.set_robust_options("huber", overlap=0.8)
    if form == "lm":
        ctx.set_optimizer(True)
    if form == "gicp":
        ctx.set_gicp_options(1e-3, 10)
    if form == "colored":
        ctx.set_colored_options(0.968, 10)
    runs = [ctx.run(np.eye(4, dtype=f32), check=False) for _ in range(2)]
    (p0, r0, s0), (p1, r1, s1) = runs
    assert s0 == s1 == 0 and np.array_equal(bits(p0), bits(p1))
    for x, y in zip(r0, r1):
        assert x["status"] == 0 and x["n_src"] == y["n_src"] == 264 and x["n_valid"] == y["n_valid"] and np.array_equal(bits(x["pose"]), bits(y["pose"]))
    check_lists(ctx, bunny["src_pts"], bunny["src_nrm"], 0.25, 21, 5, bool(resample), form)


# ------------------------------------------------------------------------------------------------ untouched paths, refusals
@pytest.mark.parametrize("knn_backend", [0, 1])
@pytest.mark.parametrize("selection", [0, 1])
def test_selection_0_and_1_ignore_the_options(gpu_ctx_factory, bunny, selection, knn_backend):
    out = []
    for opts in (None, (7, False)):
        ctx = gpu_ctx_factory()
        load(ctx, bunny)
        if opts:
            ctx.set_nss_options(*opts)
        configure(ctx, selection=selection, knn_backend=knn_backend, n_iterations=5, multires=1, proba=0.5, seed=5)
        out.append(ctx.run(np.eye(4, dtype=f32)))
    (pa, ra, _), (pb, rb, _) = out
    assert np.array_equal(bits(pa), bits(pb)) and len(ra) == len(rb)
    for x, y in zip(ra, rb):
        assert (x["n_src"], x["n_valid"], x["status"]) == (y["n_src"], y["n_valid"], y["status"]) and np.array_equal(bits(x["pose"]), bits(y["pose"]))


def test_refusals(gpu_ctx_factory, bunny):
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    for grid, resample in ((4, 1), (0, 1), (9, 1), (5, 2), (5, -1)):
        with pytest.raises(binding.IcpError) as ei:
            ctx.set_nss_options(grid, resample)
        assert ei.value.code == 1 and "grid" in str(ei.value)
    o = ctx.nss_options()
    assert (o.grid, o.resample) == (5, 1)
    ctx.set_nss_options(7, False)
    o = ctx.nss_options()
    assert (o.grid, o.resample) == (7, 0)
    assert ctx.lib.icp_set_nss_options(ctx.h, None) == 0      # NULL = defaults
    o = ctx.nss_options()
    assert (o.grid, o.resample) == (5, 1)
    ctx.params.selection = 3
    with pytest.raises(binding.IcpError) as ei:
        ctx.push_params()
    assert ei.value.code == 1
    ctx.set_target(bunny["tgt_pts"], bunny["tgt_nrm"])
    ctx.set_source(bunny["src_pts"])                          # no normals
    configure(ctx)
    _, _, rc = ctx.run(np.eye(4, dtype=f32), check=False)
    assert rc == 1 and "normals" in ctx.lib.icp_last_error(ctx.h).decode()
    with pytest.raises(binding.IcpError):
        ctx.normal_buckets()
    ctx.set_source(bunny["src_pts"], bunny["src_nrm"])
    with pytest.raises(binding.IcpError):                     # no run yet on this source
        ctx.selection(0)
    ctx.run(np.eye(4, dtype=f32))
    assert len(ctx.selection(3)) == 527
    for i in (-1, 4):
        with pytest.raises(binding.IcpError):
            ctx.selection(i)
    configure(ctx, selection=0)
    ctx.run(np.eye(4, dtype=f32))
    with pytest.raises(binding.IcpError):                     # that run had selection 0
        ctx.selection(0)


# ------------------------------------------------------------------------------------------------ what it is for
def test_incised_plane_beats_random_sampling(gpu_ctx_factory):
    """The incised plane (synth.incised_plane: 25 600 points, two V-grooves), point-to-plane, proba 0.02, 30 iterations, seeds 0..3: the
    median final translation error (the displacement of the square's centre between the estimated and the true pose) under normal-space
    sampling is below the median under RANDOM_SAMPLING on the same context.  Measured on an MI355X: see DESIGN.md 6i."""
    from icp_amd import synth
    d = synth.incised_plane()
    ctx = gpu_ctx_factory()
    load(ctx, d, colors=False)
    ctx.set_nss_options(5, True)
    c4 = np.append(d["centre"], 1.0)
    err = {}
    for selection in (1, 2):
        err[selection] = []
        for seed in range(4):
            configure(ctx, selection=selection, n_iterations=30, proba=0.02, seed=seed, max_distance=0.0025)
            pose, recs, rc = ctx.run(np.eye(4, dtype=f32), check=False)
            err[selection].append(float(np.linalg.norm((pose.astype(np.float64) - d["truth"]) @ c4)))
        print("incised plane, selection %d: translation errors [mm] %s" % (selection, ["%.3f" % (1e3 * e) for e in err[selection]]))
    assert np.median(err[2]) < np.median(err[1]), err
