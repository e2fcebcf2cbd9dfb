"""Reciprocal (mutual nearest-neighbour) rejection (icp_set_reciprocal_options) on the device against the numpy restatement
tests/reciprocal_restatement.py: teacher-forced iterations on the context's own option-off records, the smallest shapes that can go wrong,
option off is untouched, free-running runs with every way of choosing the query set, the batch and tracking entry points, refusals and
isolation, and the partial-overlap outcome the feature exists for.

Teacher-forced means: at a given pose, icp_match gives the raw matches and icp_correspond with the option off the records after weighting
and rejection (the base records).  Weighting and rejection act on every pair by itself, so with the option on the records must be the base
records with {-1, 0} wherever the restatement, applied to the raw matches, finds a judged pair not mutual -- bit for bit -- and the stats
must be the restatement's counts."""
import ctypes as C
import numpy as np
import pytest

import gicp_restatement as G
import reciprocal_restatement as RC
import robust_restatement as R
from conftest import pose_error
from support import configure, load, u32

pytestmark = pytest.mark.gpu
f32 = np.float32


def expected(base, raw, pose, src, tgt, nearest=None):
    """The records and stats the option must produce at `pose`, from the raw matches and the base records."""
    r = RC.reciprocal(raw, pose, src, tgt, nearest=nearest)
    out = np.array(base, dtype=RC.MATCH_DTYPE)
    drop = r["judged"] & ~r["mutual"]
    out["idx"][drop] = -1; out["weight"][drop] = 0.0
    return out, r["stats"], r


def teacher_forced(ctx, d, pose, label, nearest=None, strict_nv=True):
    ctx.set_reciprocal_options(False)
    raw, d2_off = ctx.match(pose)
    base, _, nv_off = ctx.correspond(pose)
    assert ctx.reciprocal_stats() == []
    exp, stats, r = expected(base, raw, pose, d["src_pts"], d["tgt_pts"], nearest)
    ctx.set_reciprocal_options(True)
    recs, sums, nv = ctx.correspond(pose)
    st = ctx.reciprocal_stats()
    ctx.set_reciprocal_options(False)
    print("%s: matched %d, mutual %d (kept %.3f), n_valid %d -> %d" % (label, stats["n_matched"], stats["n_mutual"],
                                                                     stats["n_mutual"] / max(stats["n_matched"], 1), nv_off, nv))
    assert st == [stats], (label, st, stats)
    assert np.array_equal(recs["idx"], exp["idx"]), (label, int((recs["idx"] != exp["idx"]).sum()))
    assert np.array_equal(u32(recs["weight"]), u32(exp["weight"])), label
    assert nv <= stats["n_mutual"] and nv == int(sums[0])
    if strict_nv:
        assert nv == int((exp["idx"] >= 0).sum()), label
    return stats


@pytest.fixture(scope="module")
def depth_pair():
    from icp_amd import synth
    return synth.compact_rgbd_pair()


BUNNY_POSES = [((0, 0, 0), (0, 0, 0)), ((0.01, -0.015, 0.02), (0.002, -0.003, 0.001)), ((-0.05, 0.04, 0.03), (-0.004, 0.002, 0.005))]


@pytest.mark.parametrize("metric", [0, 1, 2, 3, 4])
def test_teacher_forced_metrics(gpu_ctx_factory, bunny, depth_pair, metric):
    from icp_amd import synth
    ctx = gpu_ctx_factory()
    configure(ctx, metric=metric, weighting=1 if metric == 1 else 0, rejection=1)
    ctx.set_gicp_options(1e-3, 10)
    load(ctx, bunny)
    for k, (a, t) in enumerate(BUNNY_POSES):
        s = teacher_forced(ctx, bunny, synth.make_pose(a, t).astype(f32), "bunny metric %d pose %d" % (metric, k), strict_nv=metric < 3)
        assert 0 < s["n_mutual"] < s["n_matched"]
    configure(ctx, metric=metric, rejection=1, max_distance=0.01)
    load(ctx, depth_pair)
    s = teacher_forced(ctx, depth_pair, np.eye(4, dtype=f32), "depth/8 metric %d" % metric, strict_nv=metric < 3)
    assert 0 < s["n_mutual"] < s["n_matched"]


def test_teacher_forced_brute_backend_and_projective(gpu_ctx_factory, bunny, depth_pair):
    from icp_amd import synth
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, knn_backend=0)
    load(ctx, bunny, colors=False)
    teacher_forced(ctx, bunny, synth.make_pose(*BUNNY_POSES[1]).astype(f32), "bunny brute force")
    configure(ctx, metric=0, knn_backend=0, max_distance=0.01)
    load(ctx, depth_pair, colors=False)
    teacher_forced(ctx, depth_pair, np.eye(4, dtype=f32), "depth/8 brute force")
    o = depth_pair["organised"]; K = depth_pair["K"]
    d = dict(src_pts=o["src_pts"], src_nrm=o["src_nrm"], tgt_pts=o["tgt_pts"], tgt_nrm=o["tgt_nrm"])
    configure(ctx, metric=1, matching=1, max_distance=0.1)
    p = ctx.params
    p.fx, p.fy, p.cx, p.cy, p.width, p.height = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), 80, 60
    ctx.push_params()
    load(ctx, d, colors=False)
    s = teacher_forced(ctx, d, np.eye(4, dtype=f32), "projective", strict_nv=False)
    assert s["n_matched"] > 1000


def test_teacher_forced_fullsize(gpu_ctx_factory, orc):
    """The 370 k pair once at the identity.  370 k x 370 k distances are out of numpy's reach in seconds: here the restatement takes its
    argmin from the oracle's exact kd-tree over the source (bit-identical to the oracle's brute-force knn3, its own tests pin that), and the
    brute force still decides a sample of the pairs."""
    from icp_amd import synth
    d = synth.eth_like_pair(0)
    assert len(d["src_pts"]) == 370488
    src = np.asarray(d["src_pts"], f32)
    fin = np.flatnonzero(np.isfinite(src).all(1))
    tree = orc.KdTree(src[fin])

    def nearest(q):
        m, _ = tree.query(q, 3.0e38)
        return np.where(m["idx"] >= 0, fin[np.maximum(m["idx"], 0)], -1)
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, max_distance=10.0)
    load(ctx, d, colors=False)
    eye = np.eye(4, dtype=f32)
    s = teacher_forced(ctx, d, eye, "370k", nearest=nearest, strict_nv=False)
    assert s["n_matched"] > 300000 and 0 < s["n_mutual"] < s["n_matched"]
    raw, _ = ctx.match(eye)
    pick = np.flatnonzero(raw["idx"] >= 0)[::1499]
    q = RC.to_source_frame(eye, np.asarray(d["tgt_pts"], f32)[raw["idx"][pick]])
    assert np.array_equal(RC.mutual(q, pick, src), RC.mutual_by_nearest(q, pick, src, nearest))


def cloud_case(rng, n_src, n_tgt=1000):
    tgt = rng.uniform(0, 1, (n_tgt, 3)).astype(f32)
    src = (tgt[rng.permutation(n_tgt)[:n_src] % n_tgt] + rng.normal(0, 0.02, (n_src, 3))).astype(f32)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(f32)
    return dict(src_pts=src, src_nrm=unit(rng.normal(0, 1, (n_src, 3))), tgt_pts=tgt, tgt_nrm=unit(rng.normal(0, 1, (n_tgt, 3))))


@pytest.mark.parametrize("knn_backend", [0, 1])
def test_smallest_shapes(gpu_ctx_factory, knn_backend):
    """One leaf, one leaf +- 1, the block edge, a half-empty last leaf; non-finite points; duplicates; many-to-one; a 3 rad rotation; no match."""
    from icp_amd import synth
    rng = np.random.default_rng(3)
    ctx = gpu_ctx_factory()
    configure(ctx, metric=0, rejection=0, knn_backend=knn_backend, max_distance=0.05)
    eye = np.eye(4, dtype=f32)
    for n in (1, 7, 8, 9, 255, 257, 1000):
        d = cloud_case(rng, n)
        load(ctx, d, colors=False)
        s = teacher_forced(ctx, d, eye, "n_src %d" % n)
        assert s["n_matched"] > 0
    # NaN and inf source points: never matched, never rivals
    d = cloud_case(rng, 300)
    d["src_pts"][::7, 0] = np.nan; d["src_pts"][3::11, 2] = np.inf; d["src_pts"][5::13, 1] = -np.inf
    load(ctx, d, colors=False)
    teacher_forced(ctx, d, eye, "non-finite source")
    # exact duplicates: only the lowest index of a group is mutual
    d = cloud_case(rng, 200)
    d["src_pts"][100:] = d["src_pts"][:100]
    d["src_pts"][150:] = d["src_pts"][:50]
    load(ctx, d, colors=False)
    teacher_forced(ctx, d, eye, "duplicates")
    ctx.set_reciprocal_options(True)
    recs, _, _ = ctx.correspond(eye)
    ctx.set_reciprocal_options(False)
    assert (recs["idx"][100:] == -1).all() and (recs["idx"][:100] >= 0).any()
    # every source point matches the same target point: one mutual pair
    d = cloud_case(rng, 400)
    d["tgt_pts"][:] = (50 + rng.uniform(0, 1, d["tgt_pts"].shape)).astype(f32); d["tgt_pts"][17] = (0.5, 0.5, 0.5)
    configure(ctx, metric=0, rejection=0, knn_backend=knn_backend, max_distance=3.0)
    load(ctx, d, colors=False)
    s = teacher_forced(ctx, d, eye, "many to one")
    assert s == dict(n_matched=400, n_mutual=1)
    # a pose with a 3 rad rotation
    T = synth.make_pose((3.0, 0.4, -0.2), (0.3, -0.2, 0.1)).astype(f32)
    d = cloud_case(rng, 500)
    Ti = np.linalg.inv(T.astype(np.float64))
    d["src_pts"] = (d["src_pts"].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)
    configure(ctx, metric=0, rejection=0, knn_backend=knn_backend, max_distance=0.05)
    load(ctx, d, colors=False)
    s = teacher_forced(ctx, d, T, "3 rad")
    assert s["n_matched"] > 250 and s["n_mutual"] > 100
    # an empty match set: stats {0, 0}, the status as with the option off
    d = cloud_case(rng, 64); d["src_pts"] += f32(30)
    load(ctx, d, colors=False)
    out = {}
    for on in (False, True):
        ctx.set_reciprocal_options(on)
        recs, sums, nv = ctx.correspond(eye)
        assert (recs["idx"] < 0).all() and nv == 0
        pose, rr, rc = ctx.run(eye, check=False)
        out[on] = (rc, [r["status"] for r in rr], u32(pose).tolist())
        if on:
            assert ctx.reciprocal_stats() == [dict(n_matched=0, n_mutual=0)] * len(rr)
    ctx.set_reciprocal_options(False)
    assert out[True] == out[False] and out[True][0] == 8


def test_off_is_untouched(gpu_ctx_factory, bunny):
    import support as M
    eye = np.eye(4, dtype=f32)
    a = gpu_ctx_factory(); configure(a, metric=1, n_iterations=10); load(a, bunny)
    pa, ra, _ = a.run(eye)
    b = gpu_ctx_factory(); configure(b, metric=1, n_iterations=10); load(b, bunny)
    b.set_reciprocal_options(False)
    m0 = M.counters(b)[0]
    pb, rb, _ = b.run(eye)
    assert M.counters(b)[0] == m0 + 1                      # the merged loop was taken
    b.set_reciprocal_options(True)
    b.run(eye)
    assert M.counters(b)[0] == m0 + 1 and len(b.reciprocal_stats()) == 10      # the option does not take it
    b.set_reciprocal_options(False)
    pc, rc_, _ = b.run(eye)
    assert M.counters(b)[0] == m0 + 2 and b.reciprocal_stats() == []
    for p_, r_ in ((pb, rb), (pc, rc_)):
        assert np.array_equal(u32(pa), u32(p_))
        assert all(np.array_equal(u32(x["pose"]), u32(y["pose"])) and x["n_valid"] == y["n_valid"] for x, y in zip(ra, r_))


def shuffled(d, seed=5):
    perm = np.random.default_rng(seed).permutation(len(d["src_pts"]))
    out = dict(d); out["src_pts"] = np.ascontiguousarray(d["src_pts"][perm]); out["src_nrm"] = np.ascontiguousarray(d["src_nrm"][perm])
    return out


def test_free_running_full_resolution(gpu_ctx_factory, bunny):
    """icp_run, 10 iterations with the option on: iteration i's stats, n_valid and pose from icp_correspond (option off) at iteration
    i - 1's pose + the restatement + the point-to-plane restatement's sums, solve and composition; the pose within the suite's 1e-5."""
    d = shuffled(bunny)
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, n_iterations=10)
    load(ctx, d, colors=False)
    eye = np.eye(4, dtype=f32)
    ctx.set_reciprocal_options(True)
    pose, recs, rc = ctx.run(eye)
    st = ctx.reciprocal_stats()
    assert rc == 0 and len(recs) == len(st) == 10
    pose2, recs2, _ = ctx.run(eye)
    assert np.array_equal(u32(pose), u32(pose2)) and ctx.reciprocal_stats() == st
    ctx.set_reciprocal_options(False)
    prev = eye
    for i, r in enumerate(recs):
        raw, _ = ctx.match(prev)
        base, _, _ = ctx.correspond(prev)
        exp, stats, _ = expected(base, raw, prev, d["src_pts"], d["tgt_pts"])
        assert st[i] == stats, i
        p = ctx.transform_points(d["src_pts"], prev)
        s, _ = R.sums(1, p, d["tgt_pts"], exp, tgt_nrm=d["tgt_nrm"])
        assert r["n_valid"] == int(s[0]), i
        want = G.compose(G.solve(s), prev)
        assert np.abs(want.astype(np.float64) - r["pose"]).max() <= 1e-5, i
        prev = r["pose"]


@pytest.mark.parametrize("multires,selection,knn_backend", [(1, 0, 1), (0, 1, 1), (0, 2, 1), (1, 1, 0)])
def test_free_running_query_sets(gpu_ctx_factory, bunny, multires, selection, knn_backend):
    """Multires levels, random sampling at 0.5 and normal-space sampling on a shuffled source (sorted position never equals the index): the
    judged index is the ORIGINAL source index -- iteration i's counts equal the restatement on the raw matches of its query set at
    iteration i - 1's pose, tested against the full-resolution source."""
    from icp_amd import binding
    d = shuffled(bunny)
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, rejection=0, n_iterations=5, multires=multires, selection=selection, proba=0.5, knn_backend=knn_backend)
    load(ctx, d, colors=False)
    eye = np.eye(4, dtype=f32)
    ctx.set_reciprocal_options(True)
    pose, recs, rc = ctx.run(eye)
    st = ctx.reciprocal_stats()
    assert rc == 0 and len(st) == len(recs) >= 5
    factors = binding.schedule(ctx.params, len(d["src_pts"]))
    valid = np.isfinite(d["src_pts"]).all(1) & np.isfinite(d["src_nrm"]).all(1)
    sets = []
    for i, f in enumerate(factors):
        if selection:
            sets.append(np.asarray(ctx.selection(i), np.int64))
        elif f > 0:
            c = np.arange(0, len(valid), f); sets.append(c[valid[c]])
        else:
            sets.append(np.arange(len(valid)))
    ctx.set_reciprocal_options(False)
    prev = eye
    for i, r in enumerate(recs):
        Q = sets[i]
        assert r["n_src"] == len(Q), i
        raw, _ = ctx.match(prev)
        ref = RC.reciprocal(raw[Q], prev, d["src_pts"], d["tgt_pts"], orig=Q)
        assert st[i] == ref["stats"], (i, st[i], ref["stats"])
        assert r["n_valid"] == ref["stats"]["n_mutual"], i      # constant weights, no rejection, finite normals: every mutual pair enters
        prev = r["pose"]


def test_with_robust_mode_the_filter_comes_first(gpu_ctx_factory, bunny):
    from icp_amd import synth
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1)
    load(ctx, bunny, colors=False)
    pose = synth.make_pose(*BUNNY_POSES[1]).astype(f32)
    raw, _ = ctx.match(pose)
    base, _, _ = ctx.correspond(pose)
    exp, stats, _ = expected(base, raw, pose, bunny["src_pts"], bunny["tgt_pts"])
    o = dict(kernel="huber", overlap=0.7)
    ref = R.robust(exp, ctx.transform_points(bunny["src_pts"], pose), bunny["tgt_pts"], dict(o, kernel=1), 1)
    ctx.set_reciprocal_options(True); ctx.set_robust_options(**o)
    recs, _, nv = ctx.correspond(pose)
    rs, cs = ctx.robust_stats(), ctx.reciprocal_stats()
    ctx.set_reciprocal_options(False); ctx.set_robust_options()
    assert cs == [stats]
    assert rs[0]["n_entering"] == ref["stats"]["n_entering"] and rs[0]["n_kept"] == ref["stats"]["n_kept"]
    assert u32(f32(rs[0]["trim_d2"])) == u32(f32(ref["stats"]["trim_d2"])) and u32(f32(rs[0]["sigma"])) == u32(f32(ref["stats"]["sigma"]))
    assert np.array_equal(recs["idx"], ref["recs"]["idx"]) and np.array_equal(u32(recs["weight"]), u32(ref["recs"]["weight"]))
    assert rs[0]["n_entering"] <= stats["n_mutual"] and nv == ref["M"]


def test_with_convergence_stop(gpu_ctx_factory, bunny):
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, n_iterations=30)
    load(ctx, bunny, colors=False)
    eye = np.eye(4, dtype=f32)
    ctx.set_reciprocal_options(True)
    _, full, _ = ctx.run(eye)
    st_full = ctx.reciprocal_stats()
    ctx.set_convergence_options(rotation=1e-4, translation=1e-5, min_iterations=2, patience=1)
    pose, recs, _ = ctx.run(eye)
    st = ctx.reciprocal_stats()
    ctx.set_convergence_options(None); ctx.set_reciprocal_options(False)
    n = len(recs)
    assert ctx.convergence()["converged"] and 2 <= n < 30 and len(st) == n
    assert st == st_full[:n]
    assert all(np.array_equal(u32(a["pose"]), u32(b["pose"])) and a["n_valid"] == b["n_valid"] for a, b in zip(recs, full))
    assert np.array_equal(u32(pose), u32(recs[-1]["pose"]))


def test_batch_and_tracking_equal_per_pair_runs(gpu_ctx_factory):
    from icp_amd import binding, eth, synth
    scans = [tuple(np.ascontiguousarray(a, f32) for a in synth.laser_scan(synth.scan_pose(k), 40 + k, n_tilt=43, n_beam=135)[:2]) for k in range(3)]
    pairs = [dict(src_pts=scans[k + 1][0], src_nrm=scans[k + 1][1], tgt_pts=scans[k][0], tgt_nrm=scans[k][1]) for k in range(2)]
    ctxs = [gpu_ctx_factory()]
    for c in ctxs:
        configure(c, n_iterations=12, max_distance=0.05)
        c.set_reciprocal_options(True)
    poses, status, rc = binding.batch_run(ctxs, pairs)      # one context: pair 1's target is pair 0's source, promoted on the device
    ref = gpu_ctx_factory()
    configure(ref, n_iterations=12, max_distance=0.05)
    per_pair = []
    for i, d in enumerate(pairs):
        pose, recs, st = eth.align(ref, d, check=False, reciprocal=True)
        assert st == status[i]
        assert np.array_equal(u32(binding.pose_to_c(pose)), u32(poses[i])), i
        per_pair.append(ref.reciprocal_stats())
    assert ctxs[0].reciprocal_stats() == per_pair[1] and len(per_pair[1]) == 12
    assert all(0 < s["n_mutual"] < s["n_matched"] for s in per_pair[1])
    # tracking
    W, H = 80, 60
    K = np.array([[525.0 / 8, 0, 319.5 / 8], [0, 525.0 / 8, 239.5 / 8], [0, 0, 1]], f32)
    depth = np.stack([synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), W, H, 0x7A11 + k)[0][:, 2].reshape(H, W).copy() for k in range(3)])
    cam = binding.depth_camera(K, W, H)
    to, so = binding.depth_options(False, 1), binding.depth_options(False, 2)
    a = gpu_ctx_factory(); configure(a, n_iterations=15, max_distance=0.01); a.set_reciprocal_options(True)
    _, trecs, _ = a.track_depth_frames(depth, None, cam, to, so)
    b = gpu_ctx_factory(); configure(b, n_iterations=15, max_distance=0.01); b.set_reciprocal_options(True)
    b.set_target_depth(depth[0], None, cam, to)
    pose = np.eye(4, dtype=f32)
    for k in range(1, 3):
        b.set_source_depth(depth[k], None, cam, so)
        pose, _, st = b.run(pose, check=False)
        assert trecs[k - 1]["status"] == st
        assert np.array_equal(u32(trecs[k - 1]["pose"]), u32(pose)), k
    assert a.reciprocal_stats() == b.reciprocal_stats() and len(a.reciprocal_stats()) == 15


def test_refusals_and_isolation(gpu_ctx_factory, bunny):
    from icp_amd import binding
    lib = binding.load_library()
    ctx = gpu_ctx_factory()
    o = binding.IcpReciprocalOptions(2)
    assert lib.icp_set_reciprocal_options(ctx.h, C.byref(o)) == 1 and b"icp_set_reciprocal_options" in lib.icp_last_error(ctx.h)
    assert ctx.reciprocal_options().enabled == 0
    assert lib.icp_set_reciprocal_options(ctx.h, None) == 0 and ctx.reciprocal_options().enabled == 0
    configure(ctx, metric=1, n_iterations=8)
    load(ctx, bunny)
    eye = np.eye(4, dtype=f32)
    ctx.set_reciprocal_options(True)
    assert ctx.reciprocal_options().enabled == 1
    # colour ICP: a 6-D forward search
    configure(ctx, metric=1, n_iterations=8, color_icp=1)
    assert ctx.run(eye, check=False)[2] == 1 and "color_icp" in lib.icp_last_error(ctx.h).decode()
    with pytest.raises(binding.IcpError) as ei:
        ctx.correspond(eye)
    assert ei.value.code == 1 and "color_icp" in str(ei.value)
    configure(ctx, metric=1, n_iterations=8)
    # the non-linear optimiser
    ctx.set_optimizer(True)
    assert ctx.run(eye, check=False)[2] == 1 and "reciprocal" in lib.icp_last_error(ctx.h).decode()
    ctx.set_optimizer(None)
    for call in (lambda: ctx.run_multistart([eye]), lambda: ctx.match_seeded([eye])):
        with pytest.raises(binding.IcpError) as ei:
            call()
        assert ei.value.code == 1 and "reciprocal" in str(ei.value)
    p1, r1, _ = ctx.run(eye)
    s1 = ctx.reciprocal_stats()
    # another context, option off, runs in between: neither disturbs the other
    other = gpu_ctx_factory(); configure(other, metric=1, n_iterations=8); load(other, bunny)
    q1, _, _ = other.run(eye)
    p2, r2, _ = ctx.run(eye)
    q2, _, _ = other.run(eye)
    assert np.array_equal(u32(p1), u32(p2)) and ctx.reciprocal_stats() == s1 and np.array_equal(u32(q1), u32(q2)) and other.reciprocal_stats() == []
    fresh = gpu_ctx_factory(); configure(fresh, metric=1, n_iterations=8); load(fresh, bunny)
    assert np.array_equal(u32(fresh.run(eye)[0]), u32(q1))
    # icp_set_source drops the reverse index: a second, different source gets its own answers
    d2 = dict(bunny)
    d2["src_pts"] = np.ascontiguousarray(bunny["src_pts"][::-1][:len(bunny["src_pts"]) * 2 // 3] + f32(0.0007))
    d2["src_nrm"] = np.ascontiguousarray(bunny["src_nrm"][::-1][:len(d2["src_pts"])])
    ctx.set_source(d2["src_pts"], d2["src_nrm"], None)
    configure(ctx, metric=1, n_iterations=8)
    teacher_forced(ctx, d2, eye, "second source")
    ctx.set_source(bunny["src_pts"], bunny["src_nrm"], None)
    teacher_forced(ctx, bunny, eye, "first source again")
    # device bytes back to the baseline after destroy (the source tree and its position map included)
    import gc
    gc.collect()

    def live():
        v = C.c_int64(0)
        assert lib.icp_debug_live_bytes(C.byref(v)) == 0
        return v.value
    before = live()
    c = binding.Context(0)
    configure(c, metric=1, n_iterations=4); load(c, bunny, colors=False)
    c.set_reciprocal_options(True)
    c.run(eye); c.correspond(eye)
    assert live() > before
    c.close()
    assert live() == before


def partial_overlap_fixture():
    """ETH-like pair at 24 x 80 beams (under 2 000 points per cloud); the target loses every point beyond the 60 % quantile of the
    unperturbed source's x, so 40 % of the source has no counterpart."""
    from icp_amd import synth
    return synth.partial_overlap_pair(FIXTURE_PAIR, 24, 80, FIXTURE_QUANTILE, drop_target_normals=True)


FIXTURE_PAIR, FIXTURE_QUANTILE, FIXTURE_MAX_DISTANCE = 0, 0.6, 10.0


def test_partial_overlap_outcome():
    """The reason for the feature: the source's part without a counterpart piles many-to-one pairs on the rim of the overlap and drags the
    pose; the mutual test removes them without being told the overlap.  Point-to-plane, constant weights, no rejection, 20 iterations.
    The fixture (pair 0, 24 x 80 beams, cut at the 60 % quantile, max distance 10) was picked on the CPU with reciprocal_restatement.icp
    (brute-force matcher): over pairs 0-2, quantiles 0.6 / 0.7 and max distances 10 / 1 the option always ended closer to the ground truth;
    this one gave 0.146 rad / 0.346 m off and 1.07e-3 rad / 1.64e-3 m on.  The device gave 0.146 rad / 0.346 m and 1.07e-3 rad / 1.64e-3 m."""
    from icp_amd import binding
    d = partial_overlap_fixture()
    assert len(d["src_pts"]) <= 2000 and len(d["tgt_pts"]) <= 2000
    errs = {}
    for on in (False, True):
        ctx = binding.Context(0)
        try:
            configure(ctx, metric=1, rejection=0, n_iterations=20, max_distance=FIXTURE_MAX_DISTANCE)
            load(ctx, d, colors=False)
            ctx.set_reciprocal_options(on)
            pose, recs, rc = ctx.run(np.eye(4, dtype=f32))
            errs[on] = pose_error(pose, d["gt"])
        finally:
            ctx.close()
    (a0, t0), (a1, t1) = errs[False], errs[True]
    print("partial overlap: off %.3g rad / %.3g m, on %.3g rad / %.3g m" % (a0, t0, a1, t1))
    assert a1 <= a0 and t1 <= t0, errs
