"""Voxelized GICP on the device against the numpy restatement of its contract (tests/vgicp_restatement.py): the grid exactly (integer sums)
and bit for bit (records), the sums of one step within the summation-order bound, every step of an alignment, the stop and the drain, the
failure that carries the pose, bit-identical repeats, icp_run untouched, and the outcome on the recorded fixture."""
import ctypes as C
import functools
import json
import numpy as np
import pytest

import support as S
import vgicp_restatement as VR
import vgicp_outcome_fixture as VF
from support import pose_of, same_bits

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = 1, 3, 4, 8
N = 4099
EPS = 1e-3
NEAR = ((0.012, -0.009, 0.015), (0.02, -0.015, 0.01))
FAR = ((-0.03, 0.025, -0.02), (-0.04, 0.03, 0.035))
AWAY = ((0.0, 0.0, 0.0), (50.0, 0.0, 0.0))


def u64(a):
    return np.ascontiguousarray(a, dtype=f64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def crafted():
    """4099 target points with normals, in an order a scan would have (rows of a wavy surface), and in it:
      [30, 350)     320 consecutive points of ONE cell at both voxel sizes: the run crosses the wave boundaries 64 .. 320 and the block boundary 256
      [500, 540)    40 points of one cell across the block boundary 512
      [600, 664)    dyadic coordinates (multiples of 1/8: exactly on cell faces at 0.25), negative ones among them
      [700, 708)    single-point cells, far from everything else
      [720, 728)    positions with NaN / +inf / -inf, [728, 732) NaN normals, 732 an infinite normal component: all stay out
      4098          the last point, alone in the last (partial) block's last wave
    Returned read-only: (points, normals)."""
    r = np.random.default_rng(2021)
    k = np.arange(N)
    row, col = k // 64, k % 64
    x = -1.0 + col * (2.2 / 64) + r.normal(0, 0.002, N); y = -1.0 + row * (2.2 / 65) + r.normal(0, 0.002, N)
    z = 0.3 * np.sin(2.0 * x) + 0.2 * np.cos(3.0 * y) + 0.25 * (x > 0.4)
    n = np.stack([-0.6 * np.cos(2.0 * x), 0.6 * np.sin(3.0 * y), np.ones(N)], 1)
    n += r.normal(0, 0.02, (N, 3))
    pts = np.stack([x, y, z], 1)
    pts[30:350] = (0.66, 0.66, 0.66) + r.uniform(-0.02, 0.02, (320, 3))
    pts[500:540] = (-0.40, -0.41, 0.40) + r.uniform(-0.02, 0.02, (40, 3))
    pts[600:664] = r.integers(-9, 10, (64, 3)) / 8.0
    pts[700:708] = np.array([3.1, -2.2, 1.3]) + np.arange(8)[:, None] * np.array([0.37, -0.41, 0.29])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    pts = pts.astype(f32); n = n.astype(f32)
    bad = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (np.nan, np.nan, np.nan), (np.inf, -np.inf, 0), (-np.inf, 1, 1), (1, np.nan, 1), (1, 1, np.inf)]
    pts[720:728] = np.array(bad, f32)
    n[728:732] = np.array([(np.nan, 0, 1), (0, np.nan, 0), (0, 0, np.nan), (np.nan, np.nan, np.nan)], f32)
    n[732] = (0, np.inf, 1)
    pts.setflags(write=False); n.setflags(write=False)
    return pts, n


@functools.lru_cache(maxsize=None)
def crafted_source():
    """The crafted target moved by the inverse of a small pose (fp64, rounded once), with a zero normal and a NaN normal of its own."""
    pts, n = crafted()
    T = np.linalg.inv(pose_of((0.02, -0.015, 0.01), (0.03, 0.02, -0.025)).astype(f64))
    with np.errstate(all="ignore"):
        sp = (pts.astype(f64) @ T[:3, :3].T + T[:3, 3]).astype(f32); sn = (n.astype(f64) @ T[:3, :3].T).astype(f32)
    sn[5] = (0, 0, 0); sn[6] = (np.nan, 0, 0)
    sp.setflags(write=False); sn.setflags(write=False)
    return sp, sn


@functools.lru_cache(maxsize=None)
def crafted_grid(vs):
    return VR.grid(*crafted(), vs)


def crafted_ctx(factory, source=True):
    ctx = factory()
    ctx.set_gicp_options(EPS, 0)
    ctx.set_target(*crafted(), None)
    if source:
        ctx.set_source(*crafted_source(), None)
    return ctx


def test_crafted_target_has_what_it_claims():
    pts, n = crafted()
    ok = VR.entering(pts, n)
    assert len(pts) == N and ok.sum() == N - 13 and (pts[ok] < 0).any()
    for vs in (0.25, 0.3):
        c = VR.cell_coords(pts[ok], vs); idx = np.cumsum(ok) - 1
        assert len(np.unique(c[idx[30]:idx[349] + 1], axis=0)) == 1 and len(np.unique(c[idx[500]:idx[539] + 1], axis=0)) == 1
        g = crafted_grid(vs)
        assert g["counts"].max() >= 320 and (g["counts"] == 1).sum() >= 8 and (g["counts"] == 0).sum() > 100
    dy = pts[600:664]
    assert (dy * 8 == np.rint(dy * 8)).all() and ((dy / f32(0.25)) == np.rint(dy / f32(0.25))).any(1).sum() > 30 and (dy < 0).any()


@pytest.mark.parametrize("vs", [0.25, 0.3])
def test_grid_matches_restatement(gpu_ctx_factory, vs):
    """lo, dims, counts and the nine int64 sums exactly, the records bit for bit; a rebuild gives the same bytes; the grid goes with the
    target and with new GICP options."""
    ctx = crafted_ctx(gpu_ctx_factory, source=False)
    g = crafted_grid(vs)
    info, counts, sums, cells = ctx.voxel_grid(voxel_size=vs)
    print("grid %.2f: lo %s dims %s, %d occupied cells of %d, %d points" % (vs, info["lo"], info["dims"], info["n_occupied"], counts.size, info["n_points"]))
    assert info["lo"] == tuple(g["lo"]) and info["dims"] == tuple(g["dims"]) and info["n_occupied"] == g["n_occupied"] and info["n_points"] == g["n_points"] == N - 13
    assert np.array_equal(counts, g["counts"])
    assert np.array_equal(sums, g["sums"])
    assert np.array_equal(S.u32(cells), S.u32(g["cells"]))
    # a second build from scratch: the same bytes
    ctx.set_gicp_options(EPS, 0)
    assert ctx.lib.icp_get_voxel_grid(ctx.h, None, None, None) == ERR_INVALID_ARG       # new GICP options dropped the grid
    info2, counts2, sums2, cells2 = ctx.voxel_grid(voxel_size=vs)
    assert info2 == info and np.array_equal(counts2, counts) and np.array_equal(sums2, sums) and np.array_equal(S.u32(cells2), S.u32(cells))
    assert ctx.lib.icp_get_voxel_grid(ctx.h, None, None, None) == 0                     # any pointer may be NULL
    ctx.set_target(*crafted(), None)
    assert ctx.lib.icp_get_voxel_grid(ctx.h, None, None, None) == ERR_INVALID_ARG       # a new target dropped it
    assert "no voxel grid" in ctx.lib.icp_last_error(ctx.h).decode()


def test_grid_refusals(gpu_ctx_factory):
    """More than 2^24 cells, from two points 10^6 m apart at 1 cm (10^8 cells along x): refused by the extent, before anything is allocated,
    with a message that names the voxel size.  No entering point, no target, k = 0 without normals."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    o = binding.vgicp_options(voxel_size=0.01)
    assert ctx.lib.icp_voxelize_target(ctx.h, C.byref(o), None) == ERR_NO_TARGET
    ctx.set_gicp_options(EPS, 0)
    two = np.array([[0, 0, 0], [1e6, 0, 0]], f32); nn = np.array([[0, 0, 1], [0, 0, 1]], f32)
    ctx.set_target(two, nn, None)
    assert ctx.lib.icp_voxelize_target(ctx.h, C.byref(o), None) == ERR_INVALID_ARG
    msg = ctx.lib.icp_last_error(ctx.h).decode()
    assert "voxel_size 0.01" in msg and "2^24" in msg, msg
    with pytest.raises(VR.GridTooLarge):
        VR.grid(two, nn, 0.01)
    assert ctx.voxelize_target(voxel_size=1e5)["dims"] == (11, 1, 1)
    ctx.set_target(two, np.full((2, 3), np.nan, f32), None)
    assert ctx.lib.icp_voxelize_target(ctx.h, C.byref(o), None) == ERR_NO_TARGET
    ctx.set_target(two, None, None)
    assert ctx.lib.icp_voxelize_target(ctx.h, C.byref(o), None) == ERR_INVALID_ARG
    assert "normals" in ctx.lib.icp_last_error(ctx.h).decode()
    # the alignment's own refusals: no source; k = 0 and a source without normals
    ctx.set_target(*crafted(), None)
    p = binding.pose_to_c(np.eye(4)); o = binding.vgicp_options()
    assert ctx.lib.icp_vgicp_align(ctx.h, C.byref(o), binding._ptr(p), None, None, 0) == ERR_NO_SOURCE
    ctx.set_source(crafted_source()[0], None, None)
    assert ctx.lib.icp_vgicp_align(ctx.h, C.byref(o), binding._ptr(p), None, None, 0) == ERR_INVALID_ARG
    assert "normals" in ctx.lib.icp_last_error(ctx.h).decode()


def check_system(ctx, g, src, sn, pose, what, **kw):
    sums, counts = ctx.vgicp_system(pose, **kw)
    rcounts, rsums, rabs = VR.system(g, src, sn, pose, EPS, kw.get("min_points", 1))
    bound = rcounts[1] * 2.0 ** -52 * rabs
    err = np.abs(sums - rsums)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print("system %s %s: considered %d, valid %d, worst |sum - restatement| / bound = %.3g" % (what, kw, counts[0], counts[1], frac))
    assert tuple(counts) == tuple(rcounts), (what, counts, rcounts)
    assert (err <= bound).all(), (what, kw, err, bound)
    again, counts2 = ctx.vgicp_system(pose, **kw)
    assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts), what
    return counts


def test_system_matches_restatement(gpu_ctx_factory, bunny):
    """The sums of one step: counts exactly; every sum within n_valid 2^-52 sum |term| of the restatement's; two calls give identical bits.
    4099 source points (9 blocks of 512, the last with 3 points) at both voxel sizes, 300 of them alone (one partial block) and the bunny's 1054 (3 blocks, the last partial) against the
    bunny's own target at 2 cm voxels; poses that leave points outside the grid, in empty cells and in cells below min_points; min_points
    1 and 3.  That is 9, 1 and 3 blocks: k_sdf_solve's fold beyond 64, 256 and 512 blocks is tests/test_gpu_fold_sizes.py's."""
    ctx = crafted_ctx(gpu_ctx_factory)
    sp, sn = crafted_source()
    seen = []
    for vs in (0.25, 0.3):
        g = crafted_grid(vs)
        for pose in (np.eye(4, dtype=f32), pose_of(*NEAR), pose_of((0.3, -0.2, 0.25), (0.8, -0.5, 0.3))):
            for mp in (1, 3):
                seen.append(check_system(ctx, g, sp, sn, pose, "crafted %.2f" % vs, voxel_size=vs, min_points=mp))
    assert all(c[0] == N - 8 for c in seen)                   # the eight non-finite positions are not considered
    assert seen[0][1] > seen[1][1] > 1000 and seen[4][1] < 0.8 * seen[0][1]      # min_points 3 drops single cells; the far pose leaves the grid
    # one block, partial: the first 300 source points alone
    ctx.set_source(sp[:300], sn[:300], None)
    c = check_system(ctx, crafted_grid(0.3), sp[:300], sn[:300], pose_of(*NEAR), "crafted 0.30, 300 points", voxel_size=0.3)
    assert c[0] == 300 and 200 < c[1] < 300
    n_src = len(bunny["src_pts"])
    assert n_src == 1054
    ctx.set_target(bunny["tgt_pts"], bunny["tgt_nrm"], None)
    ctx.set_source(bunny["src_pts"], bunny["src_nrm"], None)
    g = VR.grid(bunny["tgt_pts"], bunny["tgt_nrm"], 0.02)
    for pose in (np.eye(4, dtype=f32), pose_of((0.05, -0.04, 0.03), (0.01, -0.008, 0.012))):
        for mp in (1, 3):
            c = check_system(ctx, g, bunny["src_pts"], bunny["src_nrm"], pose, "bunny 0.02", voxel_size=0.02, min_points=mp)
            assert 100 < c[1] < c[0] <= n_src


def test_align_steps_follow_the_restatement(gpu_ctx_factory):
    """8 iterations with the stops off, traced, from two starts.  Iteration i's pose within 1e-5 per element of step(system(the DEVICE's
    pose i - 1)); n_valid exactly; the cost within the summation bound.  A second run gives identical bits."""
    ctx = crafted_ctx(gpu_ctx_factory)
    sp, sn = crafted_source()
    g = crafted_grid(0.25)
    kw = dict(voxel_size=0.25, n_iterations=8, stop_rotation=0.0, stop_translation=0.0)
    for start in (np.eye(4, dtype=f32), pose_of(*FAR)):
        pose, rec, rc, trace = ctx.vgicp_align(start, trace=True, **kw)
        assert rc == 0 and rec["status"] == 0 and rec["iterations"] == 8 and len(trace) == 8
        prev = start
        for i, t in enumerate(trace):
            counts, sums, sabs = VR.system(g, sp, sn, prev, EPS)
            want, _ = VR.step(sums, counts, prev)
            diff = float(np.abs(t["pose"] - want).max())
            print("align step %d: n_valid %d, cost %.6g, |pose - restatement| = %.3g" % (i, t["n_valid"], t["cost"], diff))
            assert t["status"] == 0 and t["n_valid"] == counts[1], i
            assert diff <= 1e-5, i
            assert abs(t["cost"] - sums[27]) <= counts[1] * 2.0 ** -52 * sabs[27], i
            prev = t["pose"]
        assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose)
        assert (rec["n_depth"], rec["n_valid_first"], rec["n_valid_last"]) == (N - 8, trace[0]["n_valid"], trace[-1]["n_valid"])
        assert u64(rec["cost_first"]) == u64(trace[0]["cost"]) and u64(rec["cost_last"]) == u64(trace[-1]["cost"]) and rec["cost_last"] < rec["cost_first"]
        pose2, rec2, rc2, trace2 = ctx.vgicp_align(start, trace=True, **kw)
        assert rc2 == 0 and same_bits(pose2, pose)
        for a, b in zip(trace, trace2):
            assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])


def test_stop_drain_and_failure(gpu_ctx_factory):
    """With the stops at 1e-3 the alignment ends early; its trace is bit for bit the head of the full run's, the returned pose is the stop
    iteration's, and the records past it stay zero: the launches behind the stop have drained.  A start 50 m away has no valid point: the
    first step fails, the pose is carried, the status is ICP_ERR_NO_CORRESPONDENCES."""
    from icp_amd import binding
    ctx = crafted_ctx(gpu_ctx_factory)
    start = np.eye(4, dtype=f32)
    full_pose, full_rec, rc, full = ctx.vgicp_align(start, trace=True, stop_rotation=0.0, stop_translation=0.0)
    assert rc == 0 and len(full) == 30 and full_rec["iterations"] == 30
    pose, rec, rc, trace = ctx.vgicp_align(start, trace=True, stop_rotation=1e-3, stop_translation=1e-3)
    n = rec["iterations"]
    print("stop: %d of 30 iterations" % n)
    assert rc == 0 and 1 <= n < 30 and len(trace) == n
    for a, b in zip(trace, full):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose)
    o = binding.vgicp_options(stop_rotation=1e-3, stop_translation=1e-3)
    p = binding.pose_to_c(start); r = binding.IcpSdfFrame(); tr = (binding.IcpSdfIter * 30)()
    assert ctx.lib.icp_vgicp_align(ctx.h, C.byref(o), binding._ptr(p), C.byref(r), tr, 30) == 0
    assert r.iterations == n and not any(bytes(tr[i]) != bytes(80) for i in range(n, 30)) and bytes(tr[n - 1]) != bytes(80)
    # max_trace below n_iterations: only that many records are written
    tr2 = (binding.IcpSdfIter * 30)(); p = binding.pose_to_c(start)
    assert ctx.lib.icp_vgicp_align(ctx.h, C.byref(o), binding._ptr(p), C.byref(r), tr2, 1) == 0
    assert bytes(tr2[0]) == bytes(tr[0]) and not any(bytes(tr2[i]) != bytes(80) for i in range(1, 30))
    away = pose_of(*AWAY)
    pose, rec, rc, trace = ctx.vgicp_align(away, trace=True)
    assert rc == ERR_NO_CORRESPONDENCES and rec["status"] == rc and same_bits(pose, away) and same_bits(rec["pose"], away)
    assert rec["iterations"] == 1 and rec["n_depth"] == N - 8 and rec["n_valid_first"] == 0 and len(trace) == 1 and trace[0]["status"] == rc
    assert "icp_vgicp_align" in ctx.lib.icp_last_error(ctx.h).decode()
    # fewer than min_valid, but not none: the same failure
    pose, rec, rc = ctx.vgicp_align(pose_of(*NEAR), min_valid=4000)
    assert rc == ERR_NO_CORRESPONDENCES and 1000 < rec["n_valid_first"] < 4000 and same_bits(pose, pose_of(*NEAR))


@pytest.mark.parametrize("metric", [1, 3])
def test_icp_run_is_untouched(gpu_ctx_factory, metric):
    """icp_run (point-to-plane, GICP with its 20-neighbour normals) on a context that has voxelized, taken a system and aligned, against a
    context that never did: records and poses bit for bit."""
    from icp_amd import synth
    d = synth.eth_like_pair(0, 20, 64)
    start = np.eye(4, dtype=f32)
    runs = []
    for touched in (True, False):
        ctx = gpu_ctx_factory()
        S.configure(ctx, metric=metric, n_iterations=6, max_distance=0.5)
        S.load(ctx, d, colors=False)
        if touched:
            ctx.voxelize_target(voxel_size=0.5)
            ctx.vgicp_system(start, voxel_size=0.5)
            _, rec, rc = ctx.vgicp_align(start, voxel_size=0.5, n_iterations=5)
            assert rc == 0 and rec["n_valid_first"] > 64
        runs.append(ctx.run(start))
    (pa, ra, rca), (pb, rb, rcb) = runs
    assert rca == rcb == 0 and same_bits(pa, pb)
    S.assert_same_run(ra, rb)


def test_outcome_on_the_recorded_fixture(gpu_ctx_factory):
    """synth.eth_like_pair(0, 86, 270), the clouds' own normals, epsilon 1e-3, voxel 0.25, 30 iterations, stops off, from the identity: the
    device ends within twice the restatement's recorded error (tests/golden/vgicp_outcome.json: 2.83e-4 rad / 1.86e-3 m) and below a tenth
    of the identity's (0.056 rad / 0.042 m).  eth.align(vgicp=...) is the same call."""
    from icp_amd import eth
    with open(VF.GOLDEN) as f:
        gold = json.load(f)
    d = VF.pair()
    ctx = gpu_ctx_factory()
    ctx.set_gicp_options(VF.EPSILON, 0)
    pose, recs, rc = eth.align(ctx, d, vgicp=dict(VF.OPTIONS))
    rec = recs[0]
    rot, tr = VF.pose_error(pose, d["gt"])
    print("outcome: device %.3g rad / %.3g m, restatement %.3g rad / %.3g m, identity %.3g rad / %.3g m; n_valid %d -> %d" % (
        rot, tr, gold["rotation_rad"], gold["translation_m"], gold["identity_rotation_rad"], gold["identity_translation_m"], rec["n_valid_first"], rec["n_valid_last"]))
    assert rc == 0 and rec["iterations"] == 30 and rec["n_valid_first"] == gold["n_valid_first"]
    assert rot <= 2 * gold["rotation_rad"] and tr <= 2 * gold["translation_m"]
    assert rot < 0.1 * gold["identity_rotation_rad"] and tr < 0.1 * gold["identity_translation_m"]
    pose2, rec2, rc2 = ctx.vgicp_align(np.eye(4, dtype=f32), **VF.OPTIONS)
    assert rc2 == 0 and same_bits(pose2, pose)
