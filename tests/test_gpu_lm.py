"""The non-linear optimiser (CeresICPOptimizer) on an MI355X against the fp64 restatement (tests/lm_restatement.py).

Teacher-forced: per ICP iteration the device's own records after weighting + rejection (icp_correspond at the iteration's pose) and
its transforms go into the restatement; the device's icp_iterate from the same pose must take the same LM decisions (counts,
iterations, termination), reach the same x (1e-9 relative) and the same pose (1e-5).  Free-running: icp_run against the restatement's
own trajectory.  Plus the edge cases and the untouched linear path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_restatement as lm          # noqa: E402
from support import restated_step          # noqa: E402

pytestmark = pytest.mark.gpu


def make_ctx(gpu_ctx_factory, pair, metric, weighting=0, rejection=1, n_iterations=20, max_distance=0.0003, knn_backend=1, nonlinear=True,
             opts=None):
    c = gpu_ctx_factory()
    p = c.params
    p.metric, p.weighting, p.rejection, p.n_iterations, p.max_distance, p.knn_backend = metric, weighting, rejection, n_iterations, max_distance, knn_backend
    c.push_params()
    c.set_target(pair["tgt_pts"], pair["tgt_nrm"], pair.get("tgt_rgba"))
    c.set_source(pair["src_pts"], pair["src_nrm"], pair.get("src_rgba"))
    if nonlinear:
        c.set_optimizer(True, **(opts or {}))
    return c


def same_solve(dev, ref, x_tol=1e-9):
    """Same decisions iteration by iteration (accepted / invalid masks, the rest rejected), same counts and end, same x."""
    for k in ("iterations", "successful_steps", "unsuccessful_steps", "invalid_steps", "termination", "n_residual_blocks",
              "accepted_steps_mask", "invalid_steps_mask"):
        assert dev[k] == ref[k], (k, dev, ref)
    scale = max(np.abs(ref["x"]).max(), 1e-300)
    assert np.abs(dev["x"] - ref["x"]).max() <= x_tol * scale, (dev["x"], ref["x"])
    assert np.isclose(dev["initial_cost"], ref["initial_cost"], rtol=1e-9, atol=0)


def teacher_forced(c, pair, metric, pose, n_iter, opts=None):
    """Returns the device's summaries of the n_iter solves (each checked against the restatement)."""
    out = []
    for it in range(n_iter):
        x, summ, _, ref_pose = restated_step(c, pair, metric, pose, opts)
        dev_pose, rec = c.iterate(pose)
        dsum = c.lm_summaries()
        assert len(dsum) == 1
        same_solve(dsum[0], summ)
        assert np.abs(dev_pose - ref_pose).max() <= 1e-5, (it, dev_pose, ref_pose)
        assert rec["status"] == (8 if summ["termination"] == lm.NO_RESIDUALS else 0)
        out.append(dsum[0])
        pose = dev_pose
    return out


def bunny_pair(bunny):
    return dict(src_pts=bunny["src_pts"], src_nrm=bunny["src_nrm"], src_rgba=bunny["src_rgba"],
                tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"], tgt_rgba=bunny["tgt_rgba"])


# Options that drive k_lm_step through the branches the default options rarely reach on these pairs, checked against the restatement:
#   reject   : no step can pass min_relative_decrease = 10 -> every step rejected (radius / factor, factor x 2, J kept), iteration limit
#   small    : a tiny first radius -> small accepted steps, the radius grows, the iteration limit ends the solve
#   limit    : max_num_iterations = 1, no tolerance stop -> NO_CONVERGENCE after one step
#   radius   : rejections push the radius under a raised min_trust_region_radius -> CONVERGENCE on the radius
BRANCH_OPTS = {
    "reject": dict(min_relative_decrease=10.0, max_num_iterations=4, function_tolerance=0.0, parameter_tolerance=0.0),
    "small": dict(initial_trust_region_radius=1e-6, function_tolerance=0.0),
    "limit": dict(max_num_iterations=1, function_tolerance=0.0, parameter_tolerance=0.0),
    "radius": dict(initial_trust_region_radius=1e-1, min_trust_region_radius=5e-2, min_relative_decrease=10.0, function_tolerance=0.0,
                   parameter_tolerance=0.0),
}


@pytest.mark.parametrize("branch", sorted(BRANCH_OPTS))
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_teacher_forced_branches(gpu_ctx_factory, bunny, branch, metric):
    opts = BRANCH_OPTS[branch]
    pair = bunny_pair(bunny)
    c = make_ctx(gpu_ctx_factory, pair, metric, opts=opts)
    sums = teacher_forced(c, pair, metric, np.eye(4, dtype=np.float32), 4, opts)
    if branch == "reject":
        for s in sums:
            assert s["termination"] == lm.NO_CONVERGENCE and s["iterations"] == 4 and s["unsuccessful_steps"] == 4
            assert s["accepted_steps_mask"] == 0 and s["trust_region_radius"] == 1e4 / 2 / 4 / 8 / 16 and not np.any(s["x"])
    elif branch == "small":
        assert any(s["termination"] == lm.NO_CONVERGENCE for s in sums)
        assert any(bin(s["accepted_steps_mask"]).count("1") >= 2 and s["trust_region_radius"] > 1e-6 for s in sums)
    elif branch == "limit":
        assert all(s["termination"] == lm.NO_CONVERGENCE and s["iterations"] == 1 for s in sums)
    elif branch == "radius":
        for s in sums:                                  # 0.1 -> 0.05 (not below the minimum) -> 0.0125: CONVERGENCE after iteration 2
            assert s["termination"] == lm.CONVERGENCE and s["iterations"] == 2 and s["trust_region_radius"] == 0.1 / 2 / 4


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("weighting", [0, 1, 2, 3])
@pytest.mark.parametrize("rejection", [0, 1])
def test_teacher_forced_bunny(gpu_ctx_factory, bunny, metric, weighting, rejection):
    pair = dict(src_pts=bunny["src_pts"], src_nrm=bunny["src_nrm"], src_rgba=bunny["src_rgba"],
                tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"], tgt_rgba=bunny["tgt_rgba"])
    c = make_ctx(gpu_ctx_factory, pair, metric, weighting, rejection)
    teacher_forced(c, pair, metric, np.eye(4, dtype=np.float32), 4)


def test_teacher_forced_370k(gpu_ctx_factory):
    from icp_amd import synth
    pair = synth.eth_like_pair(0)
    assert len(pair["src_pts"]) == 370488
    c = make_ctx(gpu_ctx_factory, pair, 1, max_distance=10.0)
    teacher_forced(c, pair, 1, np.eye(4, dtype=np.float32), 3)


# Every non-linear row of bunny_experiments.csv: (metric, selection, weighting, multires); 20 iterations, max distance 0.0003, probability
# 0.5 for the random-sampling rows (here with a fixed selection_seed).
BUNNY_ROWS = {
    "bunny000": (0, 0, 0, 0), "bunny001": (1, 0, 0, 0), "bunny002": (2, 0, 0, 0),
    "bunny100": (0, 1, 0, 0), "bunny101": (1, 1, 0, 0), "bunny102": (2, 1, 0, 0),
    "bunny200": (0, 0, 1, 0), "bunny201": (1, 0, 1, 0), "bunny202": (2, 0, 1, 0),
    "bunny300": (0, 0, 0, 1), "bunny301": (1, 0, 0, 1), "bunny302": (2, 0, 0, 1),
}
SEED = 1234


def restated_run(gpu_ctx_factory, orc, bunny, metric, selection, weighting, multires, n_iter=20):
    """The restatement's own trajectory of a row: the iteration's source set rebuilt on the host -- multires level
    (PointCloud::getCoarseResolution, the oracle's restatement) and RANDOM_SAMPLING selection (icp_select_hash over the level's original
    indices, iteration number i) -- the device matcher queried at the restatement's pose, the LM solve in numpy."""
    from icp_amd import binding
    q = gpu_ctx_factory()
    q.params.metric, q.params.weighting, q.params.max_distance, q.params.knn_backend = metric, weighting, 0.0003, 1
    q.push_params()
    q.set_target(bunny["tgt_pts"], bunny["tgt_nrm"])
    prm = binding.default_params(); prm.multires, prm.n_iterations = multires, n_iter
    factors = binding.schedule(prm, len(bunny["src_pts"]))
    threshold = int(0.5 * 4294967296.0)
    pose = np.eye(4, dtype=np.float32)
    out = []
    for i, f in enumerate(factors):
        if f == 0:
            pts, nrm, idx = bunny["src_pts"], bunny["src_nrm"], np.arange(len(bunny["src_pts"]))
        else:
            pts, nrm, _, idx = orc.coarse(bunny["src_pts"], bunny["src_nrm"], None, f)
        if selection:
            keep = np.array([binding.select_hash(SEED, i, int(k)) < threshold for k in idx], bool)
            pts, nrm = pts[keep], nrm[keep]
        q.set_source(pts, nrm)
        pair = dict(src_pts=pts, src_nrm=nrm, tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"])
        _, summ, _, pose = restated_step(q, pair, metric, pose)
        out.append((len(pts), summ, pose))
    return out


@pytest.mark.parametrize("row", sorted(BUNNY_ROWS))
def test_free_running_bunny_rows(gpu_ctx_factory, orc, bunny, row):
    """icp_run of the row on the device against the restatement's trajectory, iteration by iteration: level / selection size, status,
    LM iterations and termination, pose within 1e-5; a second run is bit-identical."""
    metric, selection, weighting, multires = BUNNY_ROWS[row]
    pair = dict(src_pts=bunny["src_pts"], src_nrm=bunny["src_nrm"], tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"])
    runs = []
    for _ in range(2):
        c = make_ctx(gpu_ctx_factory, pair, metric, weighting)
        c.params.selection, c.params.selection_proba, c.params.selection_seed, c.params.multires = selection, 0.5, SEED, multires
        c.push_params()
        pose_dev, recs, rc = c.run(np.eye(4, dtype=np.float32), check=False)
        runs.append((pose_dev, recs, rc, c.lm_summaries()))
    (pose_dev, recs, rc, sums), (pose2, recs2, rc2, sums2) = runs
    assert np.array_equal(pose_dev, pose2) and rc == rc2 and all(np.array_equal(a["pose"], b["pose"]) for a, b in zip(recs, recs2))
    ref = restated_run(gpu_ctx_factory, orc, bunny, metric, selection, weighting, multires)
    assert len(recs) == len(sums) == len(ref)
    if multires:
        assert len({n for n, _, _ in ref}) > 1                   # the levels really change
    for it, (n, summ, pose) in enumerate(ref):
        assert recs[it]["n_src"] == n, it
        assert recs[it]["status"] == (8 if summ["termination"] == lm.NO_RESIDUALS else 0), it
        assert (sums[it]["termination"], sums[it]["iterations"]) == (summ["termination"], summ["iterations"]), it
        assert np.abs(recs[it]["pose"] - pose).max() <= 1e-5, (it, recs[it]["pose"], pose)
    assert rc == 0 and np.abs(pose_dev - ref[-1][2]).max() <= 1e-5


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_ear_pairs_rmse_decreases(gpu_ctx_factory, bunny, metric):
    """alignBunnyWithICP's convergence measure (main.cpp:110-124): the four ground-truth ear pairs.  With record_rmse the RMSE is taken after
    every k_lm_step, from the pose it composed: it equals icp_rmse at the recorded pose and ends below where it started."""
    pair = bunny_pair(bunny)
    c = make_ctx(gpu_ctx_factory, pair, metric)
    c.set_convergence_reference(bunny["src_pts"][bunny["gt_src_idx"]], bunny["tgt_pts"][bunny["gt_tgt_idx"]])
    c.params.record_rmse = 1
    c.push_params()
    start = c.rmse(np.eye(4, dtype=np.float32))
    pose, recs, rc = c.run(np.eye(4, dtype=np.float32))
    r = [x["rmse"] for x in recs]
    assert all(x >= 0 for x in r)
    for x in recs:
        assert x["rmse"] == c.rmse(x["pose"])
    assert r[-1] < start and r[-1] <= r[0]


def test_all_weights_zero(gpu_ctx_factory, bunny):
    """COLOR weighting with every colour difference 255 (uint8 wrap-around, weighting.h:28): every weight is exactly 0.  The blocks still
    form (counted), cost and gradient are 0: the gradient test ends each solve at iteration 0 and the pose stays where it was."""
    n_s, n_t = len(bunny["src_pts"]), len(bunny["tgt_pts"])
    pair = dict(src_pts=bunny["src_pts"], src_nrm=bunny["src_nrm"], src_rgba=np.zeros((n_s, 4), np.uint8),
                tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"], tgt_rgba=np.tile(np.array([1, 1, 1, 1], np.uint8), (n_t, 1)))
    c = make_ctx(gpu_ctx_factory, pair, 1, weighting=3, rejection=0, n_iterations=3)
    recs0, _, nv = c.correspond(np.eye(4, dtype=np.float32))
    assert nv > 0 and np.all(recs0["weight"][recs0["idx"] >= 0] == 0)
    pose, recs, rc = c.run(np.eye(4, dtype=np.float32))
    assert np.array_equal(pose, np.eye(4, dtype=np.float32)) and all(r["n_valid"] == nv for r in recs)
    for s in c.lm_summaries():
        assert s["termination"] == lm.CONVERGENCE and s["iterations"] == 0 and s["n_residual_blocks"] >= nv
        assert s["initial_cost"] == 0.0 and not np.any(s["x"])


def test_no_correspondences(gpu_ctx_factory, bunny):
    pair = dict(src_pts=bunny["src_pts"] + np.float32(10.0), src_nrm=bunny["src_nrm"], tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"])
    c = make_ctx(gpu_ctx_factory, pair, 1, n_iterations=3)
    pose, recs, rc = c.run(np.eye(4, dtype=np.float32), check=False)
    assert rc == 8 and all(r["status"] == 8 for r in recs)
    assert np.array_equal(pose, np.eye(4, dtype=np.float32))
    assert all(s["termination"] == lm.NO_RESIDUALS and s["n_residual_blocks"] == 0 for s in c.lm_summaries())


def test_nan_holes_teacher_forced(gpu_ctx_factory, bunny):
    rng = np.random.default_rng(7)
    sp = bunny["src_pts"].copy(); tn = bunny["tgt_nrm"].copy(); sn = bunny["src_nrm"].copy()
    sp[rng.choice(len(sp), 300, replace=False)] = np.nan
    tn[rng.choice(len(tn), 300, replace=False)] = np.inf
    sn[rng.choice(len(sn), 300, replace=False)] = np.nan
    pair = dict(src_pts=sp, src_nrm=sn, tgt_pts=bunny["tgt_pts"], tgt_nrm=tn)
    for metric in (1, 2):
        c = make_ctx(gpu_ctx_factory, pair, metric, rejection=0)
        teacher_forced(c, pair, metric, np.eye(4, dtype=np.float32), 2)


def test_start_at_the_minimum_stops_on_the_gradient(gpu_ctx_factory):
    """Source == target, both noise-free: every residual is zero at x = 0, the gradient test ends the solve at iteration 0."""
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.05, 0.05, (3000, 3)).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (3000, 1))
    pair = dict(src_pts=pts, src_nrm=nrm, tgt_pts=pts, tgt_nrm=nrm)
    c = make_ctx(gpu_ctx_factory, pair, 1, rejection=0)
    pose, rec = c.iterate(np.eye(4, dtype=np.float32))
    s = c.lm_summaries()[0]
    assert s["termination"] == lm.CONVERGENCE and s["iterations"] == 0 and s["final_cost"] == 0.0 and not np.any(s["x"])
    assert np.array_equal(pose, np.eye(4, dtype=np.float32)) and rec["n_valid"] == 3000


def test_linear_path_untouched(gpu_ctx_factory, bunny):
    pair = dict(src_pts=bunny["src_pts"], src_nrm=bunny["src_nrm"], tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"])
    for metric in (0, 1, 2):
        a = make_ctx(gpu_ctx_factory, pair, metric, nonlinear=False)
        b = make_ctx(gpu_ctx_factory, pair, metric, nonlinear=True)
        b.run(np.eye(4, dtype=np.float32), check=False)
        b.set_optimizer(None)
        pa, ra, _ = a.run(np.eye(4, dtype=np.float32), check=False)
        pb, rb, _ = b.run(np.eye(4, dtype=np.float32), check=False)
        assert np.array_equal(pa, pb)
        assert all(np.array_equal(x["pose"], y["pose"]) and x["n_valid"] == y["n_valid"] for x, y in zip(ra, rb))
        assert b.lm_summaries() == []


def test_tracking_matches_per_frame_runs(gpu_ctx_factory):
    """icp_track_depth_frames with the non-linear optimiser == the per-frame loop through icp_set_*_depth + icp_run, bit for bit."""
    from icp_amd import binding, synth, tum
    K = np.array([[262.5, 0, 159.75], [0, 262.5, 119.75], [0, 0, 1]], np.float32)
    depth = np.stack([synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), 320, 240, 0x7A11 + k)[0][:, 2].reshape(240, 320)
                      for k in range(3)]).astype(np.float32)
    cam = binding.depth_camera(K, 320, 240)
    a = gpu_ctx_factory(); a.set_optimizer()
    tum.reconstruct_room_params(a.params, K, 320, 240); a.push_params()
    tgt_o, src_o = tum.reconstruct_room_options(a.params)
    pose_a, recs, rc = a.track_depth_frames(depth, None, cam, tgt_o, src_o)
    b = gpu_ctx_factory(); b.set_optimizer(); b.params = a.params; b.push_params()
    b.set_target_depth(depth[0], None, cam, tgt_o)
    pose = np.eye(4, dtype=np.float32)
    for k in range(1, 3):
        b.set_source_depth(depth[k], None, cam, src_o)
        pose, _, _ = b.run(pose, check=False)
        assert np.array_equal(recs[k - 1]["pose"], pose), k
    assert np.array_equal(pose_a, pose)


def test_teacher_forced_mixed_steps(gpu_ctx_factory, bunny):
    """Rejected and accepted steps interleaved: point-to-plane from a start rotated by 1 rad about z (max distance 0.01, no rejection),
    min_relative_decrease 0.9.  The restatement's decisions here do not change when the threshold moves by 1e-5 (relative), so the
    rounding of the two sums cannot flip them; the device must take the same sequence, step by step."""
    pair = bunny_pair(bunny)
    opts = dict(min_relative_decrease=0.9)
    c = make_ctx(gpu_ctx_factory, pair, 1, rejection=0, max_distance=0.01, opts=opts)
    start = np.eye(4, dtype=np.float32)
    ca, sa = np.cos(1.0), np.sin(1.0)
    start[:2, :2] = np.array([[ca, -sa], [sa, ca]], np.float32)
    sums = teacher_forced(c, pair, 1, start, 2, opts)
    first = sums[0]
    rejected = ((1 << first["iterations"]) - 1) & ~first["accepted_steps_mask"] & ~first["invalid_steps_mask"]
    assert first["unsuccessful_steps"] > 0 and rejected & 1 and first["accepted_steps_mask"]      # rejections first, then accepted steps


# ---------------- the public runners ----------------
def test_python_runners_select_the_nonlinear_optimiser(gpu_ctx_factory, bunny):
    """CeresICPOptimizer (Python), eth.align(nonlinear=True) and a context with set_optimizer() give the same run; nonlinear=False
    returns to the linear optimiser."""
    from icp_amd import binding, eth
    pair = bunny_pair(bunny)
    ref = make_ctx(gpu_ctx_factory, pair, 1)
    pose_ref, recs_ref, _ = ref.run(np.eye(4, dtype=np.float32))
    opt = binding.CeresICPOptimizer(0)
    opt.setMetric(1); opt.setMatchingMaxDistance(0.0003); opt.setNbOfIterations(20); opt.setKnnBackend(1)
    pose_o, recs_o = opt.estimatePose(dict(pts=pair["src_pts"], nrm=pair["src_nrm"]), dict(pts=pair["tgt_pts"], nrm=pair["tgt_nrm"]), np.eye(4, dtype=np.float32))
    assert np.array_equal(pose_o, pose_ref) and len(opt.ctx.lm_summaries()) == 20
    c = gpu_ctx_factory()
    c.params.metric, c.params.max_distance, c.params.knn_backend = 1, 0.0003, 1
    pose_e, recs_e, rc = eth.align(c, pair, nonlinear=True)
    assert rc == 0 and np.array_equal(pose_e, pose_ref) and len(c.lm_summaries()) == 20
    pose_l, _, _ = eth.align(c, pair, nonlinear=False)
    lin = make_ctx(gpu_ctx_factory, pair, 1, nonlinear=False)
    assert np.array_equal(pose_l, lin.run(np.eye(4, dtype=np.float32))[0]) and c.lm_summaries() == []
    with pytest.raises(TypeError):
        c.set_optimizer(binding.lm_options(), max_num_iterations=3)


def test_tum_track_nonlinear(gpu_ctx_factory):
    """tum.track(nonlinear=True) (reconstructRoom with USE_LINEAR_ICP 0) == icp_track_depth_frames on a context with set_optimizer()."""
    from icp_amd import binding, synth, tum
    K = np.array([[262.5, 0, 159.75], [0, 262.5, 119.75], [0, 0, 1]], np.float32)
    depth = np.stack([synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), 320, 240, 0x7A11 + k)[0][:, 2].reshape(240, 320)
                      for k in range(3)]).astype(np.float32)
    seq = dict(depth=depth, rgbx=None, K=K, width=320, height=240, gt=None, frames=[0, 1, 2])
    a = gpu_ctx_factory()
    poses, recs, rc = tum.track(a, seq, with_gt=False, nonlinear=True)
    assert len(a.lm_summaries()) > 0
    b = gpu_ctx_factory(); b.set_optimizer()
    tum.reconstruct_room_params(b.params, K, 320, 240); b.push_params()
    to, so = tum.reconstruct_room_options(b.params)
    _, recs_b, rc_b = b.track_depth_frames(depth, None, binding.depth_camera(K, 320, 240), to, so)
    assert rc == rc_b and all(np.array_equal(x["pose"], y["pose"]) for x, y in zip(recs, recs_b))
    poses_l, recs_l, _ = tum.track(a, seq, with_gt=False, nonlinear=False)
    assert a.lm_summaries() == []


def test_cxx_ceres_adaptor(tmp_path, gpu_ctx_factory, bunny):
    """HipCeresICPOptimizer (include/icp_hip_adaptor.hpp) driven like alignBunnyWithICP with USE_LINEAR_ICP 0: same pose as the Python
    context, one summary per ICP iteration."""
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libdir = os.path.join(root, "icp-variants_amd", "lib")
    exe = str(tmp_path / "bunny_ceres_adaptor")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "bunny_ceres_adaptor.cpp"),
                           "-o", exe, "-L", libdir, "-licp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    dump = str(tmp_path / "bunny.bin")
    with open(dump, "wb") as f:
        for k in ("src", "tgt"):
            f.write(np.int32(len(bunny[k + "_pts"])).tobytes()); f.write(bunny[k + "_pts"].astype(np.float32).tobytes())
            f.write(bunny[k + "_nrm"].astype(np.float32).tobytes()); f.write(bunny[k + "_rgba"].astype(np.uint8).tobytes())
    for metric in (0, 1, 2):
        out = subprocess.check_output([exe, dump, str(metric)], timeout=300).decode().splitlines()
        st = dict(zip(out[-2].split()[0::2], out[-2].split()[1::2]))
        assert st["status"] == "0" and st["iterations"] == "20" and st["summaries"] == "20" and st["converged"] == "20"
        pose = np.array([float(v) for v in out[-1].split()[1:]], np.float32).reshape(4, 4)
        ref = make_ctx(gpu_ctx_factory, bunny_pair(bunny), metric)
        pose_ref, _, _ = ref.run(np.eye(4, dtype=np.float32))
        assert np.array_equal(pose, pose_ref), (metric, pose, pose_ref)
