"""GICP, colored ICP and robust mode on every form of sub-sampled query set the loop has, iteration by iteration against
tests/query_set_reference.py: the iteration on a level, a list or a Morton-sorted copy must be the restatement's step on the ORIGINAL
source rows of the set, whatever chain of indices (slot -> selection list -> sorted position -> original index) the kernels fetch the
source's attributes through.

Teacher-forced: iteration i's reference step starts from the device's own pose after iteration i - 1, on rows S_i of the full-resolution
records a second context (same clouds and parameters, multires and selection off, robust mode off) gives at that pose.  The source is
shuffled, so a kernel that reads a point's GICP normal, colour or normal at the slot or at the sorted position reads another point's;
every proper subset also asserts that the reference itself tells the two apart by 100 tolerances (wrong_slot_step), a statement about the
inputs alone."""
import numpy as np
import pytest

import query_set_reference as Q
from support import check_stats, load, restated_step, u32

pytestmark = pytest.mark.gpu
f32 = np.float32
N_ITER, PROBA, SEED = 4, 0.5, 7

# id: (multires, selection, nss resample, knn_backend)        what the loop hands the post stage
FORMS = {
    "sorted_levels": (1, 0, None, 1),                         # Morton-sorted copies + src_orig
    "list_levels": (1, 0, None, 0),                           # stride lists
    "random_lists": (0, 1, None, 1),                          # a list per iteration
    "random_on_levels": (1, 1, None, 0),                      # lists drawn from levels
    "nss_held": (1, 2, 0, 1),                                 # held sorted levels
    "nss_redrawn": (1, 2, 1, 1),                              # lists per iteration
}


@pytest.fixture(scope="module")
def clouds(bunny):
    return dict(bunny=Q.shuffled(bunny), rgbd=Q.shuffled(Q.rgbd_pair()))


def configure(ctx, cfg, form=None, robust=True, lm=False):          # not support.configure: driven by a cfg dict, sets the mode's options too
    multires, selection, resample, knn_backend = FORMS[form] if form else (0, 0, None, 1)
    p = ctx.params
    p.metric, p.weighting, p.rejection, p.color_icp, p.matching, p.knn_backend = cfg["metric"], cfg["weighting"], cfg["rejection"], 0, 0, knn_backend
    p.n_iterations, p.max_distance = N_ITER, cfg["max_distance"]
    p.multires, p.selection, p.selection_proba, p.selection_seed = multires, selection, PROBA, SEED
    ctx.push_params()
    if resample is not None:
        ctx.set_nss_options(5, bool(resample))
    if cfg["mode"] == "gicp":
        ctx.set_gicp_options(Q.EPS, cfg["covariance_k"])
    if cfg["mode"] == "colored":
        ctx.set_colored_options(Q.LAM, cfg["gradient_k"])
    if cfg["mode"] == "robust" and robust:
        ctx.set_robust_options(**cfg["robust"])
    if lm:
        ctx.set_optimizer(True)


def check_form(ctx, form, recs, factors, sets, n):
    """What can be seen from outside of the form a run took: the levels change under multires, a selection exists or not, a list per
    iteration differs from its neighbour, the merged point-to-plane loop was not taken.  (Whether a level was a sorted copy or a list is
    not observable through the C ABI; the two backends that decide it are both in FORMS.)"""
    from icp_amd import binding
    import support as M
    multires, selection, resample, knn_backend = FORMS[form]
    sizes = [r["n_src"] for r in recs]
    if multires:
        assert len(set(sizes)) > 1 and factors[-1] == 1 and factors[0] > 1 and sorted(factors, reverse=True) == factors
    else:
        assert set(factors) == {0}
    if selection == 0:
        assert sizes[-1] == n
        with pytest.raises(binding.IcpError):
            ctx.selection(0)
    else:
        assert all(0 < len(S) < n for S in sets)
        if not multires:
            assert all(not np.array_equal(a, b) for a, b in zip(sets, sets[1:]))
    assert M.counters(ctx) == (0, 0)


@pytest.mark.parametrize("mode", sorted(Q.MODES))
@pytest.mark.parametrize("form", sorted(FORMS))
def test_iterations_equal_the_reference_on_the_original_rows(gpu_ctx_factory, clouds, form, mode):
    cfg = Q.MODES[mode]
    d = clouds[cfg["cloud"]]
    n = len(d["src_pts"])
    ctx, base = gpu_ctx_factory(), gpu_ctx_factory()
    configure(ctx, cfg, form); load(ctx, d)
    configure(base, cfg, None, robust=False); load(base, d)
    eye = np.eye(4, dtype=f32)
    pose, recs, rc = ctx.run(eye)
    stats = ctx.robust_stats()
    factors, sets = Q.iteration_sets(ctx, d["src_pts"], d["src_nrm"])
    assert rc == 0 and len(recs) == len(sets) >= N_ITER and len(stats) == (len(recs) if cfg["mode"] == "robust" else 0)
    check_form(ctx, form, recs, factors, sets, n)
    data = dict(d)
    if cfg["mode"] == "gicp":
        data["gicp_src"], data["gicp_tgt"] = ctx.gicp_normals("source"), ctx.gicp_normals("target")
        assert np.array_equal(u32(data["gicp_src"]), u32(base.gicp_normals("source")))
    if cfg["mode"] == "colored":
        data["grad"] = ctx.color_gradients()
    opts = Q.step_options(cfg, transform_points=ctx.transform_points, transform_normals=ctx.transform_normals)
    prev = eye
    for i, r in enumerate(recs):
        S = sets[i]
        full, _, _ = base.correspond(prev)
        ref = Q.expected_step(cfg["mode"], S, prev, full[S], data, opts)
        err = float(np.abs(r["pose"].astype(np.float64) - ref["pose"]).max())
        line = "%s / %s iteration %d: %d points (factor %d), n_valid %d (reference %d), pose error %.3g" % (form, mode, i, len(S), factors[i], r["n_valid"], ref["n_valid"], err)
        if len(S) < n:                                        # the inputs tell a wrong-slot read apart: nothing of the device in this
            wrong = Q.wrong_slot_step(cfg["mode"], S, prev, full[S], data, opts)
            gap = float(np.abs(wrong["pose"].astype(np.float64) - ref["pose"]).max())
            print(line + ", wrong-slot gap %.3g" % gap)
            assert Q.slot_differs(S) > 0.95, line
            assert gap >= Q.MARGIN, line
        else:
            print(line)
        assert r["n_src"] == len(S) and r["status"] == 0, line
        assert r["n_valid"] == ref["n_valid"] > 0, line
        assert err <= Q.TOL, (line, r["pose"], ref["pose"])
        if cfg["mode"] == "robust":
            check_stats(stats[i], ref["stats"], line)
        prev = r["pose"]
    assert np.array_equal(u32(pose), u32(recs[-1]["pose"]))
    pose2, recs2, _ = ctx.run(eye)                            # a second run is bit-identical
    assert np.array_equal(u32(pose), u32(pose2)) and ctx.robust_stats() == stats
    assert all(np.array_equal(u32(a["pose"]), u32(b["pose"])) and (a["n_src"], a["n_valid"]) == (b["n_src"], b["n_valid"]) for a, b in zip(recs, recs2))


@pytest.mark.parametrize("form", ["nss_held", "nss_redrawn"])
def test_lm_on_normal_space_sets(gpu_ctx_factory, clouds, form):
    """The non-linear optimiser (point-to-plane) on the two normal-space forms against lm_restatement's own trajectory, iteration by
    iteration: the set of iteration i (icp_get_selection, checked against nss_restatement) becomes the source of a second context whose
    matcher the restatement queries at its own pose."""
    import lm_restatement as lm
    cfg = dict(mode="lm", metric=1, weighting=0, rejection=1, max_distance=0.0003)
    d = clouds["bunny"]
    ctx, q = gpu_ctx_factory(), gpu_ctx_factory()
    configure(ctx, cfg, form, lm=True); load(ctx, d)
    configure(q, cfg, None)
    q.set_target(d["tgt_pts"], d["tgt_nrm"], d["tgt_rgba"])
    eye = np.eye(4, dtype=f32)
    pose_dev, recs, rc = ctx.run(eye, check=False)
    sums = ctx.lm_summaries()
    factors, sets = Q.iteration_sets(ctx, d["src_pts"], d["src_nrm"])
    assert len(recs) == len(sums) == len(sets) == N_ITER and len({r["n_src"] for r in recs}) > 1
    pose = eye
    for i, S in enumerate(sets):
        assert 0 < len(S) < len(d["src_pts"]) and Q.slot_differs(S) > 0.95
        pair = dict(src_pts=d["src_pts"][S], src_nrm=d["src_nrm"][S], tgt_pts=d["tgt_pts"], tgt_nrm=d["tgt_nrm"])
        q.set_source(pair["src_pts"], pair["src_nrm"], d["src_rgba"][S])
        _, summ, _, pose = restated_step(q, pair, 1, pose)
        err = float(np.abs(recs[i]["pose"].astype(np.float64) - pose).max())
        print("%s / lm iteration %d: %d points, LM iterations %d (reference %d), pose error %.3g" % (form, i, len(S), sums[i]["iterations"], summ["iterations"], err))
        assert recs[i]["n_src"] == len(S), i
        assert recs[i]["status"] == (8 if summ["termination"] == lm.NO_RESIDUALS else 0) == 0, i
        assert (sums[i]["termination"], sums[i]["iterations"]) == (summ["termination"], summ["iterations"]), i
        assert err <= Q.TOL, (i, recs[i]["pose"], pose)
    assert rc == 0 and np.abs(pose_dev - pose).max() <= Q.TOL
    pose2, recs2, _ = ctx.run(eye, check=False)
    assert np.array_equal(u32(pose_dev), u32(pose2)) and all(np.array_equal(u32(a["pose"]), u32(b["pose"])) for a, b in zip(recs, recs2))
