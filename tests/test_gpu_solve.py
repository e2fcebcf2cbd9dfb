"""The linear solves of the device on degenerate and ill-conditioned systems, against the plain fp64 numpy reference of
tests/solve_reference.py and the oracle: dev_solve.hpp's eigen path and its (6 eps_f32)^2 cut, the guard that decides between LDL^T and
that path (and whether a merged run is abandoned), procrustes_rotation's rank rule and reflection guard, the full-pivot LU's rank rule,
the symmetric metric's division by tan_theta = 0, the moment expansion of the Procrustes matrix far from the origin.

Every case forces its correspondences (targets >= 0.5 m apart, each source next to its own target, decoys that must stay unmatched) and
first asserts that icp_correspond found exactly those, so no case can quietly turn into a different system; then its class is asserted
from the REFERENCE's spectrum (tests/test_solve_host.py does the same for the oracle, without a GPU).  The solve is reached through
icp_correspond (sums), icp_iterate, icp_run with 1 and 4 iterations on both k-NN backends, point-to-plane in both loop forms (bit-identical,
and the fallback counter says which route was taken), and icp_run_multistart (the COPY = 1 instantiation of the whole solve).

Margins of class I: solve_reference.PLANE_I_MARGIN / P2P_I_MARGIN (measured on the CPU: `python tests/test_solve_host.py --measure`)."""
import numpy as np
import pytest

import solve_reference as sr
from support import make_ctx, counters, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
BRUTE, LBVH = 0, 1
METRIC = {"p2p": 0, "plane": 1, "sym": 2}
WEIGHTINGS = (0, 1)
ICP_OK, NO_CORRESPONDENCES = 0, 8


@pytest.fixture(scope="module")
def ctxs(gpu_ctx_factory):
    """One context per (k-NN backend, loop form), shared by the cases of this module: the clouds and parameters are set per case."""
    made = {}

    def get(backend, form="separate"):
        if (backend, form) not in made:
            made[(backend, form)] = make_ctx(gpu_ctx_factory, form)
        return made[(backend, form)]
    yield get
    for c in made.values():
        c.close()


def setup(c, case, metric, backend, weighting, n_iterations=1):
    c.params.knn_backend = backend; c.params.metric = METRIC[metric]; c.params.weighting = weighting; c.params.rejection = 0
    c.params.max_distance = sr.MAX_DISTANCE; c.params.n_iterations = n_iterations; c.params.multires = 0
    c.push_params()
    c.set_target(case["tgt_pts"], case["tgt_nrm"]); c.set_source(case["src_pts"], case["src_nrm"])
    return c


def reference_of(orc, case, metric, weighting):
    s, d, w, nt, ns = sr.compacted(orc, case, weighting)
    at = s.astype(np.float64).mean(0)
    if metric == "plane":
        ref = sr.solve_plane(s, d, nt, w); cls = sr.classify(ref["spectrum"]); want = sr.PLANE_CLASS[case["name"]]
        o1, o0 = orc.solve_p2plane(s, d, nt, w, 1)[0], orc.solve_p2plane(s, d, nt, w, 0)[0]
    elif metric == "p2p":
        ref = sr.solve_p2p(s, d, w); cls = sr.p2p_class(ref); want = sr.P2P_CLASS[case["name"]]
        o1, o0 = orc.solve_p2p(s, d, w, 1), orc.solve_p2p(s, d, w, 0)
    else:
        ref = sr.solve_symmetric(s, d, ns, nt, w); cls = sr.sym_class(ref); want = sr.SYM_CLASS[case["name"]]
        o1, o0 = orc.solve_symmetric(s, d, ns, nt, w, 1)[0], orc.solve_symmetric(s, d, ns, nt, w, 0)[0]
    assert cls == want, (case["name"], metric, cls, want)
    noise = sr.rot_trans_error(o0, o1, at)[1] if case["name"] in sr.FAR and cls != "N" else 0.0
    return ref, cls, o1.astype(np.float64), at, noise


def check_pose(label, case, metric, cls, ref, o1, at, noise, pose):
    """One solve of the device (the pose after ONE iteration from the case's incoming pose) against the reference and the oracle."""
    name = case["name"]
    if cls == "N":
        assert np.isnan(pose).all(), (label, pose)
        return
    dT = sr.delta_pose(pose, case["pose"])
    if metric == "plane":
        sr.check_plane(label + " / reference", name, cls, ref, dT, at, noise)
    elif metric == "p2p":
        sr.check_p2p(label + " / reference", name, cls, ref, dT, at, noise)
    else:
        sr.check_close(label + " / reference", dT, ref["pose"], at, name in sr.FAR, noise)
    if cls != "I":
        sr.check_close(label + " / oracle mode 1", dT, o1, at, name in sr.FAR, noise)


CASES = [(n, m) for n in sr.CASES for m in ("p2p", "plane", "sym") if n in {"p2p": sr.P2P_CLASS, "plane": sr.PLANE_CLASS, "sym": sr.SYM_CLASS}[m]]


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name,metric", CASES)
def test_sums_and_one_solve(ctxs, orc, name, metric, weighting):
    """icp_correspond (forced matches, the 64 sums against fp64 numpy at rtol 1e-11), icp_iterate and icp_run with one iteration, on both
    k-NN backends.  Sum layout: DESIGN.md, "The solve on degenerate systems"."""
    case = sr.make_case(name)
    ref, cls, o1, at, noise = reference_of(orc, case, metric, weighting)
    for backend in (BRUTE, LBVH):
        c = setup(ctxs(backend), case, metric, backend, weighting)
        m, sums, nv = c.correspond(case["pose"])
        assert np.array_equal(m["idx"], case["idx"]) and nv == case["n_valid"], (backend, m["idx"])
        want = ref["sums"]
        assert np.allclose(sums[:7], want[:7], rtol=1e-13, atol=0), (backend, sums[:7], want[:7])
        k = 23 if metric == "p2p" else 34
        # rtol 1e-11 on every entry; on top of it only what the rounding of the sum itself allows: 1e-13 of the sum of the ABSOLUTE terms
        # (64 terms x eps_f64 = 7e-15).  Where all terms have one sign that is nothing beside the rtol; where they cancel -- exactly, in
        # the dyadic cases, whose reference entry is 0 -- it is the only scale there is.
        err = np.abs(sums[7:k] - want[7:k]); bound = 1e-11 * np.abs(want[7:k]) + 1e-13 * ref["sums_abs"][7:k]
        print("backend %d sums: largest error / bound %.3g" % (backend, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (backend, sums[7:k], want[7:k])
        pose, st = c.iterate(case["pose"])
        assert st["status"] == ICP_OK and st["n_valid"] == case["n_valid"] and st["n_src"] == len(case["src_pts"])
        assert np.array_equal(st["pose"], pose, equal_nan=True)
        check_pose("iterate, backend %d" % backend, case, metric, cls, ref, o1, at, noise, pose)
        rpose, recs, rc = c.run(case["pose"], check=False)
        assert rc == ICP_OK and len(recs) == 1 and recs[0]["n_valid"] == case["n_valid"] and recs[0]["status"] == ICP_OK
        check_pose("run(1), backend %d" % backend, case, metric, cls, ref, o1, at, noise, rpose)
    # (Both backends find the same matches, but their kernels fold the sums in different orders: the sums agree to rounding, not bit for
    # bit, and on a rank-deficient system the components that should be exactly zero come out as different 1e-17s.  Each backend is
    # held to the reference above.)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name,metric", CASES)
def test_four_iterations_follow_the_oracle(ctxs, orc, name, metric, weighting):
    """icp_run with four iterations: every later iteration starts from the pose a degenerate solve left.  Against the oracle's loop in
    mode 1 at the project's bar (1e-5), iteration by iteration, wherever one solve is comparable (every class but I: there the pose must
    stay a finite rigid motion).  Far-offset clouds: 3000 m out one ulp of a transformed fp32 point is 2.4e-4 m, so a pose that differs in
    its last bit re-rounds every point of a +-1 m cloud and the NEXT solve turns by 1e-5 rad or more -- the oracle's own two modes end
    2e-5 .. 4e-5 rad and 2e-4 .. 5e-4 m apart there after two iterations (1e-6 rad at 300 m).  Their distance at the same iteration,
    rotation and translation, is the noise measure of these cases from the second iteration on: 1e-5 plus 16 x it (sizes: DESIGN.md 6h).  Class I is held to rigidity
    only: one solve's weak direction is already not comparable, and nothing downstream of it is.  Symmetric at tan_theta = 0: the NaN pose is reported with ICP_OK and the true n_valid, and the NEXT
    iteration finds no correspondence -- it neither hangs nor faults."""
    case = sr.make_case(name)
    ref, cls, o1, at, noise = reference_of(orc, case, metric, weighting)
    runs = []
    for backend in (BRUTE, LBVH):
        c = setup(ctxs(backend), case, metric, backend, weighting, n_iterations=4)
        pose, recs, rc = c.run(case["pose"], check=False)
        runs.append((pose, recs, rc))
    for a, b in zip(runs[0][1], runs[1][1]):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"])
    reco = None
    if cls not in ("N", "I"):
        prm = orc.make_params(metric=METRIC[metric], weighting=weighting, rejection=0, n_iterations=4, max_distance=sr.MAX_DISTANCE, solver_mode=1)
        zc = np.zeros((len(case["src_pts"]), 4), np.uint8); zt = np.zeros((len(case["tgt_pts"]), 4), np.uint8)
        po, reco = orc.estimate_pose(prm, case["src_pts"], case["src_nrm"], zc, case["tgt_pts"], case["tgt_nrm"], zt, case["pose"])
        assert len(reco) == 4
        noises = [(0.0, 0.0)] * 4
        if name in sr.FAR:                                  # (the first iteration gets no rotation allowance: it starts from the same pose bits)
            prm.solver_mode = 0
            reco0 = orc.estimate_pose(prm, case["src_pts"], case["src_nrm"], zc, case["tgt_pts"], case["tgt_nrm"], zt, case["pose"])[1]
            noises = [sr.rot_trans_error(a["pose"], b["pose"], at) for a, b in zip(reco0, reco)]
            noises[0] = (0.0, noises[0][1])
    for backend, (pose, recs, rc) in zip((BRUTE, LBVH), runs):
        assert len(recs) == 4 and recs[0]["n_valid"] == case["n_valid"] and recs[0]["status"] == ICP_OK
        if cls == "N":
            assert np.isnan(recs[0]["pose"]).all()
            assert [r["status"] for r in recs[1:]] == [NO_CORRESPONDENCES] * 3 and all(r["n_valid"] == 0 for r in recs[1:])
            assert rc == NO_CORRESPONDENCES and np.isnan(pose).all()
            continue
        assert rc == ICP_OK and np.isfinite(pose).all()
        if cls == "I":
            for r in recs:
                assert r["status"] == ICP_OK and sr.rigid_defect(r["pose"].astype(np.float64)) <= 4 * sr.RIGID_TOL, r      # (four composed poses)
            continue
        for i, (a, b) in enumerate(zip(recs, reco)):
            assert a["n_valid"] == b["n_valid"], i
            sr.check_close("backend %d, iteration %d" % (backend, i), sr.delta_pose(a["pose"], case["pose"]), sr.delta_pose(b["pose"], case["pose"]), at, name in sr.FAR, noises[i][1], noises[i][0])


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", [n for n in sr.CASES if n in sr.PLANE_CLASS])
def test_point_to_plane_loop_forms(ctxs, orc, name, weighting):
    """Merged and separate launches stay bit-identical, and the fallback counter says which route the solve took: a system whose
    spectrum the rank rule truncates (class T) leaves the merged form exactly once per run of two or more iterations, a well-posed one (W) never; in class I either
    route is right (the guard is conservative: it sends systems with sigma_min / sigma_max below 4.3e-6 .. 7.2e-7 to the eigen path, which
    keeps their directions all the same), but it is the same route on every run."""
    case = sr.make_case(name)
    cls = sr.PLANE_CLASS[name]
    out = {}
    for form in ("separate", "merged"):
        c = ctxs(LBVH, form)
        before = counters(c)
        res = []
        for n_it in (1, 4, 4):
            setup(c, case, "plane", LBVH, weighting, n_iterations=n_it)
            pose, recs, rc = c.run(case["pose"], check=False)
            res.append((pose, recs, rc))
        after = counters(c)
        out[form] = (res, (after[0] - before[0], after[1] - before[1]))
    for (pa, ra, rca), (pb, rb, rcb) in zip(out["separate"][0], out["merged"][0]):
        assert rca == rcb == ICP_OK and same_bits(pa, pb) and len(ra) == len(rb)
        for a, b in zip(ra, rb):
            assert (a["n_valid"], a["status"], a["n_src"]) == (b["n_valid"], b["status"], b["n_src"]) and same_bits(a["pose"], b["pose"])
    assert same_bits(out["merged"][0][1][0], out["merged"][0][2][0])
    assert out["separate"][1] == (0, 0)
    runs, fallbacks = out["merged"][1]
    print(name, cls, "merged runs", runs, "fallbacks", fallbacks)
    assert runs == 2                       # (a run of ONE iteration has no second launch for its reducer to ride in: run_loop takes the separate form)
    assert fallbacks == {"T": 2, "W": 0}.get(cls, fallbacks) and fallbacks in (0, 2)


MULTISTART = [(n, m) for n, m in CASES if n in ("one", "two", "three", "collinear64", "planar", "offset_3000", "aligned", "control", "coincident16",
                                                 "ladder_0.0001", "ladder_1e-06", "mirror", "collinear_far")]      # one or two cases of every family


@pytest.mark.parametrize("name,metric", MULTISTART)
def test_multistart_runs_the_same_solve(ctxs, name, metric):
    """icp_run_multistart (its own instantiation of the whole solve) with the degenerate start among its starts: bit-identical to
    icp_run from each start."""
    case = sr.make_case(name)
    c = setup(ctxs(LBVH), case, metric, LBVH, 1, n_iterations=3)
    nudge = np.eye(4, dtype=f32); nudge[:3, 3] = [0.004, -0.002, 0.003]
    starts = [case["pose"], (nudge.astype(np.float64) @ case["pose"].astype(np.float64)).astype(f32)]
    res, stats, best = c.run_multistart(starts)
    for k, s0 in enumerate(starts):
        pose, recs, rc = c.run(s0, check=False)
        assert res[k]["status"] == rc and np.array_equal(res[k]["pose"], pose, equal_nan=True), k
        assert len(stats[k]) == len(recs) == 3
        for a, b in zip(stats[k], recs):
            assert (a["n_src"], a["n_valid"], a["status"]) == (b["n_src"], b["n_valid"], b["status"]) and np.array_equal(a["pose"], b["pose"], equal_nan=True)
    assert stats[0][0]["n_valid"] == case["n_valid"]


def _extension_ctx(factory, metric, backend, case):
    c = factory()
    p = c.params
    p.metric, p.knn_backend, p.weighting, p.rejection, p.max_distance, p.n_iterations, p.multires = metric, backend, 1, 0, sr.MAX_DISTANCE, 1, 0
    c.push_params()
    return c


def _check_minimum_norm_step(label, c, case, s_ref, sums, sa, x_ref, compose):
    """Sums as the metric's own teacher-forced test compares them; the 6 x 6 system must be rank-deficient by the reference rule (class T);
    icp_iterate's pose within 1e-5 of the restatement's minimum-norm step, nothing along the dropped directions."""
    err = np.abs(sums[1:34] - s_ref[1:34]) / (sa[1:34] + 1e-300)
    assert sums[0] == s_ref[0] == 1 and err.max() <= 1e-9, (label, sums[:34], s_ref)
    H = np.zeros((6, 6)); H[np.triu_indices(6)] = s_ref[7:28]; H = H + np.triu(H, 1).T
    ev, V = np.linalg.eigh(H)
    ratios = np.sqrt(np.maximum(ev[::-1], 0.0) / ev.max())
    print(label, "spectrum", ratios)
    assert sr.classify(ratios) == "T"
    pose_dev, st = c.iterate(case["pose"])
    assert st["status"] == ICP_OK and st["n_valid"] == 1
    pose_ref = compose(x_ref, case["pose"])
    print(label, "max |pose - restatement|", np.abs(pose_dev - pose_ref).max())
    assert np.abs(pose_dev - pose_ref).max() <= sr.POSE_TOL, (label, pose_dev, pose_ref)
    dropped = V[:, ev <= (sr.CUT / 2) ** 2 * ev.max()]
    leak = float(np.abs(dropped.T @ sr.angles_from_pose(sr.delta_pose(pose_dev, case["pose"]))).max())
    print(label, "dropped directions carry", leak)
    assert dropped.shape[1] >= 3 and leak <= sr.POSE_TOL, (label, leak)


@pytest.mark.parametrize("backend", [BRUTE, LBVH])
def test_gicp_one_correspondence(gpu_ctx_factory, backend):
    """Generalized-ICP with ONE valid pair: H = J^T M J has rank 3, the solve (point-to-plane's: rank guard, then the eigen path) must
    return the minimum-norm step of gicp_restatement (solve(lstsq=True): the same (6 eps_f32)^2 eigenvalue cut in numpy)."""
    import gicp_restatement as G
    eps = 1e-3
    case = sr.make_case("one")
    c = _extension_ctx(gpu_ctx_factory, 3, backend, case)
    c.set_gicp_options(eps, 0)                                   # covariance_k = 0: the clouds' own normals
    c.set_target(case["tgt_pts"], case["tgt_nrm"]); c.set_source(case["src_pts"], case["src_nrm"])
    recs, sums, nv = c.correspond(case["pose"])
    assert np.array_equal(recs["idx"], case["idx"]) and nv == 1
    p = c.transform_points(case["src_pts"], case["pose"]); b = c.transform_normals(c.gicp_normals("source"), case["pose"])
    j = np.maximum(recs["idx"], 0)
    s_ref, sa = G.sums(p, case["tgt_pts"][j], c.gicp_normals("target")[j], b, recs["weight"], eps, recs["idx"] >= 0)
    _check_minimum_norm_step("gicp", c, case, s_ref, sums, sa, G.solve(s_ref, lstsq=True), G.compose)
    c.close()


@pytest.mark.parametrize("backend", [BRUTE, LBVH])
def test_colored_one_correspondence(gpu_ctx_factory, backend):
    """Colored ICP with ONE valid pair on a textured plane (the target keeps its 64 points: the colour gradients need neighbours): two
    residuals, H of rank <= 2, against colored_restatement's minimum-norm step (lstsq=True)."""
    import colored_restatement as CR
    lam = 0.968
    plane = sr.make_case("planar")
    keep = np.concatenate([[27], np.flatnonzero(plane["idx"] < 0)])
    case = dict(plane, src_pts=plane["src_pts"][keep], src_nrm=plane["src_nrm"][keep], idx=plane["idx"][keep], n_valid=1)

    def tex(xy):
        g = np.clip(np.round(255.0 * (0.5 + 0.25 * np.sin(xy[:, 0] * 1.3) + 0.2 * np.cos(0.6 * xy[:, 0] + xy[:, 1]))), 0, 255).astype(np.uint8)
        return np.stack([g, g, g, np.full_like(g, 255)], 1)
    trgba, srgba = tex(case["tgt_pts"]), tex(case["src_pts"])
    c = _extension_ctx(gpu_ctx_factory, 4, backend, case)
    c.set_colored_options(lam, 10)
    c.set_target(case["tgt_pts"], case["tgt_nrm"], trgba); c.set_source(case["src_pts"], case["src_nrm"], srgba)
    recs, sums, nv = c.correspond(case["pose"])
    assert np.array_equal(recs["idx"], case["idx"]) and nv == 1
    grad = c.color_gradients()
    assert np.isfinite(grad[case["idx"][0]]).all() and np.any(grad[case["idx"][0]] != 0)
    s_ref, sa = CR.record_sums(recs, case["pose"], case["src_pts"], case["tgt_pts"], case["tgt_nrm"], grad, srgba, trgba, lam)
    H, g = CR.unpack(s_ref)
    _check_minimum_norm_step("colored", c, case, s_ref, sums, sa, np.linalg.lstsq(H, g, rcond=1e-10)[0], CR.compose)
    c.close()
