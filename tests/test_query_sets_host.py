"""tests/query_set_reference.py on the CPU: the stride rule against the oracle's getCoarseResolution, the driver against the restatements'
own step functions on whole clouds (it adds no arithmetic), and the condition that keeps tests/test_gpu_query_sets.py honest -- on every
sub-sampled set a step that reads the source's attributes at the slot instead of the original index lands at least 100 tolerances away
from the right one -- with a brute-force matcher standing in for the device's."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import colored_restatement as CR
import gicp_restatement as G
import nss_restatement as nss
import query_set_reference as Q
import reciprocal_restatement as RC
import robust_restatement as R

f32 = np.float32


def small_pose():
    from icp_amd import synth
    return synth.make_pose((0.01, -0.015, 0.02), (0.002, -0.003, 0.001)).astype(f32)


@pytest.fixture(scope="module")
def clouds(bunny):
    return dict(bunny=Q.shuffled(bunny), rgbd=Q.shuffled(Q.rgbd_pair()))


def match_brute(p, tgt, max_distance, chunk=512):
    return np.concatenate([RC.match_brute(p[a:a + chunk], tgt, max_distance) for a in range(0, len(p), chunk)])


@pytest.fixture(scope="module")
def prepared(clouds, orc):
    """Per mode: the cloud with its derived per-point attributes (restated GICP normals, colour gradients) and the full-resolution records
    at the identity: brute-force matches, then the oracle's weighting and rejection."""
    eye = np.eye(4, dtype=f32)
    out = {}
    for name, cfg in Q.MODES.items():
        d = dict(clouds[cfg["cloud"]])
        if cfg["mode"] == "gicp":
            k = cfg["covariance_k"]
            d["gicp_src"] = G.normals(d["src_pts"], k)[0] if k else d["src_nrm"]
            d["gicp_tgt"] = G.normals(d["tgt_pts"], k)[0] if k else d["tgt_nrm"]
        if cfg["mode"] == "colored":
            d["grad"] = CR.gradients(d["tgt_pts"], d["tgt_nrm"], d["tgt_rgba"], cfg["gradient_k"])[0]
        p = G.transform(eye, d["src_pts"])
        recs = match_brute(p, d["tgt_pts"], cfg["max_distance"])
        m = np.zeros(len(recs), orc.MATCH_DTYPE); m["idx"] = recs["idx"]; m["weight"] = recs["weight"]
        m = orc.apply_weights(cfg["weighting"], cfg["max_distance"], p, d["tgt_pts"], d["src_nrm"], d["tgt_nrm"], d["src_rgba"], d["tgt_rgba"], m)
        if cfg["rejection"]:
            m = orc.prune(d["src_nrm"], d["tgt_nrm"], m)
        base = np.zeros(len(m), RC.MATCH_DTYPE); base["idx"] = m["idx"]; base["weight"] = m["weight"]
        assert (base["idx"] >= 0).sum() > len(base) // 4, name
        out[name] = (cfg, d, base)
    return out


def test_stride_rule_equals_the_oracle(orc, clouds):
    d = clouds["bunny"]
    pts, nrm = d["src_pts"].copy(), d["src_nrm"].copy()
    pts[8] = np.nan; nrm[24, 1] = np.inf; pts[1052, 2] = -np.inf          # members of every level / of some: dropped, the rest keep their place
    valid = np.isfinite(pts).all(1) & np.isfinite(nrm).all(1)
    for f in (8, 4, 2):
        op, on, _, oi = orc.coarse(pts, nrm, None, f)
        S = Q.level_set(valid, f)
        assert np.array_equal(S, oi) and np.array_equal(op, pts[S]) and np.array_equal(on, nrm[S])
        assert np.array_equal(S, nss.base_set(pts, nrm, f))
    assert [len(Q.level_set(np.ones(1054, bool), f)) for f in (8, 4, 2, 1, 0)] == [132, 264, 527, 1054, 1054]


def test_hash_draw_equals_the_restatement(clouds):
    from icp_amd import binding
    base = Q.level_set(np.ones(1054, bool), 2)
    for proba in (0.5, 0.25, 1.0, 0.0):
        thr, take_all = Q.hash_threshold(proba)
        want = base if take_all else base[nss.select_hash(7, 3, base).astype(np.int64) < thr]
        assert np.array_equal(Q.hash_draw(base, proba, 7, 3, binding.select_hash), want)
        assert np.array_equal(Q.hash_draw(base, proba, 7, 3, nss.select_hash), want)


def matched_rows(d, base):
    m = base["idx"] >= 0
    j = base["idx"][m]
    recs = np.zeros(int(m.sum()), RC.MATCH_DTYPE); recs["idx"] = np.arange(len(recs)); recs["weight"] = base["weight"][m]
    return m, j, recs


def test_driver_equals_gicp_step(prepared):
    pose = small_pose()
    for name in ("gicp_k10", "gicp_own_colour_weights"):
        cfg, d, base = prepared[name]
        m, j, recs = matched_rows(d, base)
        sub = dict(src_pts=d["src_pts"][m], tgt_pts=d["tgt_pts"][j], gicp_src=d["gicp_src"][m], gicp_tgt=d["gicp_tgt"][j])
        want, s = G.step(pose, sub["src_pts"], sub["tgt_pts"], sub["gicp_src"], sub["gicp_tgt"], recs["weight"], Q.EPS)
        got = Q.expected_step("gicp", np.arange(len(recs)), pose, recs, sub, Q.step_options(cfg))
        assert np.array_equal(got["pose"], want) and np.array_equal(got["sums"], s) and got["n_valid"] == int(s[0]) > 100


def test_driver_equals_colored_step(prepared):
    pose = small_pose()
    cfg, d, base = prepared["colored"]
    m, j, recs = matched_rows(d, base)
    sub = dict(src_pts=d["src_pts"][m], src_rgba=d["src_rgba"][m], tgt_pts=d["tgt_pts"][j], tgt_nrm=d["tgt_nrm"][j], tgt_rgba=d["tgt_rgba"][j],
               grad=d["grad"][j])
    want, s = CR.step(pose, sub["src_pts"], sub["tgt_pts"], sub["tgt_nrm"], sub["grad"], sub["src_rgba"], sub["tgt_rgba"], recs["weight"], Q.LAM)
    got = Q.expected_step("colored", np.arange(len(recs)), pose, recs, sub, Q.step_options(cfg))
    assert np.array_equal(got["pose"], want) and np.array_equal(got["sums"], s) and got["n_valid"] == int(s[0]) > 1000


def test_driver_equals_robust_step(prepared):
    pose = small_pose()
    cfg, d, _ = prepared["robust_huber_plane"]
    tree = cKDTree(d["tgt_pts"].astype(np.float64))
    opt = Q.step_options(cfg)["robust"]
    want, stats = R.step(pose, d["src_pts"], d["src_nrm"], d["tgt_pts"], d["tgt_nrm"], tree, cfg["max_distance"], opt)
    p = G.transform(pose, d["src_pts"])
    dist, j = tree.query(p.astype(np.float64), k=1)
    recs = np.zeros(len(p), RC.MATCH_DTYPE)
    recs["idx"] = np.where(dist * dist <= cfg["max_distance"], j, -1); recs["weight"] = 1.0
    got = Q.expected_step("robust", np.arange(len(p)), pose, recs, d, Q.step_options(cfg))
    assert np.array_equal(got["pose"], want) and got["stats"] == stats and 0 < got["n_valid"] == stats["n_kept"] < stats["n_entering"]


def test_point_to_point_step_reaches_a_known_pose(clouds):
    """The one composition the driver does not take from a restatement's step(): Procrustes (solve_reference.solve_p2p) on the kept pairs,
    then dT * pose.  Exact correspondences under a known motion, a third of them spoiled: the trim (K = ceil(fp32(0.6) * 600) = 361 of the
    400 intact pairs) leaves none of those in, and the step lands on the motion."""
    from icp_amd import synth
    d = clouds["bunny"]
    T = synth.make_pose((0.02, -0.01, 0.015), (0.001, 0.002, -0.0015))
    tgt = d["tgt_pts"][:600]
    Ti = np.linalg.inv(T)
    src = (tgt.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)
    src[::3] += f32(0.01)                                     # 200 outliers: the largest residuals
    recs = np.zeros(600, RC.MATCH_DTYPE); recs["idx"] = np.arange(600); recs["weight"] = 1.0
    cfg = Q.MODES["robust_trim_point"]
    got = Q.expected_step("robust", np.arange(600), np.eye(4, dtype=f32), recs, dict(src_pts=src, tgt_pts=tgt, tgt_nrm=d["tgt_nrm"][:600]), Q.step_options(cfg))
    assert got["n_valid"] == got["stats"]["n_kept"] == 361 and got["stats"]["n_entering"] == 600
    assert np.abs(got["pose"].astype(np.float64) - T).max() <= 1e-6


@pytest.mark.parametrize("name", sorted(Q.MODES))
def test_wrong_slot_is_told_apart(prepared, name):
    """Stride levels 8 / 4 / 2 and one hash-drawn half sample, one step from the identity: max |wrong-slot pose - expected pose| >= 1e-3.
    The margins measured here are in DESIGN.md 6o."""
    cfg, d, base = prepared[name]
    n = len(d["src_pts"])
    valid = np.ones(n, bool)
    sets = [("stride %d" % f, Q.level_set(valid, f)) for f in (8, 4, 2)]
    sets.append(("half sample", Q.hash_draw(np.arange(n), 0.5, 7, 0, nss.select_hash)))
    eye = np.eye(4, dtype=f32)
    opts = Q.step_options(cfg)
    for label, S in sets:
        assert 100 < len(S) < n and Q.slot_differs(S) > 0.95
        right = Q.expected_step(cfg["mode"], S, eye, base[S], d, opts)
        wrong = Q.wrong_slot_step(cfg["mode"], S, eye, base[S], d, opts)
        gap = float(np.abs(wrong["pose"].astype(np.float64) - right["pose"]).max())
        print("%s, %s (%d points): wrong-slot gap %.3g, n_valid %d" % (name, label, len(S), gap, right["n_valid"]))
        assert right["n_valid"] > 20 and np.isfinite(right["pose"]).all()
        assert gap >= Q.MARGIN, (name, label, gap)
