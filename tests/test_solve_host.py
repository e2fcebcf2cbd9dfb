"""The linear solves on degenerate and ill-conditioned systems, on the CPU: the oracle (both solver modes) against the plain fp64 numpy
reference of tests/solve_reference.py, on every input family and in the classes defined there.  This is what keeps the oracle honest
where it is the checker of the device (tests/test_gpu_solve.py asserts the same things of the kernels).

Every case asserts the class it was DESIGNED for from the reference's own spectrum, so a case can never fall into an easier class
unnoticed, and none lies in the band around the rank cut where the rule's outcome flips on rounding.

Mode 0 of the oracle (fp32 sums and factorisations, the restatement of the reference's own arithmetic) is compared wherever fp32 can
hold the answer: classes W and T, the point-to-point classes with a unique optimum or a rank rule, the symmetric cases whose kept
pivot ratios are all >= 2e-4.  Its distance from mode 1 is the project's standing measure of the reference's rounding noise and enters
the translation tolerance of the far-offset clouds (16 x, at the source centroid).

`python tests/test_solve_host.py --measure` prints the floors that the margins of class I are derived from (solve_reference.py).
"""
import numpy as np
import pytest

import solve_reference as sr

WEIGHTINGS = (0, 1)          # constant, ICP_WEIGHT_DISTANCES (w varies from pair to pair)


def _case(orc, name, weighting):
    c = sr.make_case(name)
    s, d, w, nt, ns = sr.compacted(orc, c, weighting)
    assert len(c["src_pts"]) == c["n_valid"] + sr.N_DECOYS and (c["idx"] < 0).sum() == sr.N_DECOYS
    return c, s, d, w, nt, ns, s.astype(np.float64).mean(0)


def test_every_case_names_its_class():
    assert set(sr.PLANE_CLASS) == {n for n in sr.CASES if "plane" in sr.make_case(n)["metrics"]}
    assert set(sr.P2P_CLASS) == {n for n in sr.CASES if "p2p" in sr.make_case(n)["metrics"]}
    assert set(sr.SYM_CLASS) == {n for n in sr.CASES if "sym" in sr.make_case(n)["metrics"]}
    for table, classes in ((sr.PLANE_CLASS, "WIT"), (sr.P2P_CLASS, ("R0", "R1", "U", "I"))):
        for cls in classes:
            assert sum(v == cls for v in table.values()) >= 2, cls              # no class rests on a single case
    assert set(sr.SYM_CLASS.values()) == set("NTF")
    ladder = [sr.PLANE_CLASS["ladder_%g" % e] for e in sr.LADDER]
    assert all(ladder.count(c) >= 2 for c in "WIT")


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", [n for n in sr.CASES if n in sr.PLANE_CLASS])
def test_point_to_plane(orc, name, weighting):
    c, s, d, w, nt, ns, at = _case(orc, name, weighting)
    ref = sr.solve_plane(s, d, nt, w)
    cls = sr.classify(ref["spectrum"])
    print(name, "spectrum", ref["spectrum"], "class", cls)
    assert cls == sr.PLANE_CLASS[name]
    p1, x1 = orc.solve_p2plane(s, d, nt, w, 1); p0, x0 = orc.solve_p2plane(s, d, nt, w, 0)
    noise = sr.rot_trans_error(p0, p1, at)[1] if name in sr.FAR else 0.0
    sr.check_plane("oracle mode 1", name, cls, ref, p1.astype(np.float64), at, noise)
    if cls != "I":                      # (in class I fp32 factorisations hold nothing along the weak direction: cond x eps_f32 >= 1)
        sr.check_plane("oracle mode 0", name, cls, ref, p0.astype(np.float64), at, noise)
    if cls != "I":                      # the solution itself, before any pose rounding
        assert np.abs(x1 - ref["x"]).max() <= 1e-9, np.abs(x1 - ref["x"]).max()
    if name == "aligned":
        assert not x1.any() and np.array_equal(p1, np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", [n for n in sr.CASES if n in sr.P2P_CLASS])
def test_point_to_point(orc, name, weighting):
    c, s, d, w, nt, ns, at = _case(orc, name, weighting)
    ref = sr.solve_p2p(s, d, w)
    cls = sr.p2p_class(ref)
    print(name, "singular values", ref["sv"], "det(UV^T)", ref["det"], "class", cls)
    assert cls == sr.P2P_CLASS[name]
    if name == "mirror":
        assert ref["det"] < 0                                   # Kabsch's reflection guard is what this case is about
    if cls == "R0":
        assert np.array_equal(ref["R"], np.eye(3))
    p1 = orc.solve_p2p(s, d, w, 1); p0 = orc.solve_p2p(s, d, w, 0)
    noise = sr.rot_trans_error(p0, p1, at)[1] if name in sr.FAR else 0.0
    for label, p in (("oracle mode 1", p1), ("oracle mode 0", p0)):
        sr.check_p2p(label, name, cls, ref, p.astype(np.float64), at, noise)
    if cls in ("R0", "R1"):             # the rule is the same arithmetic on both sides: far tighter than the bar
        assert np.abs(p1[:3, :3] - ref["R"]).max() <= 4 * sr.EPS32


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", [n for n in sr.CASES if n in sr.SYM_CLASS])
def test_symmetric(orc, name, weighting):
    c, s, d, w, nt, ns, at = _case(orc, name, weighting)
    ref = sr.solve_symmetric(s, d, ns, nt, w)
    cls = sr.sym_class(ref)
    print(name, "pivot ratios", ref["ratios"], "class", cls)
    assert cls == sr.SYM_CLASS[name]
    p1, x1 = orc.solve_symmetric(s, d, ns, nt, w, 1); p0, x0 = orc.solve_symmetric(s, d, ns, nt, w, 0)
    if cls == "N":                      # tan_theta = 0 (ICPOptimizer.h:878-885): the reference's quirk, kept on purpose
        assert np.isnan(ref["pose"]).all() and np.isnan(p1).all() and np.isnan(p0).all()
        assert not x1[:3].any() and not x0[:3].any()
        return
    noise = sr.rot_trans_error(p0, p1, at)[1] if name in sr.FAR else 0.0
    sr.check_close("oracle mode 1", p1, ref["pose"], at, name in sr.FAR, noise)
    kept = ref["ratios"][ref["ratios"] > sr.CUT]
    if kept.min() >= sr.WELL:
        sr.check_close("oracle mode 0", p0, ref["pose"], at, name in sr.FAR, noise)
    assert np.abs(x1 - ref["x"]).max() <= 1e-12 / kept.min(), np.abs(x1 - ref["x"]).max()      # two fp64 factorisations: eps_f64 x condition


@pytest.mark.parametrize("mode", [1, 0])
def test_reversed_line_takes_the_half_turn(orc, mode):
    """u_1 = -v_1: the targets of a line in reverse order (forced correspondences cannot produce it: fed to the solve directly).  The
    oracle's half-turn branch against the numpy rule; the device's copy of that branch is reached by no test -- unpinned."""
    s = np.array([[1.5, 0.25, -0.5], [2.5, 0.25, -0.5], [4.0, 0.25, -0.5]], np.float32); d = s[::-1].copy(); w = np.ones(3, np.float32)
    ref = sr.solve_p2p(s, d, w)
    assert ref["rank"] == 1 and abs(ref["u"] @ ref["v"] + 1) < 1e-12
    assert np.allclose(ref["R"], np.diag([-1.0, -1.0, 1.0]))
    p = orc.solve_p2p(s, d, w, mode)
    assert np.abs(p[:3, :3] - ref["R"]).max() <= 4 * sr.EPS32 and np.abs(p.astype(np.float64) - ref["pose"]).max() <= sr.POSE_TOL


def test_minimal_rotation_rule():
    """The rank-1 rule itself: takes v to u, is the identity when nothing has to turn, a half turn about the kmin axis at u = -v, and
    does not depend on the sign of the singular pair."""
    rng = np.random.default_rng(3)
    for _ in range(50):
        v = rng.normal(size=3); v /= np.linalg.norm(v); u = rng.normal(size=3); u /= np.linalg.norm(u)
        R = sr.minimal_rotation(v, u)
        assert np.abs(R @ v - u).max() < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert np.abs(R - sr.minimal_rotation(-v, -u)).max() < 1e-12
        assert np.abs(R @ np.cross(v, u) - np.cross(v, u)).max() < 1e-12                 # the axis is v x u
        assert np.array_equal(sr.minimal_rotation(v, v), np.eye(3))
        H = sr.minimal_rotation(v, -v)
        assert np.abs(H @ v + v).max() < 1e-12 and np.abs(H @ H - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(H) - 1) < 1e-12
    assert np.allclose(sr.minimal_rotation([1, 0, 0], [-1, 0, 0]), np.diag([-1.0, -1.0, 1.0]))   # kmin: a tie between 1 and 2 picks 2


def test_angles_from_pose_round_trip():
    rng = np.random.default_rng(4)
    for _ in range(20):
        x = np.concatenate([rng.uniform(-1.2, 1.2, 3), rng.uniform(-5, 5, 3)])
        assert np.abs(sr.angles_from_pose(sr.pose_from_x(x)) - x).max() < 1e-12


def measure(orc):
    """The floors behind PLANE_I_MARGIN and P2P_I_MARGIN, and what a wrong rank decision costs."""
    for name in sr.CASES:
        for weighting in WEIGHTINGS:
            c, s, d, w, nt, ns, at = _case(orc, name, weighting)
            if sr.PLANE_CLASS.get(name) == "I":
                ref = sr.solve_plane(s, d, nt, w)
                floor = sr.excess_cost(ref, sr.angles_from_pose(sr.pose_from_x_f32(ref["x"]).astype(np.float64)))
                U, sv, Vt = np.linalg.svd(ref["A"], full_matrices=False)
                few = Vt[:5].T @ ((U[:, :5].T @ ref["b"]) / sv[:5])
                print("%-14s w=%d point-to-plane: fp32-pose floor %.3g, one direction too few costs %.3g" % (name, weighting, floor, sr.excess_cost(ref, few)))
            if sr.PLANE_CLASS.get(name) == "T":
                ref = sr.solve_plane(s, d, nt, w)
                U, sv, Vt = np.linalg.svd(ref["A"], full_matrices=False); k = int(ref["keep"].sum())
                many = Vt[:k + 1].T @ ((U[:, :k + 1].T @ ref["b"]) / sv[:k + 1])
                print("%-14s w=%d point-to-plane: one direction too many moves x by %.3g (|x_ref| = %.3g)" % (name, weighting, np.linalg.norm(many - ref["x"]), np.linalg.norm(ref["x"])))
            if sr.P2P_CLASS.get(name) == "I":
                ref = sr.solve_p2p(s, d, w)
                print("%-14s w=%d point-to-point: objective loss of Kabsch's R in fp32 %.3g" % (name, weighting, sr.p2p_objective_loss(ref, ref["R"].astype(np.float32))))
            if name in sr.FAR:
                pairs = [("p2p", orc.solve_p2p(s, d, w, 0), orc.solve_p2p(s, d, w, 1))]
                if name in sr.PLANE_CLASS:
                    pairs.append(("plane", orc.solve_p2plane(s, d, nt, w, 0)[0], orc.solve_p2plane(s, d, nt, w, 1)[0]))
                if name in sr.SYM_CLASS:
                    pairs.append(("sym", orc.solve_symmetric(s, d, ns, nt, w, 0)[0], orc.solve_symmetric(s, d, ns, nt, w, 1)[0]))
                for metric, a, b in pairs:
                    print("%-14s w=%d %s: oracle mode 0 against mode 1 at the centroid %.3g m" % (name, weighting, metric, sr.rot_trans_error(a, b, at)[1]))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    from oracle import oracle
    oracle.build()
    measure(oracle)                 # (--measure is accepted and means the same)
