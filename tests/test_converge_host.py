"""Stopping on a converged pose, the parts that need no GPU: the numpy restatement (tests/converge_restatement.py) on exact rotations and
on the committed bunny oracle runs, the eligibility / patience / min_iterations arithmetic, and the C ABI of the option."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import converge_restatement as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def Rz(theta, t=(0, 0, 0)):
    T = np.eye(4)
    T[:3, :3] = [[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


def measure64(A, B):
    """The restatement's own formulas with no fp32 rounding at either end."""
    return R.measure(A, B, np.float64)


@pytest.mark.parametrize("theta", [0.0, 1e-8, 1e-5, 3e-3, 0.2, 1.0, 1.5])
def test_measure_of_an_exact_rotation_is_abs_sin_theta(theta):
    rot, tr = measure64(Rz(theta), np.eye(4))
    assert abs(rot - abs(np.sin(theta))) <= 1e-12 and tr == 0.0
    rot, _ = measure64(Rz(-theta), np.eye(4))
    assert abs(rot - abs(np.sin(theta))) <= 1e-12
    # the fp32 form: the poses themselves are rounded to fp32 first (1e-7 per entry), the measure once at the end
    rot32, tr32 = R.measure(Rz(theta), np.eye(4))
    assert rot32.dtype == f32 and abs(float(rot32) - abs(np.sin(theta))) <= 2e-7 and tr32 == 0


def test_measure_against_a_moved_pose_and_the_translation_part():
    B = Rz(0.3, (0.1, -0.2, 0.05)); D = Rz(0.01, (1e-3, 2e-3, -2e-3))
    rot, tr = measure64(D @ B, B)                               # A = D B: dR = R_D, dt = t_D
    assert abs(rot - np.sin(0.01)) <= 1e-12 and abs(tr - 3e-3) <= 1e-12
    rot32, tr32 = R.measure(D @ B, B)
    assert abs(float(rot32) - np.sin(0.01)) <= 1e-6 and abs(float(tr32) - 3e-3) <= 1e-6


def test_more_than_a_quarter_turn_is_infinite():
    assert R.measure(Rz(np.deg2rad(120)), np.eye(4))[0] == np.inf
    assert measure64(Rz(np.deg2rad(120)), np.eye(4))[0] == np.inf
    assert R.measure(Rz(np.deg2rad(91)), np.eye(4))[0] == np.inf
    assert np.isfinite(R.measure(Rz(np.deg2rad(89)), np.eye(4))[0])


def test_nan_pose_never_meets_the_criterion():
    A = np.eye(4); A[0, 0] = np.nan
    rot, tr = R.measure(A, np.eye(4))
    assert not R.met(rot, tr, dict(rotation=10, translation=10))
    A = np.eye(4); A[1, 3] = np.nan
    rot, tr = R.measure(A, np.eye(4))
    assert rot == 0 and np.isnan(tr) and not R.met(rot, tr, dict(rotation=10, translation=10))
    n, conv, trace = R.stop_index([A] * 3, np.eye(4), [0] * 3, [0] * 3, dict(rotation=10, translation=10))
    assert (n, conv) == (3, False) and [t[3] for t in trace] == [0, 0, 0]


def test_identical_poses_measure_exactly_zero():
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        w, x, y, z = q
        T = np.eye(4, dtype=f32)
        T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        rot, tr = R.measure(T, T)
        # dR = R R^T is symmetric to the bit (the same products in the same order), so its skew part is exactly zero; dt is not:
        # t - (R R^T) t carries the pose's own orthogonality error, 1e-7 |t|, hence t = 0 here
        assert rot == 0
    assert R.measure(np.eye(4), np.eye(4)) == (0, 0)
    T[:3, 3] = 0
    assert R.measure(T, T) == (0, 0)


def test_bunny_point_to_plane_run_stops_after_eight_iterations(bunny_oracle):
    P = bunny_oracle["m1_w0_r1_mode0_poses"]
    opts = dict(rotation=1e-5, translation=1e-6)
    n, conv, trace = R.stop_index(P, np.eye(4), [0] * len(P), [0] * len(P), opts)
    assert (n, conv) == (8, True) and len(trace) == 8 and trace[7][3] == 1
    # the stop point is unambiguous: an order of magnitude on both sides of both bounds
    full = R.stop_index(P, np.eye(4), [0] * len(P), [0] * len(P), dict(rotation=1e-30, translation=1e-30))[2]
    assert full[6][0] > 10 * 1e-5 and full[6][1] > 10 * 1e-6 and full[7][0] < 1e-5 and full[7][1] < 1e-6 / 2
    assert all(t[0] < 1e-5 / 10 and t[1] < 1e-6 / 10 for t in full[8:])


def test_bunny_point_to_point_run_never_stops(bunny_oracle):
    P = bunny_oracle["m0_w0_r1_mode0_poses"]
    n, conv, trace = R.stop_index(P, np.eye(4), [0] * len(P), [0] * len(P), dict(rotation=1e-5, translation=1e-6))
    assert (n, conv) == (len(P), False) and all(t[3] == 0 for t in trace)


def test_eligibility_on_a_multires_schedule():
    factors = [8, 4, 2, 1, 1, 1, 1]
    assert R.eligible(factors) == [False, False, False, False, True, True, True]
    assert R.eligible([0, 0, 0]) == [True, True, True]
    assert R.eligible([1]) == [True] and R.eligible([2, 1]) == [False, False]
    assert R.eligible([8, 4, 2, 1, 1, 1, 1], [0, 0, 0, 0, 0, 8, 0]) == [False, False, False, False, True, False, True]
    # the schedule the library computes for the bunny source (1054 points): 8, 4, 2, 1, 1 ...: first eligible index 4
    from icp_amd import binding
    p = binding.default_params(); p.multires = 1; p.n_iterations = 6
    f = binding.schedule(p, 1054)
    assert f[:5] == [8, 4, 2, 1, 1] and R.eligible(f).index(True) == 4
    still = [np.eye(4)] * len(f)
    n, conv, trace = R.stop_index(still, np.eye(4), f, [0] * len(f), dict(rotation=10, translation=10))
    assert (n, conv) == (5, True) and [t[2] for t in trace] == [0, 0, 0, 0, 1]


def test_patience_and_min_iterations_arithmetic():
    still = [np.eye(4)] * 12
    for patience in (1, 2, 3, 8):
        for min_it in (1, 2, 5, 9, 12, 20):
            n, conv, trace = R.stop_index(still, np.eye(4), [0] * 12, [0] * 12, dict(rotation=10, translation=10, patience=patience, min_iterations=min_it))
            want = max(patience, min_it)
            assert (n, conv) == ((want, True) if want <= 12 else (12, False))
            assert [t[3] for t in trace] == list(range(1, n + 1))
    # a miss or an ineligible iteration resets the streak
    moved = [Rz(0.0), Rz(0.0), Rz(0.1), Rz(0.1), Rz(0.1), Rz(0.1)]
    n, conv, trace = R.stop_index(moved, np.eye(4), [0] * 6, [0] * 6, dict(rotation=1e-3, translation=1e-3, patience=3))
    assert (n, conv) == (6, True) and [t[3] for t in trace] == [1, 2, 0, 1, 2, 3]
    n, conv, trace = R.stop_index(moved, np.eye(4), [0] * 6, [0, 0, 0, 8, 0, 0], dict(rotation=1e-3, translation=1e-3, patience=3))
    assert (n, conv) == (6, False) and [t[3] for t in trace] == [1, 2, 0, 0, 1, 2]


def test_abi_defaults_and_struct_sizes():
    from icp_amd import binding
    lib = binding.load_library()
    assert C.sizeof(binding.IcpConvergenceOptions) == 20 and C.sizeof(binding.IcpConvergenceStep) == 16 and C.sizeof(binding.IcpConvergenceResult) == 20
    assert binding.CONVERGENCE_STEP_DTYPE.itemsize == 16
    o = binding.IcpConvergenceOptions(7, 0.5, 0.5, 9, 9)
    assert lib.icp_convergence_options_default(C.byref(o)) == 0
    assert (o.enabled, o.min_iterations, o.patience) == (0, 1, 1) and o.rotation_eps > 0 and o.translation_eps > 0
    assert lib.icp_convergence_options_default(None) == 1          # ICP_ERR_INVALID_ARG
    assert lib.icp_set_convergence_options(None, C.byref(o)) == 1 and lib.icp_get_convergence(None, None) == 1


def test_header_functions_are_exported():
    from icp_amd import binding
    lib = binding.load_library()
    txt = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(icp_\w*convergence\w*)\s*\(", txt, flags=re.M))
    want = {"icp_convergence_options_default", "icp_set_convergence_options", "icp_get_convergence_options", "icp_get_convergence", "icp_get_convergence_trace"}
    assert want <= declared
    exported = set(re.findall(r" T (icp_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()))
    for name in want:
        assert name in binding.EXPORTS and hasattr(lib, name) and name in exported, name
