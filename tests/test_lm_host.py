"""The non-linear optimiser without a GPU: the fp64 restatement (tests/lm_restatement.py) against finite differences and scipy, its
trust-region rules one by one, the C ABI's new types against the header, and the new kernels' register budget."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_restatement as lm          # noqa: E402
from device_asm import device_asm, kernel_resources

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MATCH = np.dtype([("idx", np.int32), ("weight", np.float32)])


def synthetic_blocks(metric, n=40, seed=0, weights=None):
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(n, 3)).astype(np.float32)
    q = (s + 0.05 * rng.normal(size=(n, 3))).astype(np.float32)
    nq = rng.normal(size=(n, 3)); nq = (nq / np.linalg.norm(nq, axis=1, keepdims=True)).astype(np.float32)
    ns = rng.normal(size=(n, 3)); ns = (ns / np.linalg.norm(ns, axis=1, keepdims=True)).astype(np.float32)
    m = np.zeros(n, MATCH); m["idx"] = np.arange(n); m["weight"] = rng.uniform(0.2, 1.0, n) if weights is None else weights
    return lm.blocks(metric, s, ns, q, nq, m)


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("x0", [(0.3, -0.2, 0.1, 0.05, -0.02, 0.03), (1e-9, -2e-9, 5e-10, 0.01, 0.0, -0.01), (0.0,) * 6])
def test_jacobian_matches_central_differences(metric, x0):
    """Both branches of AngleAxisRotatePoint (theta^2 above and below DBL_EPSILON) and all three residuals: the Jet Jacobian is the
    derivative of the residual expression itself (on the first-order branch the step stays inside that branch)."""
    b = synthetic_blocks(metric)
    x0 = np.array(x0, np.float64)
    f0, J = lm.residuals(x0, b)
    small = x0[:3] @ x0[:3] <= lm.DBL_EPS
    Jn = np.zeros_like(J)
    for k in range(6):
        h = (5e-9 if small and k < 3 else 1e-6)
        e = np.zeros(6); e[k] = h
        Jn[:, k] = (lm.residuals(x0 + e, b)[0] - lm.residuals(x0 - e, b)[0]) / (2 * h)
    assert np.allclose(J, Jn, rtol=1e-6, atol=1e-8), np.abs(J - Jn).max()
    if np.all(x0 == 0):                                 # at x = 0 the rotation columns are -[p]x (times lambda w)
        s = b["s"].astype(np.float64); lw = lm.LAMBDA_POINT * b["w"].astype(np.float64)
        n = len(s)
        assert np.allclose(J[:n, 0:3], lw[:, None] * np.stack([np.zeros(n), s[:, 2], -s[:, 1]], 1), rtol=0, atol=1e-15)


def test_lambda_is_the_widened_float():
    assert lm.LAMBDA_POINT == 0.10000000149011612


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_minimiser_reaches_scipy_minimum(metric):
    """On small synthetic problems the LM solve, run to convergence, lands where scipy's least_squares does."""
    from scipy.optimize import least_squares
    b = synthetic_blocks(metric, n=60, seed=3 + metric)
    x, summ, _ = lm.solve_blocks(b, dict(max_num_iterations=200, function_tolerance=1e-14, parameter_tolerance=1e-14))
    assert summ["termination"] == lm.CONVERGENCE
    ref = least_squares(lambda z: lm.residuals(z, b)[0], np.zeros(6), jac=lambda z: lm.residuals(z, b)[1], xtol=1e-15, ftol=1e-15, gtol=1e-15)
    assert np.allclose(x, ref.x, rtol=1e-6, atol=1e-9), (x, ref.x)
    assert summ["final_cost"] <= ref.cost * (1 + 1e-9) + 1e-18


def quad(Hm, gv, c0=1.0):
    """A quadratic with exact J^T J = Hm and gradient Hm x + gv at x: cost = c0 + g.x + 1/2 x H x."""
    Hm = np.asarray(Hm, np.float64); gv = np.asarray(gv, np.float64)
    return lambda x: (c0 + gv @ x + 0.5 * x @ Hm @ x, Hm, Hm @ x + gv)


def test_gradient_stop_at_iteration_zero():
    x, s, d = lm.solve(quad(np.eye(6), np.full(6, 1e-11)))
    assert s["termination"] == lm.CONVERGENCE and s["iterations"] == 0 and s["successful_steps"] == 1 and d == []
    assert np.all(x == 0)


def test_iteration_limit_and_radius_growth():
    """A well-posed quadratic: every step is accepted; rho = 1 triples the radius each time (capped at 1e16)."""
    H = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]) * 1e6
    x, s, d = lm.solve(quad(H, np.ones(6) * 1e6, c0=1e9), dict(max_num_iterations=3, function_tolerance=0.0, initial_trust_region_radius=1e-6))
    assert d == ["accept"] * 3 and s["termination"] == lm.NO_CONVERGENCE and s["iterations"] == 3
    assert s["successful_steps"] == 4 and s["unsuccessful_steps"] == 0
    assert np.isclose(s["trust_region_radius"], 1e-6 * 27, rtol=1e-9)


def test_rejected_steps_shrink_the_radius_by_a_growing_factor():
    """A model that promises a decrease the true cost never delivers: radius 1e4 -> /2 -> /4 -> /8."""
    H = np.eye(6); g = np.ones(6)

    def ev(x):
        c, Hm, gg = quad(H, g, 10.0)(x)
        return (10.0 + 1.0 if np.any(x) else 10.0), Hm, gg        # every candidate costs more
    x, s, d = lm.solve(ev, dict(max_num_iterations=3))
    assert d == ["reject"] * 3 and s["termination"] == lm.NO_CONVERGENCE and np.all(x == 0)
    assert s["trust_region_radius"] == 1e4 / 2 / 4 / 8 and s["unsuccessful_steps"] == 3 and s["successful_steps"] == 1


def test_decision_masks():
    """accepted_steps_mask / invalid_steps_mask: bit k - 1 for LM iteration k, in the order the iterations ran."""
    H = np.eye(6); g = np.ones(6)
    state = {"n": 0}

    def ev(x):                                        # candidates alternate: worse, better, worse, ...
        if not np.any(x):
            return 10.0, H, g
        state["n"] += 1
        return (11.0 if state["n"] % 2 else 10.0 - state["n"]), H, g
    _, s, d = lm.solve(ev, dict(max_num_iterations=4, min_relative_decrease=0.0))
    assert d == ["reject", "accept", "reject", "accept"]
    assert s["accepted_steps_mask"] == 0b1010 and s["invalid_steps_mask"] == 0
    _, s, d = lm.solve(lambda x: (1.0, -np.eye(6) * 1e3, np.ones(6)), dict(jacobi_scaling=0))
    assert s["invalid_steps_mask"] == 0b11111 and s["accepted_steps_mask"] == 0


def test_function_and_parameter_tolerance():
    _, s, d = lm.solve(lambda x: (1.0, np.eye(6), np.ones(6) * 1e-3))           # the candidate costs the same: function tolerance
    assert d == ["function_tolerance"] and s["termination"] == lm.CONVERGENCE and s["iterations"] == 1
    _, s, d = lm.solve(quad(np.eye(6) * 1e30, np.full(6, 1e-9)))                 # a step of ~1e-39 against 1e-8 (0 + 1e-8)
    assert d == ["parameter_tolerance"] and s["termination"] == lm.CONVERGENCE


def test_invalid_steps_end_in_failure_with_x_zero():
    """A non-positive damped system (or a model change <= 0) is an invalid step, treated as a rejection; five in a row is FAILURE and
    the parameters stay at 0."""
    H = -np.eye(6) * 1e3
    x, s, d = lm.solve(lambda x: (1.0, H, np.ones(6)), dict(jacobi_scaling=0))
    assert d == ["invalid"] * 5 and s["termination"] == lm.FAILURE and s["invalid_steps"] == 5 and np.all(x == 0)
    assert s["trust_region_radius"] == 1e4 / 2 / 4 / 8 / 16


def test_non_finite_start_is_failure_and_no_blocks_is_no_residuals():
    _, s, _ = lm.solve(lambda x: (np.nan, np.eye(6), np.ones(6)))
    assert s["termination"] == lm.FAILURE
    _, s, _ = lm.solve(lambda x: (0.0, np.zeros((6, 6)), np.zeros(6)), nblocks=0)
    assert s["termination"] == lm.NO_RESIDUALS


def test_block_rules():
    """Validity: idx >= 0, finite source and target points; the second block needs the finite normal(s); weight 0 still forms blocks."""
    s = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 1, 0]], np.float32)
    q = s.copy(); q[2] = 0
    nq = np.array([[0, 0, 1], [np.inf, 0, 0], [0, 0, 1], [0, 0, 1]], np.float32)
    ns = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [np.nan, 0, 1]], np.float32)
    m = np.zeros(4, MATCH); m["idx"] = [0, 1, 2, -1]; m["weight"] = [1, 0, 1, 1]
    assert lm.n_blocks(lm.blocks(0, s, ns, q, nq, m)) == 2
    assert lm.n_blocks(lm.blocks(1, s, ns, q, nq, m)) == 3
    m["idx"][3] = 3
    assert lm.n_blocks(lm.blocks(2, s, ns, q, nq, m)) == 4          # pair 3: no symmetric block (NaN source normal)
    c, H, g = lm.evaluate(np.zeros(6), lm.blocks(1, s[:2], ns[:2], q, nq, m[:2]))
    assert c == 0.0 and not np.any(g)


def test_compose_is_fp32_left_product():
    x = np.array([0.01, -0.02, 0.03, 0.1, 0.2, -0.3])
    P = np.eye(4, dtype=np.float32); P[:3, 3] = [1, 2, 3]
    out = lm.compose(x, P)
    ref = np.eye(4); ref[:3, :3] = lm.angle_axis_to_matrix(x); ref[:3, 3] = x[3:]
    assert out.dtype == np.float32 and np.allclose(out, ref @ P, atol=1e-6)
    assert np.array_equal(lm.compose(np.zeros(6), P), P)


# ---------------- C ABI ----------------
def header_layout():
    """sizeof / offsetof of the new types as a C compiler lays them out from include/icp_hip.h."""
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "icp_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(icp_params), sizeof(icp_lm_options), sizeof(icp_lm_summary),
           offsetof(icp_lm_options, max_num_iterations), offsetof(icp_lm_summary, initial_cost), offsetof(icp_lm_summary, x));
    printf("%d %d %d %d\n", ICP_LM_CONVERGENCE, ICP_LM_NO_CONVERGENCE, ICP_LM_FAILURE, ICP_LM_NO_RESIDUALS);
    return 0;
}
'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c"); exe = os.path.join(d, "l")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    return [int(v) for v in out[0].split()], [int(v) for v in out[1].split()]


def test_struct_layouts_match_header():
    from icp_amd import binding
    (sp, so, ss, o_it, o_cost, o_x), enums = header_layout()
    assert sp == 80 == ctypes.sizeof(binding.IcpParams)              # icp_params keeps its size
    assert so == ctypes.sizeof(binding.IcpLmOptions) and o_it == binding.IcpLmOptions.max_num_iterations.offset
    assert ss == ctypes.sizeof(binding.IcpLmSummary) == 104
    assert o_cost == binding.IcpLmSummary.initial_cost.offset and o_x == binding.IcpLmSummary.x.offset
    assert enums == [binding.LM_CONVERGENCE, binding.LM_NO_CONVERGENCE, binding.LM_FAILURE, binding.LM_NO_RESIDUALS]


def test_default_options_are_the_contract():
    from icp_amd import binding
    o = binding.lm_options()
    ref = lm.default_options()
    for k, v in ref.items():
        assert getattr(o, k) == v, k


def test_entry_points_without_a_device():
    """On a box without a GPU there is no context to select the optimiser on (ICP_ERR_NO_DEVICE from icp_ctx_create); the new entry
    points refuse a NULL context with ICP_ERR_INVALID_ARG and never touch a device; the options default needs none."""
    from icp_amd import binding
    lib = binding.load_library()
    h = ctypes.c_void_p()
    rc = lib.icp_ctx_create(0, ctypes.byref(h))
    if rc == 0:
        lib.icp_ctx_destroy(h)
        pytest.skip("a HIP device is visible")
    assert rc == 9 and not h.value
    o = binding.IcpLmOptions()
    assert lib.icp_lm_options_default(ctypes.byref(o)) == 0 and o.max_num_iterations == 10
    assert lib.icp_lm_options_default(None) == 1
    assert lib.icp_set_optimizer(None, ctypes.byref(o)) == 1 and lib.icp_set_optimizer(None, None) == 1
    cnt = ctypes.c_int32(-1)
    assert lib.icp_get_lm_summaries(None, None, 0, ctypes.byref(cnt)) == 1


def test_lm_kernels_register_budget():
    """k_lm_eval / k_lm_step / k_lm_init: no scratch; k_lm_eval keeps three waves per SIMD (<= 168 VGPRs) and no AGPRs.  k_lm_step is one
    wave with nothing to overlap: it may use the whole register file, AGPRs included, but never scratch."""
    seen = {n: r for n, r in kernel_resources(device_asm()).items() if "k_lm_" in n}
    assert len(seen) == 3, seen
    for name, f in seen.items():
        assert f["private_seg_size"] == 0, (name, f)
        if "k_lm_step" not in name:
            assert f["num_agpr"] == 0 and f["num_vgpr"] <= 168, (name, f)
