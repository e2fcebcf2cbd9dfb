"""Trimmed ICP and the robust kernels on the host side: the option and stats records, the new symbols, argument validation without a
device, the restatement's selection against np.sort and its robust factors against closed forms (tests/robust_restatement.py), and the
register / scratch budget of the new kernels (compile only)."""
import ctypes
import os
import re
import numpy as np
import pytest

import robust_restatement as R
from device_asm import device_asm, kernel_resources

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def test_structs_layout_and_defaults():
    from icp_amd import binding
    assert ctypes.sizeof(binding.IcpRobustOptions) == 16 and ctypes.sizeof(binding.IcpRobustStats) == 16
    assert [binding.IcpRobustOptions.tuning.offset, binding.IcpRobustOptions.sigma.offset, binding.IcpRobustOptions.overlap.offset] == [4, 8, 12]
    assert [binding.IcpRobustStats.n_kept.offset, binding.IcpRobustStats.trim_d2.offset, binding.IcpRobustStats.sigma.offset] == [4, 8, 12]
    lib = binding.load_library()
    o = binding.IcpRobustOptions(3, 1.0, 2.0, 0.5)
    assert lib.icp_robust_options_default(ctypes.byref(o)) == 0
    assert (o.kernel, o.tuning, o.sigma, o.overlap) == (0, 0.0, 0.0, 1.0)
    assert lib.icp_robust_options_default(None) == 1
    assert ctypes.sizeof(binding.IcpParams) == 80


def test_new_symbols_exported():
    from icp_amd import binding
    lib = binding.load_library()
    names = ("icp_robust_options_default", "icp_set_robust_options", "icp_get_robust_options", "icp_get_robust_stats")
    for name in names:
        assert name in binding.EXPORTS and hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    assert "ICP_ROBUST_TUKEY = 3" in hdr and "typedef struct icp_robust_stats" in hdr
    for name in names:
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert "setRobustOptions(int kernel, float tuning, float sigma, float overlap)" in open(os.path.join(ROOT, "include", "icp_hip_adaptor.hpp")).read()
    assert hasattr(binding.LinearICPOptimizer, "setRobustOptions") and hasattr(binding.Context, "robust_stats")


def test_null_context_and_arguments_refused():
    from icp_amd import binding
    lib = binding.load_library()
    o = binding.IcpRobustOptions(1, 0.0, 0.0, 0.5)
    st = (binding.IcpRobustStats * 2)(); n = ctypes.c_int32(0)
    assert lib.icp_set_robust_options(None, ctypes.byref(o)) == 1
    assert lib.icp_set_robust_options(None, None) == 1
    assert lib.icp_get_robust_options(None, ctypes.byref(o)) == 1
    assert lib.icp_get_robust_stats(None, st, 2, ctypes.byref(n)) == 1


def test_selection_against_sort():
    rng = np.random.default_rng(3)
    cases = [
        rng.random(1000).astype(f32),                                           # plain
        np.repeat(f32([0.1, 0.2, 0.3]), [300, 400, 300]),                      # ties across every threshold
        np.full(257, f32(0.5)),                                                 # all equal
        (np.uint32(f32(0.25).view(np.uint32)) + rng.permutation(np.arange(900, dtype=np.uint32))).view(f32),   # only the lowest bits differ
        np.concatenate([rng.random(90).astype(f32), np.full(10, np.inf, f32)]),                               # +inf keys
        f32([0.7]), f32([0.7, 0.2]),                                                                          # m = 1, m = 2
    ]
    for r2 in cases:
        k = r2.view(np.uint32)
        v = np.sort(r2.astype(np.float64))
        for ov in (1.0, 0.9, 0.7, 0.5, 0.3, 0.01):
            m, K, Km, t, med, M = R.select(k, ov)
            assert m == len(r2) and 1 <= K <= m and K == min(max(int(np.ceil(np.float64(f32(ov)) * m)), 1), m)
            assert Km == (K + 1) // 2
            assert np.uint32(t).view(f32) == v[K - 1] and np.uint32(med).view(f32) == v[Km - 1]
            assert M == int((r2.astype(np.float64) <= v[K - 1]).sum()) and M >= K
    # SKIP keys never enter; m = 0
    k = np.full(5, R.SKIP, np.uint32)
    assert R.select(k, 0.5) == (0, 0, 0, None, None, 0)
    k[2] = f32(0.5).view(np.uint32)
    assert R.select(k, 0.5)[:3] == (1, 1, 1)
    # uint32 order is numeric order for non-negative floats, +inf at the top
    x = np.sort(np.concatenate([rng.random(100).astype(f32) * f32(1e30), f32([0, np.inf, 1e-40])]))
    assert np.all(np.diff(x.view(np.uint32).astype(np.int64)) >= 0)


def test_entering_and_keys():
    p = f32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 3, 4], [1e20, 0, 0]])
    q = f32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    k, ent = R.keys(np.array([0, 0, 0, 0, -1]), p, q)
    assert list(ent) == [True, True, False, True, False]
    assert k[2] == R.SKIP and k[4] == R.SKIP and k[3].view(f32) == f32(25) and k[0] == 0
    k, _ = R.keys(np.array([0, 0]), f32([[3e19, 0, 0], [1, 1, 1]]), q[:2])
    assert k[0] == np.uint32(0x7F800000)                                         # r^2 overflows to +inf: a legal key


def test_rho_closed_forms():
    r2 = f32([0.0, 0.01, 1.0, 4.0, 25.0, np.inf])
    u = np.sqrt(r2.astype(np.float64)) / 2.0
    c = R.tuning(R.HUBER, 0)
    assert c == float(f32(1.345))
    assert np.array_equal(R.rho(R.HUBER, c, 2.0, r2), np.where(u <= c, 1.0, c / u))
    c = R.tuning(R.CAUCHY, 0)
    assert np.allclose(R.rho(R.CAUCHY, c, 2.0, r2), 1 / (1 + (u / c) ** 2), rtol=1e-15, atol=0)
    c = R.tuning(R.TUKEY, 0)
    t = R.rho(R.TUKEY, c, 2.0, r2)
    assert np.allclose(t, np.where(u < c, (1 - (u / c) ** 2) ** 2, 0.0), rtol=1e-14, atol=1e-300)
    assert t[-1] == 0 and R.rho(R.HUBER, 1.345, 2.0, r2)[-1] == 0
    for kern in (R.HUBER, R.CAUCHY, R.TUKEY):
        assert np.all(R.rho(kern, 1.0, 0.0, r2) == 1.0) and np.all(R.rho(kern, 1.0, np.inf, r2) == 1.0)
    assert np.all(R.rho(R.NONE, 1.0, 1.0, r2) == 1.0)
    assert R.tuning(R.HUBER, 3.0) == 3.0
    assert R.scale(0.5, f32(4).view(np.uint32)) == float(f32(0.5)) and R.scale(0.0, f32(4).view(np.uint32)) == 1.4826 * 2.0


def test_huber_with_large_c_keeps_the_weights():
    rng = np.random.default_rng(9)
    n = 500
    p = rng.normal(0, 1, (n, 3)).astype(f32); tgt = rng.normal(0, 1, (n, 3)).astype(f32)
    recs = np.zeros(n, dtype=[("idx", np.int32), ("weight", f32)])
    recs["idx"] = np.arange(n); recs["idx"][::7] = -1; recs["weight"] = rng.random(n).astype(f32)
    for metric in (0, 1):
        r = R.robust(recs, p, tgt, dict(kernel=R.HUBER, tuning=1e30, overlap=1.0), metric)
        assert np.array_equal(r["recs"], recs) and r["M"] == r["m"] == n - len(range(0, n, 7))
    r = R.robust(recs, p, tgt, dict(kernel=R.NONE, overlap=0.5), 1)
    kept = r["recs"]["idx"] >= 0
    assert kept.sum() == r["M"] and np.array_equal(r["recs"]["weight"], recs["weight"]) and r["stats"]["sigma"] == -1.0
    r = R.robust(recs, p, tgt, dict(kernel=R.TUKEY, overlap=0.8), 1)
    assert r["stats"]["n_kept"] == int((r["recs"]["idx"] >= 0).sum())


def test_sums_of_kept_pairs():
    rng = np.random.default_rng(4)
    n = 200
    p = rng.normal(0, 1, (n, 3)).astype(f32); tgt = rng.normal(0, 1, (n, 3)).astype(f32); tn = rng.normal(0, 1, (n, 3)).astype(f32)
    recs = np.zeros(n, dtype=[("idx", np.int32), ("weight", f32)])
    recs["idx"] = np.arange(n); recs["weight"] = 1.0
    s, _ = R.sums(0, p, tgt, recs)
    assert s[0] == n and np.allclose(s[7], n) and np.allclose(s[8:11], p.astype(np.float64).sum(0))
    s1, _ = R.sums(1, p, tgt, recs, tgt_nrm=tn)
    H, g = R.G.unpack(s1)
    assert np.all(np.linalg.eigvalsh(H) > 0)


def test_new_kernels_register_budget():
    """k_robust_*: no scratch, within 64 VGPRs (8 waves per SIMD)."""
    seen = kernel_resources(device_asm())
    rob = {n: f for n, f in seen.items() if "k_robust_" in n}
    assert len(rob) == 5, list(rob)                     # eval, select<1>, select<2>, finish, apply
    for name, f in rob.items():
        assert f["private_seg_size"] == 0 and f["num_vgpr"] <= 64, (name, f)
