"""The host arithmetic behind the merged loop's stage times (sample_iterations + stamps_to_timing, host_loop.hpp), through the library's
internal hook icp_debug_stamp_times: hand-made stamp arrays in, icp_timing and the per-iteration arrays out.  No GPU needed.

Stamps: t0[j] / t1[j] = start / end of launch j in ticks of the device's wall clock, j = 0 .. iters, launch `iters` the closing one."""
import ctypes as C
import numpy as np
import pytest

from icp_amd import binding

f32 = np.float32


def stamp_times(t0, t1, n_done, mode, phase, ticks_per_ms):
    lib = binding.load_library()
    iters = len(t0) - 1
    assert len(t1) == iters + 1
    a0 = np.ascontiguousarray(t0, np.uint64); a1 = np.ascontiguousarray(t1, np.uint64)
    tm = binding.IcpTiming()
    m = np.full(n_done, 7, f32); p = np.full(n_done, 7, f32); s = np.full(n_done, 7, f32)
    u64p, f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    lib.icp_debug_stamp_times.argtypes = [u64p, u64p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_double, C.POINTER(binding.IcpTiming), f32p, f32p, f32p]
    lib.icp_debug_stamp_times.restype = C.c_int32
    rc = lib.icp_debug_stamp_times(a0.ctypes.data_as(u64p), a1.ctypes.data_as(u64p), iters, n_done, mode, phase, float(ticks_per_ms), C.byref(tm),
                                   m.ctypes.data_as(f32p), p.ctypes.data_as(f32p), s.ctypes.data_as(f32p))
    assert rc == 0
    return dict(match_ms=tm.match_ms, post_ms=tm.weight_reject_build_ms, solve_ms=tm.solve_ms, total_ms=tm.total_ms, iterations=tm.iterations,
                sampled=tm.sampled_iterations), m, p, s


def make_run(iters, base=0, spans=None, gap=40, closing=670):
    """Launch j starts `gap` ticks behind the end of launch j - 1 and lasts spans[j] ticks; the closing launch lasts `closing`."""
    spans = [1300 + 17 * j for j in range(iters)] if spans is None else spans
    t0, t1, t = [], [], base
    for j in range(iters + 1):
        t0.append(t); t += spans[j] if j < iters else closing; t1.append(t); t += gap
    return t0, t1, spans


def test_every_iteration_at_the_rate_given():
    for rate in (100000.0, 25000.0, 123456.0):                    # ticks per millisecond: 100 MHz, and two others no literal would fit
        t0, t1, spans = make_run(5, base=10 ** 6)
        tm, m, p, s = stamp_times(t0, t1, 5, 1, 0, rate)
        assert tm["iterations"] == 5 and tm["sampled"] == 5
        assert np.array_equal(m, f32([x / rate for x in spans])) and np.array_equal(p, f32([0] * 5))
        assert np.array_equal(s, f32([0, 0, 0, 0, 670 / rate]))
        assert tm["match_ms"] == pytest.approx(float(np.sum(m.astype(np.float64))), rel=1e-12)
        assert tm["post_ms"] == 0 and tm["solve_ms"] == pytest.approx(float(s[-1]), rel=1e-12)
        assert tm["total_ms"] == pytest.approx((t1[5] - t0[0]) / rate, rel=1e-12)


def test_differences_are_taken_in_64_bits():
    """A counter that has run for years: the stamps lie beyond 2^32 and beyond 2^53, where neither a 32-bit difference nor a conversion to
    double BEFORE the subtraction keeps single ticks."""
    for base in (2 ** 32 - 700, 2 ** 40 + 3, 2 ** 62 + 12345):
        t0, t1, spans = make_run(3, base=base, spans=[1, 1319, 100001])
        tm, m, p, s = stamp_times(t0, t1, 3, 1, 0, 100000.0)
        assert np.array_equal(m, f32([1 / 100000.0, 1319 / 100000.0, 100001 / 100000.0])), (base, m)
        assert tm["total_ms"] == pytest.approx((t1[3] - t0[0]) / 100000.0, rel=1e-12)


def test_mode_0_reports_the_total_alone():
    t0, t1, _ = make_run(4)
    tm, m, p, s = stamp_times(t0, t1, 4, 0, 3, 100000.0)
    assert tm["match_ms"] == 0 and tm["post_ms"] == 0 and tm["solve_ms"] == 0 and tm["sampled"] == 0 and tm["iterations"] == 4
    assert (m == -1).all() and (p == -1).all() and (s == -1).all()
    assert tm["total_ms"] == pytest.approx((t1[4] - t0[0]) / 100000.0, rel=1e-12)


@pytest.mark.parametrize("mode", [2, 3, 5, 17])
def test_sampling_rotates_and_scales(mode):
    iters = 12
    t0, t1, spans = make_run(iters)
    rate = 100000.0
    seen = set()
    for phase in range(2 * mode):
        tm, m, p, s = stamp_times(t0, t1, iters, mode, phase, rate)
        want = [i for i in range(iters) if (i + phase % mode) % mode == 0]
        got = np.nonzero(m >= 0)[0].tolist()
        assert got == want, (mode, phase, got)
        assert all(m[i] == -1 and p[i] == -1 and s[i] == -1 for i in range(iters) if i not in want)
        assert tm["sampled"] == len(want)
        if want:
            scale = iters / len(want)
            assert tm["match_ms"] == pytest.approx(scale * sum(spans[i] / rate for i in want), rel=1e-6)
            # the closing launch counts as the last iteration's solve, scaled like every sampled figure
            assert tm["solve_ms"] == pytest.approx(scale * 670 / rate if iters - 1 in want else 0.0, rel=1e-6)
        else:
            assert tm["match_ms"] == 0 and tm["solve_ms"] == 0
        assert tm["total_ms"] == pytest.approx((t1[iters] - t0[0]) / rate, rel=1e-12)
        seen.add(tuple(want))
    assert len(seen) == (mode if mode <= iters else iters + 1)    # every offset is taken in turn (past the run's length: each iteration alone, or none)


def test_a_sample_that_hits_no_iteration():
    t0, t1, _ = make_run(3)
    tm, m, p, s = stamp_times(t0, t1, 3, 5, 1, 100000.0)          # (i + 1) % 5 == 0 first at i = 4
    assert tm["sampled"] == 0 and tm["match_ms"] == 0 and tm["solve_ms"] == 0 and (m == -1).all() and (s == -1).all()
    assert tm["iterations"] == 3 and tm["total_ms"] > 0


def test_a_stopped_run_reports_what_ran_and_nothing_stale():
    """Ten launches enqueued, the run stopped after four iterations: the launches behind the stop drain, their matcher blocks stamp no
    end, and the end folded for them is the maximum of a stale buffer -- here from an earlier, LATER-looking run, or zero.  None of it may
    show: n_done entries, no solve (the closing launch belongs to no reported iteration), the total from the first start to the closing end."""
    iters, n_done, rate = 10, 4, 100000.0
    t0, t1, spans = make_run(iters, base=5 * 10 ** 9)
    for j in range(n_done, iters):
        t1[j] = 9 * 10 ** 12 if j % 2 else 0                     # stale / never written
    for mode, phase in ((1, 0), (2, 0), (2, 1), (3, 2)):
        tm, m, p, s = stamp_times(t0, t1, n_done, mode, phase, rate)
        want = [i for i in range(n_done) if mode == 1 or (i + phase % mode) % mode == 0]
        assert len(m) == n_done and tm["iterations"] == n_done and tm["sampled"] == len(want)
        assert np.array_equal(m[want], f32([spans[i] / rate for i in want]))
        assert (s[want] == 0).all() and tm["solve_ms"] == 0
        assert tm["match_ms"] == pytest.approx(n_done / len(want) * sum(spans[i] / rate for i in want), rel=1e-6)
        assert tm["total_ms"] == pytest.approx((t1[iters] - t0[0]) / rate, rel=1e-12) and tm["total_ms"] < 1.0


def test_arguments_are_checked():
    lib = binding.load_library()
    t0, t1, _ = make_run(2)
    with pytest.raises(AssertionError):
        stamp_times(t0, t1, 3, 1, 0, 100000.0)                    # more iterations done than planned
    with pytest.raises(AssertionError):
        stamp_times(t0, t1, 2, 1, 0, 0.0)                         # no clock rate
    assert hasattr(lib, "icp_debug_stamp_times")
