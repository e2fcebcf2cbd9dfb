"""The merged loop's stage times from the device's clock, and a merged run with nothing on the stream but its launches (RingStamps in
dev_solve.hpp, enqueue_merged / stamps_to_timing in host_loop.hpp).

What is checked: the timing mode changes no result (the stamps ride in launches whose arithmetic they must not touch); the times are
consistent with each other and with the host's own clock around the call; nothing of one run's stamps reaches the next; a run that stops
early or falls back to the separate form reports what it ran; the context's pose state is left as the separate form leaves it.

Shapes: a matcher block takes 256 queries, the reducer blocks that fold the block-end stamps have 128 threads.  The source sizes put the
matcher grid at 1, 2, 128, 129 and 257 blocks, one query short of, at and one query past each edge (the last one a block more)."""
import ctypes as C
import time
import numpy as np
import pytest

import support as S
from support import counters, u32

pytestmark = pytest.mark.gpu
f32 = np.float32
QPB = 256                                                     # queries per matcher block (BVH_QPB)
SIZES = [QPB * k + d for k in (1, 2, 128, 129, 257) for d in (-1, 0, 1)]
MODES = (0, 1, 2, 5)


@pytest.fixture(scope="module")
def scans():
    """One synthetic laser pair, made once: the target thinned (a small tree), the source with more points than the largest size."""
    from icp_amd import synth
    d = synth.eth_like_pair(0, n_tilt=172, n_beam=540)
    assert len(d["src_pts"]) > max(SIZES) and np.isfinite(d["src_pts"]).all() and np.isfinite(d["src_nrm"]).all()
    order = np.random.default_rng(5).permutation(len(d["src_pts"]))          # a prefix of any length covers the whole scan
    return dict(tgt=(d["tgt_pts"][::3].copy(), d["tgt_nrm"][::3].copy()), src_pts=d["src_pts"][order].copy(), src_nrm=d["src_nrm"][order].copy())


def merged_ctx(factory, scans, **params):
    c = S.make_ctx(factory, "merged", **dict(dict(max_distance=0.5, n_iterations=3), **params))
    c.set_target(*scans["tgt"])
    return c


def set_source(c, scans, n):
    c.set_source(scans["src_pts"][:n], scans["src_nrm"][:n])


def tick_ms(c):
    khz = C.c_int32(0)
    assert c.lib.icp_debug_wall_clock_khz(c.h, C.byref(khz)) == 0 and khz.value > 0
    return 1.0 / khz.value


def timed_run(c, pose):
    t = time.perf_counter()
    out = c.run(pose, check=False)
    return out, (time.perf_counter() - t) * 1e3


def check_times(c, mode, n_run, planned, host_ms, label=""):
    """Test 2's conditions on the run the context has just made: n_run iterations reported of `planned` enqueued, in timing mode `mode`."""
    tm = c.timing(); a, b, d = c.iteration_times()
    tick = tick_ms(c)
    print("%s mode %d: total %.4f ms, host %.4f ms, match sum %.4f, closing %.4f, sampled %d / %d" %
          (label, mode, tm["total_ms"], host_ms, float(a[a > 0].sum()), float(d[-1]) if len(d) else -1.0, tm["sampled_iterations"], n_run))
    assert tm["iterations"] == n_run and len(a) == len(b) == len(d) == n_run, label
    assert 0 < tm["total_ms"] <= host_ms, (label, tm, host_ms)
    if mode == 0:
        assert tm["match_ms"] == 0 and tm["solve_ms"] == 0 and tm["sampled_iterations"] == 0 and (a == -1).all() and (d == -1).all(), (label, tm)
        return set()
    sampled = set(np.nonzero(a > 0)[0].tolist())
    assert ((a > 0) | (a == -1)).all() and (a > 0).sum() + (a < 0).sum() == n_run, (label, a)
    assert tm["sampled_iterations"] == len(sampled), (label, tm)
    if mode == 1:
        assert len(sampled) == n_run, (label, a)
    else:                                                        # every mode-th iteration of the plan, from some offset
        assert len({i % mode for i in sampled}) <= 1, (label, mode, a)
        assert len(sampled) in (n_run // mode, (n_run + mode - 1) // mode), (label, mode, a)
    closing = float(d[n_run - 1]) if (n_run - 1) in sampled and n_run == planned else 0.0
    if (n_run - 1) in sampled and n_run == planned:
        assert closing > 0, (label, d)                           # the closing launch, behind the last iteration of a run that ran them all
    # the spans are disjoint intervals inside the run: one tick of slack for each launch's pair of clock reads
    assert float(a[a > 0].astype(np.float64).sum()) + closing <= tm["total_ms"] + (planned + 1) * tick, (label, a, d, tm)
    if len(sampled):
        scale = n_run / len(sampled)
        assert abs(tm["match_ms"] - scale * float(a[a > 0].astype(np.float64).sum())) <= 1e-6 * tm["match_ms"] + 1e-9, (label, tm, a)
    return sampled


@pytest.mark.parametrize("n", SIZES)
def test_results_do_not_depend_on_the_timing_mode(gpu_ctx_factory, scans, n):
    c = merged_ctx(gpu_ctx_factory, scans)
    set_source(c, scans, n)
    T0 = S.rand_pose(n, 0.02, 0.05)
    for iters in (2, 3, 7):
        c.params.n_iterations = iters; c.push_params()
        ref = None
        for mode in MODES:
            before = counters(c)
            c.set_stage_timing(mode)
            (pose, recs, rc), host_ms = timed_run(c, T0)
            assert counters(c) == (before[0] + 1, before[1]), (n, iters, mode)      # merged, no fallback
            assert rc == 0 and len(recs) == iters and all(r["n_src"] == n for r in recs) and recs[-1]["n_valid"] > 0
            check_times(c, mode, iters, iters, host_ms, "n %d iters %d" % (n, iters))
            if ref is None:
                ref = (pose, recs)
            else:
                assert np.array_equal(u32(pose), u32(ref[0])), (n, iters, mode)
                S.assert_same_run(recs, ref[1])
                assert all(np.array_equal(u32(a["pose"]), u32(b["pose"])) for a, b in zip(recs, ref[1]))
    c.close()


def test_times_are_consistent_and_the_sample_rotates(gpu_ctx_factory, scans):
    c = merged_ctx(gpu_ctx_factory, scans, n_iterations=6)
    set_source(c, scans, 33025)
    T0 = S.rand_pose(3, 0.02, 0.05)
    c.set_stage_timing(1)
    _, host_ms = timed_run(c, T0)
    assert check_times(c, 1, 6, 6, host_ms, "mode 1") == set(range(6))
    a, b, d = c.iteration_times()
    assert (a > 0).all() and d[-1] > 0 and (b == 0).all() and (d[:-1] == 0).all()
    c.set_stage_timing(3)
    seen = []
    for k in range(3):
        _, host_ms = timed_run(c, T0)
        a, _, _ = c.iteration_times()
        assert (a > 0).sum() == 2 and (a < 0).sum() == 4
        seen.append(frozenset(check_times(c, 3, 6, 6, host_ms, "mode 3 run %d" % k)))
    assert len(set(seen)) == 3, seen                             # the offset moves on with every run
    c.set_stage_timing(0)
    _, host_ms = timed_run(c, T0)
    check_times(c, 0, 6, 6, host_ms, "mode 0")
    tm = c.timing()
    assert tm["match_ms"] == 0 and tm["sampled_iterations"] == 0 and tm["total_ms"] > 0
    c.close()


def test_twenty_runs_back_to_back(gpu_ctx_factory, scans):
    """Modes and source sizes alternate on one context: a stamp block left over from the run before -- another size, another mode, another
    number of launches -- would put a time outside the run's own host interval."""
    c = merged_ctx(gpu_ctx_factory, scans)
    T0 = S.rand_pose(11, 0.02, 0.05)
    sizes = (33025, 513)
    for k in range(20):
        n = sizes[k % 2]; mode = MODES[(k // 2) % 4]; iters = 3 + (k % 3) * 2
        set_source(c, scans, n)
        c.params.n_iterations = iters; c.push_params()
        c.set_stage_timing(mode)
        (pose, recs, rc), host_ms = timed_run(c, T0)
        assert rc == 0 and len(recs) == iters
        check_times(c, mode, iters, iters, host_ms, "run %d n %d" % (k, n))
    assert counters(c) == (20, 0)
    c.close()


def test_a_run_that_stops_on_a_converged_pose(gpu_ctx_factory, bunny):
    import test_gpu_converge as G
    c = G.make_ctx(gpu_ctx_factory, "merged")
    G.load(c, bunny)
    c.set_stage_timing(1)
    ref = G.reference_run(c)
    planned = len(ref["recs"])
    opts = G.eps_of(ref)
    c.set_convergence_options(**opts)
    before = counters(c)
    (pose, recs, rc), host_ms = timed_run(c, G.EYE)
    n = len(recs)
    assert counters(c) == (before[0] + 1, before[1])             # merged, and a stop is no fault
    assert rc == 0 and 1 <= n <= planned - 3, (n, planned)       # the stop comes well before the last iteration
    cv = c.convergence()
    assert cv["converged"] and cv["iterations_run"] == n and cv["iterations_planned"] == planned
    assert all(G.same_record(a, b) for a, b in zip(recs, ref["recs"]))
    assert check_times(c, 1, n, planned, host_ms, "stopped") == set(range(n))
    a, b, d = c.iteration_times()
    assert len(a) == n and (a > 0).all() and c.timing()["total_ms"] > 0
    c.set_convergence_options(None)
    c.close()


def test_a_run_that_falls_back(gpu_ctx_factory):
    import solve_reference as sr
    case = sr.make_case("coincident16")                           # every normal equal: rank-deficient, the merged form's solve refuses it
    out = {}
    for form in ("merged", "separate"):
        c = S.make_ctx(gpu_ctx_factory, form, rejection=0, max_distance=sr.MAX_DISTANCE, n_iterations=4, multires=0)
        c.set_target(case["tgt_pts"], case["tgt_nrm"]); c.set_source(case["src_pts"], case["src_nrm"])
        c.set_stage_timing(1)
        before = counters(c)
        (pose, recs, rc), host_ms = timed_run(c, case["pose"])
        after = counters(c)
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 1) if form == "merged" else (0, 0)), (form, before, after)
        tm = c.timing(); a, b, d = c.iteration_times()
        print(form, tm, a, d)
        assert rc == 0 and len(recs) == 4 and len(a) == 4
        assert (a > 0).all() and (d > 0).all() and 0 < tm["total_ms"] <= host_ms and tm["sampled_iterations"] == 4      # the separate form's events
        out[form] = (pose, recs)
        c.close()
    assert np.array_equal(u32(out["merged"][0]), u32(out["separate"][0]))
    S.assert_same_run(out["merged"][1], out["separate"][1])


def test_the_pose_state_a_merged_run_leaves(gpu_ctx_factory, scans):
    """icp_iterate directly behind icp_run.  The merged loop never touches the context's own pose state; its first launch leaves the
    incoming pose there, where the separate form's upload would have.  Two contexts that differ in the form alone (the form is fixed when
    a context is made) must agree bit for bit on the run, on the iteration behind it, and on a second run from there."""
    out = {}
    for form in ("merged", "separate"):
        c = S.make_ctx(gpu_ctx_factory, form, max_distance=0.5, n_iterations=3)
        c.set_target(*scans["tgt"]); set_source(c, scans, 4099)
        T0 = S.rand_pose(21, 0.02, 0.05)
        pose, recs, rc = c.run(T0, check=False)
        assert rc == 0 and counters(c)[0] == (1 if form == "merged" else 0)
        p2, rec = c.iterate(pose)
        p3, recs3, rc3 = c.run(p2, check=False)
        out[form] = (pose, recs, p2, rec, p3, recs3)
        c.close()
    m, s = out["merged"], out["separate"]
    assert np.array_equal(u32(m[0]), u32(s[0])) and np.array_equal(u32(m[2]), u32(s[2])) and np.array_equal(u32(m[4]), u32(s[4]))
    S.assert_same_run(m[1], s[1]); S.assert_same_run([m[3]], [s[3]]); S.assert_same_run(m[5], s[5])
