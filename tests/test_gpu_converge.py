"""Stopping the ICP loop on the device when the pose has converged (icp_set_convergence_options) against the numpy restatement
tests/converge_restatement.py.  Every case runs its configuration twice on one context: with the option off -- the reference, whose
recorded poses feed the restatement -- and with it on, which must stop where the restatement stops, report a bit-identical prefix of the
reference's records, end on the pose of its last record and trace the restatement's measures.

The bounds of a case are the geometric mean of two successive increments of its reference run, chosen (pick_eps) so that no increment of
that run lies within a factor 1.25 of either bound: rounding cannot decide the outcome.  Trace tolerance: the nine products of dR are
exact in fp64, what differs between the device and numpy is at most the order of a few fp64 sums and the one fp32 rounding at the end:
1e-6 relative (fp32 eps = 6e-8 and change), or 1e-12 absolute for measures that cancel to nearly nothing."""
import os
import numpy as np
import pytest

import converge_restatement as R
import support as S
from support import counters, u32

pytestmark = pytest.mark.gpu
f32 = np.float32
EYE = np.eye(4, dtype=f32)
TINY = dict(rotation=1e-30, translation=1e-30)        # never met: the restatement's measures of a whole run


def make_ctx(factory, form="merged", **params):               # this file's defaults: the bunny's threshold, 20 iterations
    return S.make_ctx(factory, form, **dict(dict(max_distance=0.0003, n_iterations=20), **params))


def load(c, d, colors=False):                                 # this file's default: no colours
    S.load(c, d, colors)


def same_record(a, b):
    return (a["n_src"], a["n_valid"], a["status"]) == (b["n_src"], b["n_valid"], b["status"]) and np.array_equal(u32(a["pose"]), u32(b["pose"])) \
        and np.array_equal(u32(f32(a["rmse"])), u32(f32(b["rmse"]))) and np.array_equal(u32(f32(a["benchmark_error"])), u32(f32(b["benchmark_error"])))


def same_dicts(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        for k in x:
            if not np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True):
                return False
    return True


def pick_eps(traces):
    """(rotation_eps, translation_eps, margin): the geometric means of two successive increments of a reference run for which the nearest
    increment of all of `traces` is farthest from either bound (as a factor).  An exact zero is below every bound."""
    def factor(x, eps):
        x = float(x)
        return np.inf if x == 0 or not np.isfinite(x) else max(x / eps, eps / x)
    best = None
    for tr in traces:
        for k in range(1, len(tr)):
            er, et = np.sqrt(float(tr[k - 1][0]) * float(tr[k][0])), np.sqrt(float(tr[k - 1][1]) * float(tr[k][1]))
            if not (np.isfinite(er) and np.isfinite(et) and er > 0 and et > 0):
                continue
            margin = min(min(factor(t[0], er), factor(t[1], et)) for t2 in traces for t in t2)
            if best is None or margin > best[2]:
                best = (er, et, margin)
    assert best is not None
    return best


def reference_run(c, pose_in=EYE):
    """The option-off run: (pose, records, status, robust stats, LM summaries, factors, restatement trace of the whole run)."""
    from icp_amd import binding
    c.set_convergence_options(None)
    pose, recs, rc = c.run(pose_in, check=False)
    cv = c.convergence()
    assert cv == dict(converged=False, iterations_run=len(recs), iterations_planned=len(recs), rotation=-1.0, translation=-1.0)
    assert len(c.convergence_trace()) == 0
    factors = binding.schedule(c.params, c.n_src)
    assert len(factors) == len(recs)
    full = R.stop_index([r["pose"] for r in recs], pose_in, factors, [r["status"] for r in recs], TINY)[2]
    return dict(pose=pose, recs=recs, rc=rc, rob=c.robust_stats(), lm=c.lm_summaries(), factors=factors, full=full)


def stopped_run(c, ref, opts, pose_in=EYE, label=""):
    """The option-on run against the restatement on the reference's records.  Returns (n_run, pose, trace, converged)."""
    c.set_convergence_options(**opts)
    o = c.convergence_options()
    assert o.enabled == 1 and o.rotation_eps == f32(opts["rotation"]) and o.translation_eps == f32(opts["translation"])
    pose, recs, rc = c.run(pose_in, check=False)
    want_n, want_conv, want_trace = R.stop_index([r["pose"] for r in ref["recs"]], pose_in, ref["factors"], [r["status"] for r in ref["recs"]], opts)
    trace = c.convergence_trace()
    print("%s: eps (%.3g, %.3g) n_run %d / %d (restatement %d), last measure (%.3g, %.3g)" %
          (label, opts["rotation"], opts["translation"], len(recs), len(ref["recs"]), want_n, trace[-1]["rotation"], trace[-1]["translation"]))
    assert len(recs) == want_n, label                                                                      # n_run == stop_index(...)
    assert all(same_record(a, b) for a, b in zip(recs, ref["recs"])), label                                # a bit-identical prefix
    assert np.array_equal(u32(pose), u32(recs[-1]["pose"])), label                                         # the pose of the last record
    firsts = [r["status"] for r in recs if r["status"] != 0]
    assert rc == (firsts[0] if firsts else 0), label                                                       # the status of the records reported
    assert same_dicts(c.robust_stats(), ref["rob"][:want_n]) and same_dicts(c.lm_summaries(), ref["lm"][:want_n]), label
    assert len(trace) == want_n, label
    for k, (t, w) in enumerate(zip(trace, want_trace)):
        for got, exp in ((t["rotation"], w[0]), (t["translation"], w[1])):
            assert got == exp or abs(float(got) - float(exp)) <= max(1e-6 * abs(float(exp)), 1e-12), (label, k, got, exp)
        assert (t["eligible"], t["streak"]) == (w[2], w[3]), (label, k)
    cv = c.convergence()
    assert (cv["converged"], cv["iterations_run"], cv["iterations_planned"]) == (want_conv, want_n, len(ref["recs"])), label
    assert u32(f32(cv["rotation"])) == u32(trace[-1]["rotation"]) and u32(f32(cv["translation"])) == u32(trace[-1]["translation"]), label
    assert c.timing()["iterations"] == want_n and all(len(a) == want_n for a in c.iteration_times()), label
    return want_n, pose, trace, want_conv


def eps_of(ref, **more):
    er, et, margin = pick_eps([ref["full"]])
    assert margin > 1.25, margin
    return dict(rotation=er, translation=et, **more)


@pytest.mark.parametrize("multires", [0, 1])
def test_point_to_plane_stops_in_the_merged_form_and_in_the_separate_form_alike(gpu_ctx_factory, bunny, multires):
    kw = dict(multires=multires, max_distance=0.001 if multires else 0.0003)
    out = {}
    for form in ("merged", "separate"):
        c = make_ctx(gpu_ctx_factory, form, **kw)
        load(c, bunny)
        ref = reference_run(c)
        opts = eps_of(ref)
        if not multires:
            assert pick_eps([ref["full"]])[2] > 10            # the bunny point-to-plane run: an order of magnitude on both sides
        before = counters(c)
        n, pose, trace, conv = stopped_run(c, ref, opts, label="p2plane %s multires %d" % (form, multires))
        assert conv and n < len(ref["recs"])
        # one more merged run and no fallback: a stop must not look like a fault
        assert counters(c) == ((before[0] + 1, 0) if form == "merged" else (0, 0))
        # ... and nothing of it is left in the ring, the state or the seeds: the plain run again
        again = reference_run(c)
        assert np.array_equal(u32(again["pose"]), u32(ref["pose"])) and all(same_record(a, b) for a, b in zip(again["recs"], ref["recs"]))
        out[form] = (n, pose, trace, opts)
        c.close()
    assert out["merged"][3] == out["separate"][3]
    assert out["merged"][0] == out["separate"][0] and np.array_equal(u32(out["merged"][1]), u32(out["separate"][1]))
    assert out["merged"][2].tobytes() == out["separate"][2].tobytes()


def test_point_to_point_never_meets_the_bounds(gpu_ctx_factory, bunny):
    c = make_ctx(gpu_ctx_factory, metric=0)
    load(c, bunny)
    ref = reference_run(c)
    opts = dict(rotation=1e-5, translation=1e-6)
    assert all(min(max(float(t[0]) / 1e-5, 1e-5 / float(t[0])), max(float(t[1]) / 1e-6, 1e-6 / float(t[1]))) > 1.25 for t in ref["full"])
    n, pose, trace, conv = stopped_run(c, ref, opts, label="p2p")
    assert not conv and n == 20 and np.array_equal(u32(pose), u32(ref["pose"]))
    c.close()


CASES = {
    "symmetric": dict(params=dict(metric=2)),
    "gicp": dict(params=dict(metric=3)),
    "colored": dict(params=dict(metric=4), colors=True),
    "robust": dict(params=dict(metric=1), robust=dict(kernel="huber", overlap=0.8)),
    "lm": dict(params=dict(metric=1, n_iterations=12), lm=True),
    "brute": dict(params=dict(metric=1, knn_backend=0)),
    "random_patience3": dict(params=dict(metric=1, selection=1, selection_proba=0.7, selection_seed=11), more=dict(patience=3)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_other_configuration_against_the_restatement(gpu_ctx_factory, bunny, case):
    cfg = CASES[case]
    c = make_ctx(gpu_ctx_factory, **cfg["params"])
    load(c, bunny, cfg.get("colors", False))
    if "robust" in cfg:
        c.set_robust_options(**cfg["robust"])
    if cfg.get("lm"):
        c.set_optimizer(True)
    ref = reference_run(c)
    assert ref["rc"] == 0
    n, pose, trace, conv = stopped_run(c, ref, eps_of(ref, **cfg.get("more", {})), label=case)
    if "robust" in cfg:
        assert len(c.robust_stats()) == n
    if cfg.get("lm"):
        assert len(c.lm_summaries()) == n
    if c.params.selection:
        assert len(c.selection(len(ref["recs"]) - 1)) > 0          # icp_get_selection keeps serving the planned draws
    assert counters(c) == (0, 0)
    c.close()


@pytest.mark.parametrize("form", ["merged", "separate"])
def test_loose_bounds_stop_at_the_first_iteration_that_may(gpu_ctx_factory, bunny, form):
    c = make_ctx(gpu_ctx_factory, form)
    load(c, bunny)
    ref = reference_run(c)
    assert all(float(t[0]) < 10 / 1.25 and float(t[1]) < 10 / 1.25 for t in ref["full"])
    for min_it, patience in ((1, 1), (3, 1), (1, 4), (5, 2), (2, 8), (20, 1), (21, 1)):
        n, _, trace, conv = stopped_run(c, ref, dict(rotation=10, translation=10, min_iterations=min_it, patience=patience), label="loose %s %d %d" % (form, min_it, patience))
        assert n == min(max(min_it, patience), 20) and conv == (max(min_it, patience) <= 20)
    c.close()
    c = make_ctx(gpu_ctx_factory, form, multires=1, max_distance=0.001)
    load(c, bunny)
    ref = reference_run(c)
    assert ref["factors"][:5] == [8, 4, 2, 1, 1]
    n, _, trace, conv = stopped_run(c, ref, dict(rotation=10, translation=10), label="loose multires " + form)
    assert n == 5 and conv and list(trace["eligible"]) == [0, 0, 0, 0, 1]         # the first eligible index is 4
    c.close()


@pytest.mark.parametrize("n_iterations", [1, 2])
def test_smallest_runs(gpu_ctx_factory, bunny, n_iterations):
    """n_iterations = 2: the smallest ring, the stop of iteration 1 travels in the closing launch; 1: no ring at all."""
    for form in ("merged", "separate"):
        c = make_ctx(gpu_ctx_factory, form, n_iterations=n_iterations)
        load(c, bunny)
        ref = reference_run(c)
        for min_it in (1, 2):
            n, pose, _, conv = stopped_run(c, ref, dict(rotation=10, translation=10, min_iterations=min_it), label="%d iterations %s" % (n_iterations, form))
            assert n == min(min_it, n_iterations) and conv == (min_it <= n_iterations)
        assert counters(c) == ((3, 0) if form == "merged" and n_iterations == 2 else (0, 0))          # (a run of one iteration has no ring)
        c.close()


def test_multistart_refuses_the_option(gpu_ctx_factory, bunny):
    from icp_amd import binding
    c = make_ctx(gpu_ctx_factory)
    load(c, bunny)
    c.set_convergence_options(rotation=1e-5, translation=1e-6)
    with pytest.raises(binding.IcpError) as ei:
        c.run_multistart([EYE, EYE])
    assert ei.value.code == 1 and "icp_set_convergence_options" in str(ei.value)
    c.set_convergence_options(None)
    assert c.convergence_options().enabled == 0
    res, _, best = c.run_multistart([EYE, EYE])
    assert len(res) == 2
    for bad in (dict(rotation=0, translation=1), dict(rotation=1, translation=float("inf")), dict(rotation=1, translation=float("nan")),
                dict(rotation=1, translation=1, min_iterations=0), dict(rotation=1, translation=1, patience=0), dict(rotation=1, translation=1, patience=9)):
        with pytest.raises(binding.IcpError) as ei:
            c.set_convergence_options(**bad)
        assert ei.value.code == 1 and "icp_set_convergence_options" in str(ei.value)
    assert c.convergence_options().enabled == 0
    c.close()


def test_batch_run_reports_each_contexts_own_run(gpu_ctx_factory, bunny):
    from icp_amd import binding
    moved = dict(bunny)
    T = np.eye(4); T[:3, 3] = [2e-4, -1e-4, 1e-4]
    moved["src_pts"] = (bunny["src_pts"].astype(np.float64) + T[:3, 3]).astype(f32)
    pairs = [bunny, moved]
    single = []
    opts = None
    for d in pairs:
        c = make_ctx(gpu_ctx_factory)
        load(c, d)
        ref = reference_run(c)
        if opts is None:
            opts = eps_of(ref)
        c.set_convergence_options(**opts)
        pose, recs, rc = c.run(EYE)
        single.append((pose, c.convergence(), c.convergence_trace()))
        c.close()
    assert single[0][1]["converged"]
    ctxs = [make_ctx(gpu_ctx_factory), make_ctx(gpu_ctx_factory)]
    for c in ctxs:
        c.set_convergence_options(**opts)
    poses, status, rc = binding.batch_run(ctxs, [dict(src_pts=d["src_pts"], src_nrm=d["src_nrm"], tgt_pts=d["tgt_pts"], tgt_nrm=d["tgt_nrm"]) for d in pairs])
    assert rc == 0
    got = [(c.convergence(), c.convergence_trace()) for c in ctxs]
    for i in range(2):
        assert np.array_equal(u32(binding.pose_to_c(single[i][0])), u32(poses[i])), i
        assert any(g[0] == single[i][1] and g[1].tobytes() == single[i][2].tobytes() for g in got), i        # (which context took which pair is the scheduler's choice)
    for c in ctxs:
        c.close()


def test_tracked_frames_stop_like_single_runs(gpu_ctx_factory):
    from icp_amd import binding, synth
    W, H = 160, 120
    K = np.array([[131.25, 0, 79.5], [0, 131.25, 59.5], [0, 0, 1]], f32)
    a, b2 = synth.rgbd_pair(0, width=W, height=H, K=K), synth.rgbd_pair(1, width=W, height=H, K=K)
    depth = np.stack([p[:, 2].reshape(H, W).copy() for p in (a["tgt_pts"], a["src_pts"], b2["src_pts"])])        # three frames of the trajectory
    cam = binding.depth_camera(K, W, H)
    to, so = binding.depth_options(False, 1), binding.depth_options(False, 2)
    kw = dict(n_iterations=15, max_distance=0.01)
    # the reference: frame by frame with the option off, for the bounds
    r = make_ctx(gpu_ctx_factory, **kw)
    r.set_target_depth(depth[0], None, cam, to)
    pose, fulls = EYE, []
    for k in (1, 2):
        r.set_source_depth(depth[k], None, cam, so)
        ref = reference_run(r, pose)
        fulls.append(ref["full"]); pose = ref["pose"]
    er, et, margin = pick_eps(fulls)
    assert margin > 1.25
    opts = dict(rotation=er, translation=et)
    # frame by frame with the option on
    r.set_convergence_options(**opts)
    pose, per_frame = EYE, []
    for k in (1, 2):
        r.set_source_depth(depth[k], None, cam, so)
        pose, recs, st = r.run(pose, check=False)
        per_frame.append((pose, len(recs), st, r.convergence()))
    assert any(f[3]["converged"] and f[1] < 15 for f in per_frame)
    t = make_ctx(gpu_ctx_factory, **kw)
    t.set_convergence_options(**opts)
    final, trecs, _ = t.track_depth_frames(depth, None, cam, to, so)
    for k in range(2):
        assert trecs[k]["iterations"] == per_frame[k][1] and trecs[k]["status"] == per_frame[k][2], k
        assert np.array_equal(u32(trecs[k]["pose"]), u32(per_frame[k][0])), k
    assert np.array_equal(u32(final), u32(per_frame[1][0])) and t.convergence() == per_frame[1][3]
    r.close(); t.close()


def test_cxx_adaptor_sets_and_clears_the_criteria(gpu_ctx_factory, bunny, tmp_path):
    """setConvergenceCriteria / clearConvergenceCriteria on HipLinearICPOptimizer from a C++14 host (tests/cpp/converge_adaptor.cpp)."""
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libdir = os.path.join(root, "icp-variants_amd", "lib")
    exe = os.path.join(str(tmp_path), "converge_adaptor")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "converge_adaptor.cpp"),
                           "-o", exe, "-L", libdir, "-licp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    c = make_ctx(gpu_ctx_factory)
    load(c, bunny)
    ref = reference_run(c)
    opts = eps_of(ref)
    want_n = R.stop_index([r["pose"] for r in ref["recs"]], EYE, ref["factors"], [r["status"] for r in ref["recs"]], opts)[0]
    c.close()
    dump = os.path.join(str(tmp_path), "bunny.bin")
    with open(dump, "wb") as f:
        for k in ("src", "tgt"):
            f.write(np.int32(len(bunny[k + "_pts"])).tobytes()); f.write(bunny[k + "_pts"].astype(f32).tobytes())
            f.write(bunny[k + "_nrm"].astype(f32).tobytes()); f.write(bunny[k + "_rgba"].astype(np.uint8).tobytes())
    out = subprocess.check_output([exe, dump, repr(float(f32(opts["rotation"]))), repr(float(f32(opts["translation"])))], timeout=120).decode().split()
    assert out == ["off", "20", "on", str(want_n), "cleared", "20", "same_prefix", "1", "ends_on_last_record", "1", "refused", "1", "1", "ceres", "0"] and want_n < 20
