"""The 34 reduced sums of every accumulation route against ONE fp64 reference, at source sizes on the edges of the folds.

Routes ("the accumulation routes"): (1) k_post (+ k_sym_accumulate) and k_reduce_solve, reached through icp_correspond whatever
the matcher; (2) the epilogue of k_knn_bvh_post<DIM, WIDE> and k_reduce_solve, the separate form of the loop; (3) the epilogue of
k_knn_bvh_post_ring<DIM, WIDE> with the reducer riding in front of the next launch, the merged form, the default.  (2) and (3) are reached
through the test hook icp_debug_loop_sums (Context.loop_sums), which reports the kernel family and instantiation that ran: every case
asserts it, and that the pose the hook composed is the pose of the same iteration of icp_run in that form, bit for bit.

The reference (tests/sums_cases.py): the oracle's matcher, weights and rejection, then tests/robust_restatement.py's fp32 rows with fp64
products and sums.  Every comparison: count and n_valid exact, sums[1:34] within 1e-9 of the reference relative to its sums of absolute
terms, records (where the route keeps them: icp_correspond; the fused matcher through icp_match_seeded) bit-equal to the oracle's.
One exception, by design of the kernel and found by these tests: the fused point-to-plane epilogue of routes (2) and (3) does not fold
sum s and sum d (slots 1..6; only the means need them, and point-to-plane has no use for means) and stores +0 there; the tests assert
exactly that and compare the other 27 sums.  icp_correspond's point-to-plane sums (route 1) carry all 33.
tests/test_sums_host.py shows that one pair dropped or doubled moves a sum by >= 1.06e-5 at every size."""
import ctypes as C
import functools

import numpy as np
import pytest

import sums_cases as S
import support as M
from support import u32

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 7
ERR_INVALID_ARG = 1


# this file's defaults: 2 iterations, S.MAX_DIST, half the points under a selection, the 80 x 60 camera under projective matching
configure = functools.partial(M.configure, n_iterations=2, proba=0.5, seed=SEED, max_distance=S.MAX_DIST, K=S.K8, width=80, height=60)


class Case:
    """One source against one target at S.pose(): the moved points, the oracle's raw matches (made once), the records per (weighting,
    rejection)."""

    def __init__(self, orc, n, hostile, edges=True, kind="knn3", tgt=None, match=None, subset=None):
        self.orc, self.n, self.kind = orc, n, kind
        self.tgt = tgt if tgt is not None else (S.organised_target(hostile) if kind == "projective" else S.target(hostile))
        self.pts, self.nrm, self.rgba, self.cluster, self.nan_pt = S.source(n, hostile, edges)
        self.label = "n %d %s%s%s" % (n, kind, " hostile" if hostile else "", "" if edges else " no NaN points")
        self.T = S.pose()
        self.match = match if match is not None else S.matcher(orc, kind, self.tgt, self.rgba)
        self.at(self.T, subset)
        self._recs = {}

    def at(self, T, subset=None):
        """(Re)match at pose T, over the source points `subset` (positions; None: all)."""
        self.sub = np.arange(self.n) if subset is None else np.asarray(subset)
        sel = (self.pts[self.sub], self.nrm[self.sub])
        self.q, self.qn = S.moved(self.orc, sel, T)
        self.srgba = self.rgba[self.sub]
        m = S.matcher(self.orc, self.kind, self.tgt, self.srgba) if self.kind == "knn6" else self.match
        self.raw = m(self.q)
        self._recs = {}

    def recs(self, weighting, rejection):
        k = (weighting, rejection)
        if k not in self._recs:
            r = S.records(self.orc, weighting, rejection, self.q, self.qn, self.srgba, self.tgt, self.raw)
            valid = S.valid_mask(self.q, self.tgt, r)
            if len(self.sub) == self.n:
                S.check_inputs(self.pts, self.cluster, self.nan_pt, valid, self.label)
            self._recs[k] = r
        return self._recs[k]

    def check(self, metric, weighting, rejection, dev_sums, dev_nv, tag, nonfinite=False, means_unused=False):
        """The sums of one device call against the reference.  Symmetric: the means as the device has them (sum s / n, sum d / n rounded
        to fp32, as teacher_forced of tests/test_gpu_robust.py takes them); sum s and sum d themselves are among the sums compared."""
        r = self.recs(weighting, rejection)
        means = (f32(dev_sums[1:4] / dev_sums[0]), f32(dev_sums[4:7] / dev_sums[0])) if metric == 2 and dev_sums[0] > 0 else None
        ref, ab = S.sums(metric, self.q, self.qn, self.tgt, r, means)
        label = "%s metric %d weighting %d rejection %d %s" % (self.label, metric, weighting, rejection, tag)
        err = S.compare(dev_sums, dev_nv, ref, ab, label, allow_nonfinite=nonfinite, means_unused=means_unused)
        print("%s: %d valid, largest error %.3g of an absolute sum" % (label, dev_nv, err))
        return ref


def empty_blocks(lib, case):
    """Blocks of the fused routes whose 256 queries all belong to the cluster, by the library's own block -> wave mapping: the cluster
    is the run of Morton positions behind the other finite points (S.check_inputs asserts why)."""
    n = case.n
    start = int((~case.cluster & ~case.nan_pt).sum()); stop = start + int(case.cluster.sum())
    mgrid = (n + S.BLOCK - 1) // S.BLOCK
    nw = C.c_int32(0)
    lib.icp_debug_wave_slot(0, 0, mgrid, C.byref(nw))
    assert nw.value * 64 == S.BLOCK
    out = 0
    for lb in range(mgrid):
        slots = [lib.icp_debug_wave_slot(lb, w, mgrid, None) for w in range(nw.value)]
        out += all(start <= 64 * s_ and 64 * s_ + 64 <= stop for s_ in slots)
    return out


def load(ctx, case, colors=True):                           # not support.load: a Case, not a dict of clouds
    ctx.set_target(case.tgt[0], case.tgt[1], case.tgt[2] if colors else None)
    ctx.set_source(case.pts, case.nrm, case.rgba if colors else None)


def variants(n):
    """(hostile, edges): finite normals and the hostile ones; the two smallest sizes also without their NaN points (with them no pair is left)."""
    out = [(False, True), (True, True)]
    return out + [(False, False)] if n <= 2 else out


def hits_inf(case, recs):
    i = S.pair()["organised_of"][S.INF_TARGET] if case.kind == "projective" else S.INF_TARGET
    return bool((S.valid_mask(case.q, case.tgt, recs) & (recs["idx"] == i)).any())


# --------------------------------------------------------------------------------------------------------- route (1): icp_correspond
def correspond_case(ctx, case, metric, combos, hostile, **cfg):
    for weighting, rejection in combos:
        configure(ctx, metric, weighting, rejection, **cfg)
        m, sums, nv = ctx.correspond(case.T)
        r = case.recs(weighting, rejection)
        assert np.array_equal(m["idx"], r["idx"]) and np.array_equal(u32(m["weight"]), u32(r["weight"])), (case.label, metric, weighting, rejection)
        poisoned = hostile and metric != 0
        ref = case.check(metric, weighting, rejection, sums, nv, "k_post", nonfinite=poisoned)
        if poisoned and hits_inf(case, r):
            assert not np.isfinite(ref[7:34]).all(), case.label      # the infinite normal really reached the rows
        if rejection == 1 and case.n >= 63:
            assert (r["idx"] < 0).sum() > (case.raw["idx"] < 0).sum(), case.label      # the rejection really removed something


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("n", S.SIZES)
def test_correspond_sums_brute(gpu_ctx_factory, orc, n, metric):
    """k_post (+ k_sym_accumulate) + k_reduce_solve behind the 3-D brute-force matcher: 256 threads per block, at most 512 blocks, a
    grid-stride loop from 131 073 records on; k_reduce_solve folds 1 .. 512 partials.  Every weighting and rejection with finite normals;
    the hostile normals with every weighting and rejection for point-to-point, and in kind for the other two (tests/sums_cases.py)."""
    ctx = M.make_ctx(gpu_ctx_factory, "merged")
    full = [(w, r) for w in (0, 1, 2, 3) for r in (0, 1)]
    for hostile, edges in variants(n):
        case = Case(orc, n, hostile, edges)
        load(ctx, case)
        correspond_case(ctx, case, metric, full if (not hostile or metric == 0) else [(0, 1), (1, 0)], hostile, knn_backend=0)
    ctx.close()


@pytest.mark.parametrize("kind", ["knn6", "projective"])
@pytest.mark.parametrize("n", S.SMALL)
def test_correspond_sums_other_matchers(gpu_ctx_factory, orc, n, kind):
    """The same route behind the 6-D brute-force matcher (colour features, colour weighting) and the projective matcher (organised
    80 x 60 target)."""
    ctx = M.make_ctx(gpu_ctx_factory, "merged")
    cfg = dict(knn_backend=0, color_icp=1) if kind == "knn6" else dict(matching=1)
    for hostile in (False, True):
        case = Case(orc, n, hostile, kind=kind)
        load(ctx, case)
        for metric in (0, 1, 2):
            correspond_case(ctx, case, metric, [(3, 1), (0, 0)] if kind == "knn6" else [(0, 1), (1, 0), (2, 1)], hostile, **cfg)
    ctx.close()


# ------------------------------------------------------------------------------- routes (2) and (3): the loop's own sums, through the hook
FAMILY = {"k_post": 0, "k_knn_bvh_post": 1, "k_knn_bvh_post_ring": 2}


def loop_case(ctx, form, case, metric, weighting, rejection, dim=3, wide=0, iteration=0, pose=None, records=True, nonfinite=False, compare_pose=True, **cfg):
    """One iteration through the hook in `form`: route code, sums, the fused matcher's records, and the composed pose against icp_run's
    record of that iteration (and icp_iterate's for the full cloud in the separate form)."""
    configure(ctx, metric, weighting, rejection, **cfg)
    T = case.T if pose is None else pose
    sums, nv, composed, route = ctx.loop_sums(T, form, iteration)
    family = "k_knn_bvh_post_ring" if form == "merged" else ("k_knn_bvh_post" if metric in (0, 1) else "k_post")
    assert (route["family"], route["dim"], route["wide"]) == (FAMILY[family], dim, wide), (case.label, form, metric, route)
    tag = "%s<%d, %s> iteration %d" % (family, dim, "true" if wide else "false", iteration)
    case.check(metric, weighting, rejection, sums, nv, tag, nonfinite=nonfinite, means_unused=metric == 1)      # (metric 1 here: always a fused route)
    r = case.recs(weighting, rejection)
    if records and metric != 2:                                # (icp_match_seeded: the fused kernel of this form with its records kept)
        m, _ = ctx.match_seeded([T])
        assert np.array_equal(m["idx"], r["idx"]) and np.array_equal(u32(m["weight"]), u32(r["weight"])), (case.label, tag)
    if not compare_pose:
        return route
    runs0, falls0 = M.counters(ctx)
    _, recs, rc = ctx.run(case.T, check=False)
    runs1, falls1 = M.counters(ctx)
    assert runs1 - runs0 == (1 if form == "merged" and metric == 1 else 0)
    if form == "merged" and route["fault"]:                    # the rank guard failed in the ring: run_loop repeats the run in the separate form
        assert route["fault"] == 2 and falls1 - falls0 == 1 and np.array_equal(u32(composed), u32(T)), (case.label, tag, route)
        return route
    assert route["fault"] == 0
    if iteration > 0:
        assert np.array_equal(u32(recs[iteration - 1]["pose"]), u32(T))
    assert recs[iteration]["n_valid"] == nv and np.array_equal(u32(recs[iteration]["pose"]), u32(composed)), (case.label, tag)
    if form == "separate" and not cfg.get("multires") and not cfg.get("selection"):
        if nv == 0:                                            # (icp_iterate reports the empty iteration as an error)
            with pytest.raises(Exception) as ei:
                ctx.iterate(T)
            assert ei.value.code == 8
        else:
            p1, st = ctx.iterate(T)
            assert st["n_valid"] == nv and np.array_equal(u32(p1), u32(composed)), (case.label, tag)
    return route


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("n", S.SIZES)
def test_loop_sums(gpu_ctx_factory, orc, n, form):
    """DIM = 3, the full cloud: 256 queries per block in Morton order, ceil(n / 256) partials (256 and 257 of them at n = 65 281 and
    65 537: the reducer's 256-thread fold), whole blocks without a valid pair (the cluster).  Separate: metrics 0, 1 fused, 2 through
    k_post; merged: point-to-plane only (run_loop merges nothing else)."""
    ctx = M.make_ctx(gpu_ctx_factory, form)
    for hostile, edges in variants(n):
        case = Case(orc, n, hostile, edges)
        load(ctx, case, colors=False)
        if n >= 1054:
            assert empty_blocks(ctx.lib, case) >= 1, n
        for metric in (0, 1, 2):
            if form == "merged" and metric != 1:
                if not hostile and edges:
                    configure(ctx, metric)
                    with pytest.raises(Exception) as ei:
                        ctx.loop_sums(case.T, form)
                    assert ei.value.code == ERR_INVALID_ARG and "merged form" in str(ei.value)
                continue
            poisoned = hostile and metric != 0
            for weighting, rejection in ([(0, 1)] if poisoned else [(0, 1), (1, 1), (0, 0)]):
                loop_case(ctx, form, case, metric, weighting, rejection, nonfinite=poisoned, compare_pose=not poisoned)
    ctx.close()


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("n", S.SMALL)
def test_loop_sums_colour6d(gpu_ctx_factory, orc, n, form):
    """DIM = 6: colour features in the search, colour weighting."""
    ctx = M.make_ctx(gpu_ctx_factory, form)
    case = Case(orc, n, False, kind="knn6")
    load(ctx, case)
    for metric in ((1,) if form == "merged" else (0, 1)):
        for rejection in (1, 0):
            loop_case(ctx, form, case, metric, 3, rejection, dim=6, color_icp=1)
    ctx.close()


def level_positions(orc, case, factor):
    """The source positions of a multires level (PointCloud::getCoarseResolution, the oracle's restatement); factor 0: the full cloud."""
    if factor == 0:
        return np.arange(case.n)
    return orc.coarse(case.pts, case.nrm, None, factor)[3]


@pytest.mark.parametrize("mode", ["multires", "selection", "multires_selection"])
@pytest.mark.parametrize("n", S.SEL)
def test_loop_sums_selected_queries(gpu_ctx_factory, orc, n, mode):
    """Query sets that are not the resident cloud: a multires level (a Morton-sorted copy of its own: both forms) and random
    re-sampling with proba 0.5 (the `sel`-indexed path: index lists drawn per iteration; the loop does not merge it, and the hook
    refuses).  Iterations 0 and 1 of the plan, each at the pose icp_run had there."""
    from icp_amd import binding
    multires, selection = int("multires" in mode), int("selection" in mode)
    case = Case(orc, n, False)
    for form in M.FORMS:
        ctx = M.make_ctx(gpu_ctx_factory, form)
        load(ctx, case, colors=False)
        configure(ctx, 1, multires=multires, selection=selection)
        if form == "merged" and selection:
            with pytest.raises(Exception) as ei:
                ctx.loop_sums(case.T, form)
            assert ei.value.code == ERR_INVALID_ARG and "merged form" in str(ei.value)
            ctx.close()
            continue
        factors = binding.schedule(ctx.params, n)
        assert len(factors) >= 2 and (not multires or factors[0] > 1)
        for metric in ((1,) if form == "merged" else (0, 1)):
            configure(ctx, metric, multires=multires, selection=selection)
            _, recs, _ = ctx.run(case.T, check=False)
            for it in (0, 1):
                pos = level_positions(orc, case, factors[it])
                if selection:
                    th = int(float(f32(0.5)) * 4294967296.0)
                    pos = pos[np.array([binding.select_hash(SEED, it, int(k)) < th for k in pos], bool)]
                T = case.T if it == 0 else recs[0]["pose"]
                case.at(T, pos)
                assert 0 < len(pos) < n and S.valid_mask(case.q, case.tgt, case.recs(0, 1)).sum() * 4 >= len(pos), (mode, it, len(pos))
                loop_case(ctx, form, case, metric, 0, 1, iteration=it, pose=T, records=False, multires=multires, selection=selection)
        ctx.close()
    case.at(case.T)


@pytest.fixture(scope="module")
def deep_target(orc):
    """524 289 + 4 096 target points (more than 8 four-wide levels: the <DIM, true> instantiations): the frame tiled with jitter, and the
    oracle's exact kd-tree over it."""
    tp, tn, tc = S.target(False)
    m = 524289 + 4096
    rng = np.random.default_rng(99)
    pick = np.arange(m) % len(tp)
    pts = (tp[pick] + rng.normal(0, 4e-3, (m, 3))).astype(f32)
    kd = orc.KdTree(pts)
    return (pts, tn[pick].copy(), tc[pick].copy()), kd


@pytest.mark.parametrize("form", M.FORMS)
def test_loop_sums_deep_tree(gpu_ctx_factory, orc, deep_target, form):
    """<3, true>: the tree of a target of more than 524 288 points, 1 054 queries.  (<6, true> needs a coloured target of that size and a
    6-D scan of it in the oracle, which has no 6-D tree: left out.)"""
    tgt, kd = deep_target
    case = Case(orc, 1054, False, tgt=tgt, match=lambda q: kd.query(q, S.MAX_DIST)[0])
    ctx = M.make_ctx(gpu_ctx_factory, form)
    load(ctx, case, colors=False)
    for weighting in (0, 1):
        loop_case(ctx, form, case, 1, weighting, 1, wide=1)
    ctx.close()


def test_hook_refusals(gpu_ctx_factory, orc):
    ctx = M.make_ctx(gpu_ctx_factory, "merged")
    case = Case(orc, 257, False)
    load(ctx, case, colors=False)
    configure(ctx, 1)
    for setup, undo in ((lambda: ctx.set_robust_options("huber", overlap=0.7), lambda: ctx.set_robust_options()),
                        (lambda: ctx.set_optimizer(True), lambda: ctx.set_optimizer(None))):
        setup()
        for form in M.FORMS:
            with pytest.raises(Exception) as ei:
                ctx.loop_sums(case.T, form)
            assert ei.value.code == ERR_INVALID_ARG
        undo()
    for form in M.FORMS:
        with pytest.raises(Exception) as ei:
            ctx.loop_sums(case.T, form, 2)                     # the plan has two iterations
        assert ei.value.code == ERR_INVALID_ARG
    configure(ctx, 1, n_iterations=1)                          # run_loop merges from two iterations on
    with pytest.raises(Exception) as ei:
        ctx.loop_sums(case.T, "merged")
    assert ei.value.code == ERR_INVALID_ARG
    ctx.loop_sums(case.T, "separate")
    ctx.close()
