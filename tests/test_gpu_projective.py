"""k_projective (csrc/dev_projective.hpp) on frames built to break it: the crafted plane of tests/projective_restatement.py, where every
distance is exact and a query between two or four pixels ties exactly, where the clipped window takes every width from 1 to 25 columns at
every alignment of its first column (the 16-byte, 8-byte and scalar stages of a window row), where queries lie exactly on the threshold,
and where the target has holes by x alone.  The records are the oracle's, which tests/test_projective_host.py pins to the numpy
restatement on the same cases; every comparison is bit for bit but the pose of the one-iteration test.

Entry points: icp_query_matches (pretransformed queries), icp_match (the transform in the kernel; the only one that returns d2),
icp_correspond (the full query set behind weighting and rejection), the loop's `sel`-indexed launch under RANDOM_SAMPLING, and icp_run.
No entry point returns the records of a `sel`-indexed launch (icp_correspond ignores `selection`, include/icp_hip.h), so that launch is
held to the oracle's records of the selected queries through the sums the loop reduced from them (Context.loop_sums): on the exact
lattice a sum of source points, target points and their products is exact in fp64 in any order, so one record resolved to the
neighbouring pixel, or read at the slot instead of at sel[slot], changes a sum that must be EQUAL."""
import numpy as np
import pytest

import projective_restatement as P
import support as M
from support import POSE_TOL, bits, u32

pytestmark = pytest.mark.gpu
f32 = np.float32
EYE = np.eye(4, dtype=f32)
SIZE_IDS = ["%dx%d" % s for s in P.SIZES]
PROBA, SEED = 0.5, 7


def projective_ctx(factory, c, max_distance, **kw):
    ctx = factory()
    M.configure(ctx, matching=1, knn_backend=0, max_distance=max_distance, K=c["K"], width=c["W"], height=c["H"], **kw)
    return ctx


def plane_normals(n):
    return np.tile(np.array([[0, 0, -1]], f32), (n, 1))


def same_records(m, d2, mo, do, label):
    bad = np.flatnonzero((m["idx"] != mo["idx"]) | (u32(m["weight"]) != u32(mo["weight"])) | (False if d2 is None else bits(d2) != bits(do)))
    assert len(bad) == 0, "%s: %d records differ, the first at query %d: device (%d, %r, d2 %r), oracle (%d, %r, d2 %r)" % (
        label, len(bad), bad[0], m["idx"][bad[0]], m["weight"][bad[0]], None if d2 is None else d2[bad[0]], mo["idx"][bad[0]], mo["weight"][bad[0]], do[bad[0]])


@pytest.fixture(scope="module")
def oracle_at_identity(orc):
    """(W, H, threshold) -> the oracle's (records, d2) of the case's own queries, made once."""
    memo = {}

    def get(W, H, thr):
        if (W, H, thr) not in memo:
            c = P.case(W, H)
            memo[W, H, thr] = orc.projective(c["queries"], c["tgt"], W, H, c["K"], thr)
        return memo[W, H, thr]
    return get


# ------------------------------------------------------------------------------------------------------------ 1. every crafted size
@pytest.mark.parametrize("size", P.SIZES, ids=SIZE_IDS)
def test_crafted_queries_every_size_and_threshold(gpu_ctx_factory, orc, oracle_at_identity, size):
    """icp_query_matches on the lattice and the odd queries: idx and weight.  icp_query_matches returns no distances, so d2 comes from
    icp_match at the identity on the same points as the resident source (the oracle's own transform in front of its matcher, as everywhere)."""
    W, H = size
    c = P.case(W, H)
    q = c["queries"]
    assert len(q) % 256 != 0
    ctx = projective_ctx(gpu_ctx_factory, c, 0.0)
    ctx.set_target(c["tgt"]); ctx.set_source(q)
    qi = orc.transform_points(q, EYE)
    for thr in P.THRESHOLDS:
        M.configure(ctx, matching=1, knn_backend=0, max_distance=thr, K=c["K"], width=W, height=H)
        mo, do = oracle_at_identity(W, H, thr)
        same_records(ctx.query_matches(q), None, mo, do, "%d x %d threshold %g icp_query_matches" % (W, H, thr))
        m, d2 = ctx.match(EYE)
        mi, di = orc.projective(qi, c["tgt"], W, H, c["K"], thr)
        same_records(m, d2, mi, di, "%d x %d threshold %g icp_match" % (W, H, thr))
        lat = slice(0, len(q) - P.N_ODD)                      # the lattice passes the identity unchanged: the same records
        assert np.array_equal(mi["idx"][lat], mo["idx"][lat]) and np.array_equal(bits(di[lat]), bits(do[lat]))
        print("%d x %d threshold %g: %d of %d queries matched, %d with d2 == 2^-14" % (W, H, thr, (m["weight"] > 0).sum(), len(q), (d2 == f32(P.HALF_PIXEL_D2)).sum()))
    ctx.close()


# ------------------------------------------------------------------------------------------------------ 2. the transform in the kernel
@pytest.mark.parametrize("size", [(37, 29), (40, 30)], ids=["37x29", "40x30"])
def test_crafted_source_under_poses(gpu_ctx_factory, orc, size):
    """icp_match at the identity and two small poses.  Moved, the lattice is no longer exact: real-valued distances through the same
    clipped windows and the same holes."""
    W, H = size
    c = P.case(W, H)
    ctx = projective_ctx(gpu_ctx_factory, c, 0.0)
    ctx.set_target(c["tgt"]); ctx.set_source(c["queries"])
    for k, T in enumerate((EYE, M.rand_pose(1, 0.01, 0.01), M.rand_pose(2, 0.04, 0.04))):
        q = orc.transform_points(c["queries"], T)
        assert np.array_equal(bits(ctx.transform_points(c["queries"], T)), bits(q))
        for thr in P.THRESHOLDS:
            M.configure(ctx, matching=1, knn_backend=0, max_distance=thr, K=c["K"], width=W, height=H)
            m, d2 = ctx.match(T)
            mo, do = orc.projective(q, c["tgt"], W, H, c["K"], thr)
            same_records(m, d2, mo, do, "%d x %d pose %d threshold %g" % (W, H, k, thr))
        assert (mo["weight"] > 0).sum() > 2000, (size, k)       # (threshold 10: the moved lattice still fills the image's windows)
    ctx.close()


# ------------------------------------------------------------------------------------------------------ 3. a sub-sampled query set
def exact_sums(q, tgt, recs):
    """[n, sum s, sum d, sum w, sum w s, sum w d, sum d (w s)^T] of the valid pairs, fp64: the point-to-point sums of icp_correspond."""
    import robust_restatement as R
    return R.sums(0, q, tgt, recs)[0]


def test_selected_queries_through_the_loop(gpu_ctx_factory, orc, oracle_at_identity):
    """The 37 x 29 case as resident source.  icp_correspond: the records of the full query set (weighting and rejection off: the
    matcher's own).  RANDOM_SAMPLING at 0.5: the loop's first iteration launches k_projective with an index list; the sums it reduced
    equal, exactly, the fp64 sums of the oracle's records of the queries sel[k] -- and differ from those of queries 0 .. len(sel) - 1."""
    from icp_amd import binding
    W, H = 37, 29
    c = P.case(W, H)
    q, tgt = c["queries"], c["tgt"]
    thr = P.HALF_PIXEL_D2
    ctx = projective_ctx(gpu_ctx_factory, c, thr, metric=0, rejection=0, n_iterations=1)
    ctx.set_target(tgt, plane_normals(len(tgt))); ctx.set_source(q, plane_normals(len(q)))
    mo, do = oracle_at_identity(W, H, thr)
    qi = orc.transform_points(q, EYE)
    mi, _ = orc.projective(qi, tgt, W, H, c["K"], thr)
    m, sums, nv = ctx.correspond(EYE)
    same_records(m, None, mi, do, "icp_correspond")
    ref = exact_sums(qi, tgt, mi)
    assert nv == ref[0] > 1000 and np.array_equal(sums[:34], ref), (nv, ref[0])

    M.configure(ctx, metric=0, rejection=0, n_iterations=1, matching=1, knn_backend=0, max_distance=thr, K=c["K"], width=W, height=H, selection=1, proba=PROBA, seed=SEED)
    sums, nv, _, route = ctx.loop_sums(EYE, "separate", 0)
    sel = np.asarray(ctx.selection(0), np.int64)
    th = int(float(f32(PROBA)) * 4294967296.0)
    assert np.array_equal(sel, np.flatnonzero(np.array([binding.select_hash(SEED, 0, k) < th for k in range(len(q))])))
    assert 0.4 * len(q) < len(sel) < 0.6 * len(q) and (route["family"], route["wide"], route["fault"]) == (0, -1, 0)
    ref = exact_sums(qi[sel], tgt, mi[sel])                   # the record at selected position k is the oracle's record of query sel[k]
    slot = exact_sums(qi[:len(sel)], tgt, mi[:len(sel)])      # what a launch that ignored the list would have matched
    print("selection: %d of %d queries, %d valid pairs (%d in the first %d queries)" % (len(sel), len(q), ref[0], slot[0], len(sel)))
    assert ref[0] > 300 and ref[0] != slot[0] and not np.array_equal(ref[4:7], slot[4:7])
    assert nv == ref[0] and np.array_equal(sums[:34], ref), (nv, ref[0], sums[:7], ref[:7])
    _, recs, rc = ctx.run(EYE, check=False)                   # and the run itself counts the same pairs
    assert recs[0]["n_src"] == len(sel) and recs[0]["n_valid"] == ref[0]
    ctx.close()


# ------------------------------------------------------------------------------------------------- 4. one iteration as the loop runs it
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_one_iteration_on_a_depth_pair(gpu_ctx_factory, orc, metric):
    """A 37 x 29 pair of wavy depth frames through the crafted camera (the plane is rank-deficient for a solve), the source with holes,
    holes by x alone and the nine odd queries: projective matching, rejection on, one iteration of icp_run against the oracle's."""
    from conftest import pose_error
    d = P.wavy_pair()
    W, H, K = d["W"], d["H"], d["K"]
    ctx = projective_ctx(gpu_ctx_factory, d, 0.01, metric=metric, rejection=1, n_iterations=1)
    ctx.set_target(d["tgt_pts"], d["tgt_nrm"]); ctx.set_source(d["src_pts"], d["src_nrm"])
    T0 = M.rand_pose(4, 0.01, 0.01)
    pose, recs, rc = ctx.run(T0)
    prm = orc.make_params(metric=metric, matching=1, rejection=1, n_iterations=1, max_distance=0.01, K=K, width=W, height=H, solver_mode=1)
    po, ro = orc.estimate_pose(prm, d["src_pts"], d["src_nrm"], None, d["tgt_pts"], d["tgt_nrm"], None, T0)
    ang, tr = pose_error(pose, po)
    print("metric %d: n_valid %d (oracle %d), pose error %.3g rad %.3g m" % (metric, recs[0]["n_valid"], ro[0]["n_valid"], ang, tr))
    assert rc == 0 and len(recs) == len(ro) == 1
    assert recs[0]["n_valid"] == ro[0]["n_valid"] > 100
    assert ang < POSE_TOL and tr < POSE_TOL
    assert pose_error(po, T0)[1] > 1e-3                       # (the iteration moved the pose: the comparison is of a solve, not of T0)
    ctx.close()


# ----------------------------------------------------------------------------------------------------------------------- 5. repeats
def test_repeats_are_identical(gpu_ctx_factory):
    W, H = 37, 29
    c = P.case(W, H)
    ctx = projective_ctx(gpu_ctx_factory, c, P.HALF_PIXEL_D2)
    ctx.set_target(c["tgt"]); ctx.set_source(c["queries"])
    T = M.rand_pose(2, 0.04, 0.04)
    a, b = ctx.query_matches(c["queries"]), ctx.query_matches(c["queries"])
    assert a.tobytes() == b.tobytes()
    (ma, da), (mb, db) = ctx.match(T), ctx.match(T)
    assert ma.tobytes() == mb.tobytes() and da.tobytes() == db.tobytes()
    ctx.close()
