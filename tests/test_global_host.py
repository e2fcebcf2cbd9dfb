"""Global registration without a GPU: the structs and defaults of the C ABI, the invariants of the numpy restatement
(tests/global_restatement.py) that the GPU tests compare the device with, the properties of the input clouds of tests/global_cases.py that
those tests rely on (ties in every list, collinear and nearly collinear triples, M = n), and the resource report of the new kernels."""
import ctypes as C
import numpy as np
import pytest

import global_cases as gc
import global_restatement as gr
from device_asm import device_asm, kernel_resources


def test_struct_layouts_and_defaults():
    from icp_amd import binding
    lib = binding.load_library()
    assert C.sizeof(binding.IcpGlobalOptions) == 8 * 4
    # pose 64 | n_inliers 4 | reserved 4 | sum_d2 8 | status 4 | draw 12 = 96, the double on an 8-byte boundary, no hidden padding
    assert C.sizeof(binding.IcpGlobalHypothesis) == 96 and binding.IcpGlobalHypothesis.sum_d2.offset == 72
    assert binding.GLOBAL_HYPOTHESIS_DTYPE.itemsize == 96
    assert sum(C.sizeof(t) for _, t in binding.IcpGlobalHypothesis._fields_) == 96
    for name in ("pose", "n_inliers", "reserved", "sum_d2", "status", "draw"):
        assert binding.GLOBAL_HYPOTHESIS_DTYPE.fields[name][1] == getattr(binding.IcpGlobalHypothesis, name).offset, name
    o = binding.IcpGlobalOptions()
    assert lib.icp_global_options_default(C.byref(o)) == 0
    assert (o.k, o.feature_stride, o.mutual, o.n_hypotheses, o.seed, o.n_best) == (20, 1, 1, 4096, 0, 16)
    assert np.float32(o.edge_similarity) == np.float32(0.9) and np.float32(o.inlier_distance) == np.float32(0.005)
    assert lib.icp_global_options_default(None) == 1
    assert lib.icp_set_global_options(None, C.byref(o)) == 1 and lib.icp_compute_features(None, 0) == 1
    n = C.c_int32(0)
    assert lib.icp_register_global(None, None, None, C.byref(n)) == 1 and lib.icp_get_global_hypotheses(None, None, 0, C.byref(n)) == 1


@pytest.fixture(scope="module")
def source_features(bunny):
    return gr.features(bunny["src_pts"], bunny["src_nrm"], 10)


def test_quarter_turn_leaves_the_histograms_unchanged(bunny, source_features):
    """(x, y, z) -> (-y, x, z) of points and normals is exact in every operation of the contract: x^2 + y^2 and a_x b_x + a_y b_y commute,
    the cross product's components move and change sign with it.  So the neighbour lists, the integer SPFH and the FPFH bits are equal."""
    def turn(a):
        return np.stack([-a[:, 1], a[:, 0], a[:, 2]], axis=1).astype(np.float32)
    f = source_features
    g = gr.features(turn(bunny["src_pts"]), turn(bunny["src_nrm"]), 10)
    assert np.array_equal(f["idx"], g["idx"]) and np.array_equal(f["d2"], g["d2"])
    assert np.array_equal(f["counts"], g["counts"]) and np.array_equal(f["pairs"], g["pairs"])
    assert np.array_equal(f["F"].view(np.uint32), g["F"].view(np.uint32))


def test_general_rigid_motion_leaves_fpfh_nearly_unchanged(bunny, source_features):
    """A general rotation rounds the moved fp32 coordinates, so a pair feature within ~1e-5 bin units of a boundary may change bins and a
    near-tie at the k-th neighbour may swap: a handful of rows at most.  Every other row moves by fp64 rounding alone."""
    rng = np.random.default_rng(5)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(2.0) * K + (1 - np.cos(2.0)) * (K @ K)
    p = (bunny["src_pts"].astype(np.float64) @ R.T + np.array([0.05, -0.02, 0.1])).astype(np.float32)
    nr = (bunny["src_nrm"].astype(np.float64) @ R.T).astype(np.float32)
    g = gr.features(p, nr, 10)
    diff = np.abs(g["F"] - source_features["F"]).max(axis=1)
    assert np.isfinite(diff).all()
    assert (diff > 1e-4).sum() <= len(diff) // 100, (diff > 1e-4).sum()


def test_sub_histograms_sum_to_one(source_features):
    f = source_features
    c = f["counts"].astype(np.int64).reshape(-1, 3, gr.BINS).sum(axis=2)
    assert np.array_equal(c, np.repeat(f["pairs"][:, None], 3, axis=1))          # h = counts / pairs: each third sums to exactly 1
    assert (f["pairs"] > 0).all() and (f["pairs"] <= 9).all()
    s = f["F"].astype(np.float64).reshape(-1, 3, gr.BINS).sum(axis=2)              # F = h + sum w h(q), sum w = 1: each third sums to 2
    assert np.abs(s - 2.0).max() < 1e-5


def test_matcher_equals_a_kd_tree(bunny, source_features):
    """Against scipy's cKDTree in 33-D (fp64 distances of the same fp32 rows), wherever the two nearest distances differ by more than the
    fp32 sum can err: 35 roundings of 2^-24 relative each on either distance, 4.2e-6 together -- 1e-5 asked for."""
    from scipy.spatial import cKDTree
    Fs = source_features["F"]
    Ft = gr.features(bunny["tgt_pts"], bunny["tgt_nrm"], 10)["F"]
    idx, best, second = gr.match_rows(Fs, Ft, with_second=True)
    _, j = cKDTree(Ft.astype(np.float64)).query(Fs.astype(np.float64), k=1)
    clear = second > best * np.float32(1 + 1e-5)
    assert clear.sum() > 0.95 * len(Fs)
    assert np.array_equal(idx[clear], j[clear])
    # ties and NaN rows: the lowest index wins, NaN rows neither match nor are matched
    T = np.concatenate([Ft[:5], Ft[:5]]); T[1] = np.nan
    Q = np.concatenate([Ft[:5], np.full((1, 33), np.nan, np.float32)])
    assert gr.match_rows(Q, T).tolist() == [0, 6, 2, 3, 4, -1]
    assert gr.match_rows(Q, T[:0]).tolist() == [-1] * 6


def test_ransac_recovers_a_known_pose_through_outliers():
    rng = np.random.default_rng(11)
    n = 200
    s = (rng.uniform(-0.05, 0.05, (n, 3))).astype(np.float32)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(1.3) * K + (1 - np.cos(1.3)) * (K @ K)
    tr = np.array([0.03, -0.07, 0.02])
    t = (s.astype(np.float64) @ R.T + tr).astype(np.float32)
    out = rng.permutation(n)[:60]                                                  # 30 % outliers
    t[out] = rng.uniform(-0.1, 0.1, (60, 3)).astype(np.float32)
    r = gr.ransac(s, t, seed=3, H=4096, edge_similarity=0.9, inlier_distance=0.005)
    assert (r["status"] == gr.REPEATED).sum() > 0 and (r["status"] == gr.EDGES).sum() > 0 and (r["status"] == gr.VALID).sum() > 100
    best = r["order"][0]
    assert r["n_inliers"][best] >= 140
    P = r["poses"][best].reshape(4, 4).T.astype(np.float64)
    from conftest import pose_error
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = tr
    ang, dist = pose_error(P, T)
    # exact inliers: the fit errs by the fp32 rounding of the points (3e-9 m) over the triangle's size, far below these
    assert ang < 1e-4 and dist < 1e-5, (ang, dist)
    # the ranking: inliers descending, then the sum ascending, then h
    o = r["order"]
    key = list(zip(-r["n_inliers"][o].astype(int), r["sum_d2"][o], o))
    assert key == sorted(key) and (r["status"][o] == gr.VALID).all()


def test_rows_form_equals_the_full_call(bunny, source_features):
    """neighbour_lists and spfh with rows = ... give the rows of the full call: what lets a large cloud be checked on a sample."""
    f = source_features
    p, nr = bunny["src_pts"], bunny["src_nrm"]
    rows = np.sort(np.random.default_rng(3).choice(len(p), 100, replace=False))
    idx, d2 = gr.neighbour_lists(p, 10, rows=rows)
    assert np.array_equal(idx, f["idx"][rows]) and np.array_equal(d2.view(np.uint32), f["d2"][rows].view(np.uint32))
    counts, pairs, margin, gap = gr.spfh(p, nr, idx, d2, rows=rows)
    assert np.array_equal(counts, f["counts"][rows]) and np.array_equal(pairs, f["pairs"][rows])
    assert np.array_equal(margin, f["margin"][rows]) and np.array_equal(gap, f["gap"][rows])
    q = p.copy(); q[rows[0]] = np.nan                                    # a non-finite row has no list, in either form
    a, b = gr.neighbour_lists(q, 10, rows=rows[:3]), gr.neighbour_lists(q, 10)
    assert (a[0][0] == -1).all() and np.isinf(a[1][0]).all() and np.array_equal(a[0], b[0][rows[:3]])


# ---- the conditions the device tests of tests/test_gpu_global.py rely on, proved with the restatement alone ----
EXCLUDE_MARGIN, EXCLUDE_GAP = 1e-6, 1e-9          # tests/test_gpu_global.py's


@pytest.mark.parametrize("k", [5, 10, 20])
def test_lattices_tie_in_every_list(k):
    """(a) every neighbour list of the integer lattices holds an exact fp32 distance tie, no point would be excluded from the SPFH
    comparison, and every point has a feature."""
    for name, (p, nr) in gc.lattices().items():
        f = gr.features(p, nr, k)
        assert (np.diff(f["d2"], axis=1) == 0).any(axis=1).all(), name
        assert f["margin"].min() >= EXCLUDE_MARGIN and f["gap"].min() >= EXCLUDE_GAP, (name, f["margin"].min(), f["gap"].min())
        assert not np.isnan(f["F"]).any(), name


def strip_pairs(cloud, mutual):
    p, nr = cloud
    f = gr.features(p, nr, 10)
    assert not np.isnan(f["F"]).any() and f["margin"].min() >= EXCLUDE_MARGIN and f["gap"].min() >= EXCLUDE_GAP
    si, ti = gr.correspondences(f["F"], f["F"], 1, mutual)
    assert np.array_equal(si, np.arange(len(p))) and np.array_equal(ti, si)          # a cloud against itself: every pair (i, i)
    return p[si], p[ti]


@pytest.mark.parametrize("mutual", [True, False])
def test_line_cloud_has_repeated_and_degenerate_hypotheses_only(mutual):
    """(b)"""
    cs, ct = strip_pairs(gc.line_cloud(), mutual)
    assert len(cs) >= 3
    r = gr.ransac(cs, ct, gc.LINE_SEED, gc.LINE_H, 0.9, 0.005)
    count = np.bincount(r["status"], minlength=4)
    assert count[gr.VALID] == 0 and count[gr.EDGES] == 0 and count[gr.REPEATED] > 0 and count[gr.DEGENERATE] > 400, count
    assert len(r["order"]) == 0


def test_ribbon_cloud_straddles_the_collinearity_threshold():
    """(c) both VALID and DEGENERATE, each at least a tenth of the non-repeated hypotheses, and every one of them farther from the threshold
    than RIBBON_BAND (relative): the device and the restatement evaluate the same fp64 expression, so their statuses must be equal."""
    cs, ct = strip_pairs(gc.ribbon_cloud(), True)
    r = gr.ransac(cs, ct, gc.RIBBON_SEED, gc.RIBBON_H, 0.9, 0.005)
    count = np.bincount(r["status"], minlength=4)
    tried = count[gr.VALID] + count[gr.DEGENERATE]
    assert count[gr.EDGES] == 0 and tried == gc.RIBBON_H - count[gr.REPEATED]
    assert count[gr.VALID] >= 0.1 * tried and count[gr.DEGENERATE] >= 0.1 * tried, count
    sel = r["status"] != gr.REPEATED
    for side in (cs, ct):
        cc, thr = gc.collinearity(np.asarray(side, np.float32)[r["draws"][sel]].astype(np.float64))
        assert (thr > 0).all() and (np.abs(cc - thr) > gc.RIBBON_BAND * thr).all(), (np.abs(cc - thr) / thr).min()
        assert np.array_equal(~(cc > thr), r["status"][sel] == gr.DEGENERATE)


def test_bunny_sub_clouds_give_m_equal_n(bunny):
    """(d) without the mutual test n source points against the whole target give M = n, no point near a bin boundary; with the edge test
    off every case but the two whose pairs share a target point has valid hypotheses."""
    ft = gr.features(bunny["tgt_pts"], bunny["tgt_nrm"], gc.SUB_K)
    assert ft["margin"].min() >= EXCLUDE_MARGIN and ft["gap"].min() >= EXCLUDE_GAP
    assert {n for n, start, H in gc.EDGE_CASES if start == 0} == set(gc.SUB_SIZES)
    for n, start in sorted({(n, start) for n, start, H in gc.EDGE_CASES}):
        sp, sn, _, _ = gc.sub_clouds(bunny, n, start)
        f = gr.features(sp, sn, gc.SUB_K)
        assert f["margin"].min() >= EXCLUDE_MARGIN and f["gap"].min() >= EXCLUDE_GAP, n
        si, ti = gr.correspondences(f["F"], ft["F"], 1, False)
        assert len(si) == n and np.array_equal(si, np.arange(n)), n
        r = gr.ransac(sp[si], bunny["tgt_pts"][ti], gc.edge_seed(n, start, 512), 512, 0.0, 0.005)
        count = np.bincount(r["status"], minlength=4)
        if (n, start) in ((3, 0), (4, 0)):
            assert count[gr.VALID] == 0 and count[gr.DEGENERATE] > 100, (n, start, count)
        else:
            assert count[gr.VALID] > 100, (n, start, count)


def test_n_best_case_has_fewer_valid_hypotheses_than_n_best(bunny, source_features):
    """N_BEST_H hypotheses on the bunny leave between 65 and 255 valid ones: more than one 64-start block of the multi-start score fold,
    fewer than n_best = 256."""
    ft = gr.features(bunny["tgt_pts"], bunny["tgt_nrm"], gc.N_BEST_K)
    si, ti = gr.correspondences(source_features["F"], ft["F"], 1, True)
    r = gr.ransac(bunny["src_pts"][si], bunny["tgt_pts"][ti], 0, gc.N_BEST_H, 0.9, 0.005)
    assert 65 <= len(r["order"]) <= 255, len(r["order"])


def test_coincident_cloud_has_more_copies_than_k():
    p, nr, copies = gc.coincident_cloud()
    assert len(copies) == gc.COPIES > 20 and (p[copies] == p[gc.COPY_AT]).all()
    f = gr.features(p, nr, 20)
    assert (f["d2"][copies] == 0).all() and np.isin(f["idx"][copies], copies).all()        # the 20 lowest-index copies, all at d2 = 0
    assert (f["idx"][copies] == copies[:20]).all()
    assert (f["pairs"][copies] == 0).all() and np.isnan(f["F"][copies]).all()
    rest = np.setdiff1d(np.arange(len(p)), copies)
    assert not np.isnan(f["F"][rest]).any() and f["margin"].min() >= EXCLUDE_MARGIN and f["gap"].min() >= EXCLUDE_GAP


MATCHER_VGPR_BUDGET = 96            # the 36 KiB tile allows four blocks (16 waves) per CU; 96 registers keep five waves per SIMD possible


def test_new_kernels_have_no_scratch_and_the_matcher_keeps_its_budget():
    seen = kernel_resources(device_asm())

    def kernels(prefix):
        return {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev" + prefix)}
    for prefix, count in (("11k_fpfh_spfhILi", 3), ("6k_fpfhE", 1), ("15k_feature_matchE", 1), ("12k_ransac_fitE", 1), ("14k_ransac_scoreE", 1)):
        ks = kernels(prefix)
        assert len(ks) == count, (prefix, list(ks))
        for name, f in ks.items():
            assert f["private_seg_size"] == 0, (name, f)
    (name, f), = kernels("15k_feature_matchE").items()
    assert f["num_vgpr"] <= MATCHER_VGPR_BUDGET and f["num_agpr"] == 0, (name, f)
