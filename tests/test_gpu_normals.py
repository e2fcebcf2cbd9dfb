"""k-NN normals on the device (k_normals_knn<K> behind icp_estimate_normals, PointCloud.h:41-76) against the oracle's
orc_estimate_normals, on EVERY point.

The oracle restates the device contract (neighbour set = the k smallest (fp32 d2, index) pairs, fp64 mean / covariance in
neighbour order, the same cyclic fp64 Jacobi, flip and curvature; icp_oracle.cpp), so a correct kernel lands within a few fp32
ulps of it everywhere, and one wrong neighbour moves a normal by orders of magnitude more.  Per point:
  * the NaN patterns of normals and curvature are identical;
  * |n_dev - n_orc| <= 2e-6 (max over components) and |curv_dev - curv_orc| <= 2e-6;
  * except where the oracle's neighbourhood has no usable eigen-gap (l1 - l0 <= 1e-9 lmax: collinear or isotropic points,
    direction not unique): there n_dev^T C n_dev <= l0 + 1e-9 lmax with C from the oracle's neighbour set, |n_dev| = 1 and the
    flip towards the viewpoint holds.  Curvature is compared on every point.
No point is skipped.  The fraction of bit-identical normals is reported, not asserted (fp64 sqrt / division on gfx950 are not
known to round like the host's).  PCL parity stays unpinned (PCL absent): see orc_estimate_normals.
"""
import numpy as np
import pytest

from support import check_normals

pytestmark = pytest.mark.gpu
f32 = np.float32


def dev_vs_oracle(ctx, orc, pts, k, vp=(0.0, 0.0, 0.0), label=""):
    nrm, curv = ctx.estimate_normals(pts, k, np.asarray(vp, f32))
    s = check_normals(orc, pts, k, vp, nrm, curv, label)
    print("normals %(label)s: n=%(n)d normals=%(n_normals)d ambiguous=%(n_ambiguous)d worst |dn|=%(worst_nrm).3g "
          "worst |dcurv|=%(worst_curv).3g bit-identical=%(bit_identical).6f" % s)
    return nrm, curv, s


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


@pytest.fixture(scope="module")
def scans():
    from icp_amd import synth
    T = synth.scan_pose(0)
    noisy, _, _ = synth.laser_scan(T, 3, n_tilt=40, n_beam=160, sigma=0.01)
    clean, _, _ = synth.laser_scan(T, 3, n_tilt=40, n_beam=160, sigma=0.0)
    return dict(noisy=noisy, clean=clean, sensor=T[:3, 3].astype(f32))


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7, 8])
def test_k_sweep_on_scans(ctx, orc, scans, k):
    """Every K instantiation, on a noisy scan and on a noise-free one (grid-pattern near-ties between beams)."""
    for name in ("noisy", "clean"):
        dev_vs_oracle(ctx, orc, scans[name], k, scans["sensor"], "%s k=%d" % (name, k))


@pytest.mark.parametrize("k", [3, 5, 8])
def test_block_and_tree_edges(ctx, orc, k):
    """Cloud sizes around K, the 256-thread block and the leaf / tree-level boundaries."""
    rng = np.random.default_rng(100 + k)
    for n in sorted({3, 4, k - 1, k, k + 1, 255, 256, 257, 4097}):
        pts = rng.uniform(-1, 1, (n, 3)).astype(f32)
        dev_vs_oracle(ctx, orc, pts, k, (0.1, 3.0, -2.0), "uniform n=%d k=%d" % (n, k))


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7, 8])
def test_exact_ties_on_lattices(ctx, orc, k):
    """Integer lattices: nearly every neighbourhood has exact fp32 distance ties, decided by the lowest index."""
    g = np.arange(40, dtype=f32)
    plane = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((40, 40), 3, f32)], -1).reshape(-1, 3)
    h = np.arange(14, dtype=f32)
    block = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    shuffled = block[np.random.default_rng(k).permutation(len(block))]
    for name, pts in (("plane", plane), ("block", block), ("shuffled block", shuffled)):
        dev_vs_oracle(ctx, orc, pts, k, (-5.5, 7.25, 30.0), "lattice %s k=%d" % (name, k))


def test_repeats_and_degenerate_shapes(ctx, orc):
    """Duplicated points, a cloud of one point, collinear points, NaN / inf holes, fewer than 3 finite points, all NaN."""
    rng = np.random.default_rng(5)
    base = rng.normal(0, 1, (700, 3)).astype(f32)
    pairs = base[rng.permutation(np.repeat(np.arange(700), 2))]
    one = np.tile(np.array([[0.5, -1.25, 2.0]], f32), (600, 1))
    t = rng.uniform(0, 10, (500, 1)).astype(f32)
    line = t * np.array([[0.6, 0.0, 0.8]], f32) + np.array([[1, 2, 3]], f32)
    holes = rng.normal(0, 1, (3000, 3)).astype(f32)
    holes[rng.choice(3000, 300, replace=False)] = np.nan
    holes[rng.choice(3000, 100, replace=False), rng.integers(0, 3, 100)] = np.inf
    holes[rng.choice(3000, 50, replace=False), 2] = -np.inf
    two = np.full((300, 3), np.nan, f32); two[10] = [1, 2, 3]; two[200] = [1, 2, 3.5]
    three = np.full((300, 3), np.nan, f32); three[[7, 150, 299]] = [[1, 2, 3], [1, 2, 3.5], [1.5, 2, 3]]
    cases = [("pairs", pairs, 5), ("one point", one, 5), ("one point", one, 8), ("line", line, 5), ("line", line, 3),
             ("holes", holes, 5), ("holes", holes, 8), ("two finite", two, 5), ("three finite", three, 5)]
    for name, pts, k in cases:
        for vp in ((0, 0, 0), (4, -3, 1)):
            dev_vs_oracle(ctx, orc, pts, k, vp, "%s k=%d vp=%s" % (name, k, vp))
    for n in (1, 2, 3, 1000):
        nrm, curv, _ = dev_vs_oracle(ctx, orc, np.full((n, 3), np.nan, f32), 5, label="all NaN n=%d" % n)   # ICP_OK, NaN everywhere
        assert np.isnan(nrm).all() and np.isnan(curv).all()
    nrm, _, _ = dev_vs_oracle(ctx, orc, one, 4, (9, 0, 0), "one point, viewpoint +x")
    assert (nrm == np.array([1, 0, 0], f32)).all()
    nrm, _, _ = dev_vs_oracle(ctx, orc, three, 5, (0, 0, 0), "three finite")
    assert np.isfinite(nrm[[7, 150, 299]]).all()


def test_scale_extremes(ctx, orc, scans):
    """Clusters 1e-3 apart beside clusters 1e2 apart, and a whole scan offset by 1e4 m (fp32 spacing ~1e-3 there)."""
    rng = np.random.default_rng(9)
    tight = (rng.integers(0, 6, (40, 3)) * f32(1e-3))[:, None, :] + rng.normal(0, 1e-4, (40, 25, 3))
    wide = (rng.integers(-3, 4, (40, 3)) * f32(1e2))[:, None, :] + rng.normal(0, 1.0, (40, 25, 3))
    mixed = np.concatenate([tight.reshape(-1, 3), wide.reshape(-1, 3)]).astype(f32)
    mixed = mixed[rng.permutation(len(mixed))]
    for k in (3, 5, 8):
        dev_vs_oracle(ctx, orc, mixed, k, (0.5, 0.5, 500.0), "mixed scales k=%d" % k)
    off = (scans["noisy"].astype(np.float64) + 1e4).astype(f32)
    dev_vs_oracle(ctx, orc, off, 5, scans["sensor"] + f32(1e4), "offset 1e4")


def test_full_size_scan_k5(ctx, orc):
    """One 370 488-point scan (344 x 1077, synth.laser_scan defaults) at k = 5: what prepare_pair runs on ETH data, deep tree."""
    from icp_amd import synth
    T = synth.scan_pose(1)
    pts, _, _ = synth.laser_scan(T, 11)
    assert len(pts) == 370488
    _, _, s = dev_vs_oracle(ctx, orc, pts, 5, (0, 0, 0), "full size k=5")
    assert s["n_normals"] > 0.9 * len(pts)


def test_context_state_untouched(gpu_ctx_factory, orc):
    """icp_estimate_normals between set_target / set_source and run reuses tgt_flag and staging as scratch: the run's pose and
    records stay bit-identical to a run without it."""
    from icp_amd import synth
    p = synth.eth_like_pair(0, n_tilt=43, n_beam=135)
    other = synth.laser_scan(synth.scan_pose(2), 4, n_tilt=60, n_beam=200)[0]     # larger than either cloud: scratch regrows
    results = []
    for between in (False, True):
        c = gpu_ctx_factory()
        c.params.max_distance = 0.5; c.params.metric = 1; c.params.n_iterations = 10; c.params.knn_backend = 1
        c.push_params()
        c.set_target(p["tgt_pts"], p["tgt_nrm"]); c.set_source(p["src_pts"], p["src_nrm"])
        if between:
            nrm, curv = c.estimate_normals(other, 6, (1, 2, 3))
            check_normals(orc, other, 6, (1, 2, 3), nrm, curv, "between set_source and run")
        pose, recs, _ = c.run(np.eye(4))
        results.append((pose, recs))
    (pa, ra), (pb, rb) = results
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert len(ra) == len(rb) > 0
    for a, b in zip(ra, rb):
        assert a["n_src"] == b["n_src"] and a["n_valid"] == b["n_valid"] and a["status"] == b["status"]
        assert np.array_equal(a["pose"].view(np.uint32), b["pose"].view(np.uint32))
        assert np.array_equal(np.float32([a["rmse"], a["benchmark_error"]]).view(np.uint32), np.float32([b["rmse"], b["benchmark_error"]]).view(np.uint32))


def test_bad_k_is_rejected_and_context_stays_usable(ctx, orc):
    from icp_amd import binding
    pts = np.random.default_rng(1).normal(0, 1, (500, 3)).astype(f32)
    for k in (2, 9, 0, -1):
        with pytest.raises(binding.IcpError) as e:
            ctx.estimate_normals(pts, k)
        assert e.value.code == 1                                                      # ICP_ERR_INVALID_ARG
    dev_vs_oracle(ctx, orc, pts, 5, (0, 0, 0), "after rejected k")
