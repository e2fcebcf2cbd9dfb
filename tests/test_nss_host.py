"""Normal-space sampling without a GPU: the numpy restatement (tests/nss_restatement.py) against the library's hash and against the
invariants the contract in include/icp_hip.h implies, and the new structs and defaults of the C ABI."""
import ctypes
import numpy as np
import pytest

import nss_restatement as nss


@pytest.fixture(scope="module")
def bunny_src(bunny):
    return bunny["src_pts"], bunny["src_nrm"]


def test_hash_equals_library_and_oracle(orc):
    from icp_amd import binding
    rng = np.random.default_rng(7)
    seeds = rng.integers(0, 2 ** 32, 40, dtype=np.uint64)
    its = np.concatenate([np.arange(20), rng.integers(0, 2 ** 32, 20, dtype=np.uint64)])
    idx = np.concatenate([np.arange(50), rng.integers(0, 2 ** 32, 50, dtype=np.uint64), [0x80000000, 0x80000125, 0xFFFFFFFF]])
    for s, it in zip(seeds, its):                            # 40 x 103 triples
        mine = nss.select_hash(int(s), int(it), idx)
        assert [int(h) for h in mine] == [binding.select_hash(int(s), int(it), int(i)) for i in idx]
        assert [int(h) for h in mine[::7]] == [int(orc.select_hash(int(s), int(it), int(i))) for i in idx[::7]]


def test_hash_is_a_bijection_of_the_index():
    """Distinct indices, distinct keys (a sample of the claim the no-tie argument rests on)."""
    h = nss.select_hash(3, 11, np.arange(1 << 20))
    assert len(np.unique(h)) == 1 << 20


def test_bunny_bucket_census(bunny_src):
    pts, nrm = bunny_src
    assert len(pts) == 1054
    for grid, non_empty in ((3, 45), (5, 116), (7, 207)):
        b = nss.buckets(pts, nrm, grid)
        assert (b != nss.NONE).all() and b.max() < 6 * grid * grid
        assert len(np.unique(b)) == non_empty
    assert np.bincount(nss.buckets(pts, nrm, 5)).max() == 69


def test_bunny_quota_branches(bunny_src):
    """proba 0.25 on the bunny: M = 264, cap 3, 16 buckets taken whole, 100 capped, 62 of them lose one point to the excess rule."""
    pts, nrm = bunny_src
    cnt = np.bincount(nss.buckets(pts, nrm, 5), minlength=150)
    M = nss.sample_size(0.25, 1054)
    q, c = nss.quotas(cnt, M, 0, 0)
    assert (M, c) == (264, 3)
    whole = (cnt > 0) & (cnt < c); capped = cnt >= c
    assert whole.sum() == 16 and capped.sum() == 100
    assert q.sum() == M
    assert (q[whole] == cnt[whole]).all() and (cnt[whole] < c).all()
    assert (q[capped] == c - 1).sum() == 62 and set(q[capped]) == {c - 1, c}
    assert (q[cnt == 0] == 0).all()


@pytest.mark.parametrize("grid", [3, 5, 7])
@pytest.mark.parametrize("proba", [0.1, 0.25, 0.5, 0.9])
def test_quota_invariants(bunny_src, grid, proba):
    pts, nrm = bunny_src
    cnt = np.bincount(nss.buckets(pts, nrm, grid), minlength=6 * grid * grid)
    M = nss.sample_size(proba, len(pts))
    for it in range(3):
        q, c = nss.quotas(cnt, M, 5, it)
        assert q.sum() == M and (q <= cnt).all()
        capped = cnt >= c
        assert q[capped].max() - q[capped].min() <= 1
        assert (q[~capped] == cnt[~capped]).all()


def test_lists_are_increasing_subsets_and_repeatable(bunny_src):
    pts, nrm = bunny_src
    factors = [4, 2, 1, 1, 1]
    a = nss.run_lists(pts, nrm, factors, 0.25, 9, grid=5, resample=True)
    b = nss.run_lists(pts, nrm, factors, 0.25, 9, grid=5, resample=True)
    for i, (f, l) in enumerate(zip(factors, a)):
        base = nss.base_set(pts, nrm, f)
        assert (np.diff(l) > 0).all() and np.isin(l, base).all()
        assert len(l) == nss.sample_size(0.25, len(base))
        assert np.array_equal(l, b[i])
    assert not np.array_equal(a[2], a[3])                    # two iterations differ
    held = nss.run_lists(pts, nrm, factors, 0.25, 9, grid=5, resample=False)
    assert np.array_equal(held[2], a[2]) and np.array_equal(held[3], a[2]) and np.array_equal(held[4], a[2])
    assert np.array_equal(held[0], a[0]) and np.array_equal(held[1], a[1])


def test_proba_edges(bunny_src):
    pts, nrm = bunny_src
    nrm = nrm.copy(); nrm[5] = 0; nrm[17, 1] = np.nan          # two points without a bucket
    bkt = nss.buckets(pts, nrm, 5)
    base = nss.base_set(pts, nrm, 0)
    sizes = {p: len(nss.draw(bkt, base, p, 1, 0, 150)) for p in (-0.5, 0.0, 1e-9, 1.0, 1.5)}
    assert sizes == {-0.5: 0, 0.0: 0, 1e-9: 1, 1.0: 1052, 1.5: 1052}
    full = nss.draw(bkt, base, 1.0, 1, 0, 150)
    assert 5 not in full and 17 not in full                  # all CANDIDATES, not all points


def test_struct_sizes_and_defaults():
    from icp_amd import binding
    assert ctypes.sizeof(binding.IcpNssOptions) == 8
    assert ctypes.sizeof(binding.IcpParams) == 80
    lib = binding.load_library()
    o = binding.IcpNssOptions(0, 0)
    assert lib.icp_nss_options_default(ctypes.byref(o)) == 0 and (o.grid, o.resample) == (5, 1)
    assert lib.icp_nss_options_default(None) == 1            # ICP_ERR_INVALID_ARG
    assert lib.icp_set_nss_options(None, ctypes.byref(o)) == 1 and lib.icp_get_nss_options(None, ctypes.byref(o)) == 1
    assert lib.icp_get_normal_buckets(None, None, 0, None) == 1 and lib.icp_get_selection(None, 0, None, 0, None) == 1
    assert (binding.SELECT_ALL, binding.SELECT_RANDOM, binding.SELECT_NORMAL_SPACE) == (0, 1, 2)


def test_incised_plane_is_seeded_and_mostly_one_bucket():
    from icp_amd import synth
    a = synth.incised_plane(); b = synth.incised_plane()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["src_pts"].shape == (25600, 3) and a["tgt_pts"].shape == (25600, 3)
    cnt = np.bincount(nss.buckets(a["src_pts"], a["src_nrm"], 5), minlength=150)
    assert cnt.max() > 0.9 * 25600 and (cnt > 100).sum() >= 5      # the plane, and the four groove flanks
