"""The bilateral depth filter off the device: the options check, the host-built tables, the properties of the
contract as the numpy restatement states it, the Python plumbing, and the outcome fixture's normals.  No GPU."""
import ctypes
import json
import os
import re
import numpy as np
import pytest

import depth_filter_restatement as DF
import depth_filter_outcome_fixture as XF
from icp_amd import binding

f32 = np.float32
MINF = f32(-np.inf)
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def tables(**kw):
    o = dict(radius=3, sigma_space=4.5, sigma_range=0.03); o.update(kw)
    return (o["radius"],) + binding.depth_filter_tables(**o)


def ulps(a, b):
    """|a - b| in units of the last place of b (fp32, same sign, finite)."""
    ia = np.ascontiguousarray(a, f32).view(np.int32).astype(np.int64); ib = np.ascontiguousarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def noisy_plane(w, h, seed, holes=0.05):
    r = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = (1.5 + 0.002 * u + 0.001 * v + r.normal(0, 0.003, (h, w))).astype(f32)
    d[r.random((h, w)) < holes] = MINF
    return d


def test_options_check_refuses_each_bad_field_and_accepts_the_defaults():
    lib = binding.load_library()
    o = binding.depth_filter_options()
    assert (o.radius, f32(o.sigma_space), f32(o.sigma_range)) == (0, f32(4.5), f32(0.03))
    chk = lambda **kw: lib.icp_depth_filter_options_check(ctypes.byref(binding.depth_filter_options(**kw)))
    assert chk() == 0 and lib.icp_depth_filter_options_check(None) == 1 and lib.icp_depth_filter_options_default(None) == 1
    for r in (1, 2, 3, 4):
        assert chk(radius=r) == 0
    for bad in (dict(radius=-1), dict(radius=5), dict(sigma_space=0.0), dict(sigma_space=-1.0), dict(sigma_space=float("nan")), dict(sigma_space=float("inf")),
                dict(sigma_range=0.0), dict(sigma_range=-0.03), dict(sigma_range=float("nan")), dict(sigma_range=float("inf")),
                dict(sigma_range=1e-19)):                 # 256 / (9 * 1e-38) overflows fp32
        assert chk(**bad) == 1, bad
        with pytest.raises(binding.IcpError):
            binding.depth_filter_tables(**bad)
    assert chk(sigma_range=1e-18) == 0                     # 2.8e37: still finite
    # the setters and getters refuse a null context without touching a device
    assert lib.icp_set_depth_filter_options(None, None) == 1 and lib.icp_get_depth_filter_options(None, ctypes.byref(o)) == 1
    assert lib.icp_filter_depth(None, None, 1, 1, None, None) == 1


def test_header_declares_the_filter():
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for name in ("icp_depth_filter_options_default", "icp_depth_filter_options_check", "icp_set_depth_filter_options", "icp_get_depth_filter_options",
                 "icp_depth_filter_tables", "icp_filter_depth"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and name in binding.EXPORTS, name
    assert "typedef struct icp_depth_filter_options" in hdr and ctypes.sizeof(binding.IcpDepthFilterOptions) == 12
    assert "ICP_DEPTH_FILTER_TILE_W = %d, ICP_DEPTH_FILTER_TILE_H = %d" % binding.DEPTH_FILTER_TILE in hdr


@pytest.mark.parametrize("radius, ss, sr", [(1, 4.5, 0.03), (2, 1.0, 0.01), (3, 4.5, 0.03), (4, 0.7, 0.2), (4, 30.0, 1e-3)])
def test_tables_are_fp64_exp_rounded_once(radius, ss, sr):
    r, S, R, ib = tables(radius=radius, sigma_space=ss, sigma_range=sr)
    ss64, sr64 = np.float64(f32(ss)), np.float64(f32(sr))          # the options are fp32 fields
    dy, dx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    S_ref = np.exp(-(dx * dx + dy * dy).astype(np.float64) / (2.0 * ss64 * ss64)).astype(f32)
    R_ref = np.exp(-4.5 * (np.arange(256, dtype=np.float64) + 0.5) / 256.0).astype(f32)
    assert S.shape == (2 * r + 1, 2 * r + 1) and R.shape == (256,)
    assert ulps(S, S_ref).max() <= 1 and ulps(R, R_ref).max() <= 1
    assert ulps(ib, f32(256.0 / (9.0 * sr64 * sr64))) <= 1
    assert (np.diff(R.astype(np.float64)) < 0).all() and R[0] < 1 and R[255] > 0            # strictly decreasing
    assert S[r, r] == f32(1) and np.array_equal(S, S.T) and np.array_equal(S, S[::-1, :]) and np.array_equal(S, S[:, ::-1])
    # the range table does not depend on the options
    assert np.array_equal(R, binding.depth_filter_tables(radius=1, sigma_space=1.0, sigma_range=0.5)[1])


def test_radius_zero_is_the_identity_and_has_no_spatial_table():
    d = noisy_plane(19, 11, 1)
    d[3, 4] = f32(np.nan)
    S, R, ib = binding.depth_filter_tables(radius=0)
    assert S.shape == (1, 1)
    out = DF.filter_depth(d, 0, S, R, ib)
    assert np.array_equal(out.view(np.uint32), d.view(np.uint32)) and out is not d


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_unusable_centres_pass_through(radius):
    d = noisy_plane(23, 17, 2)
    specials = [MINF, f32(np.nan), f32(np.inf), f32(0), f32(-0.0), f32(-1.25)]
    spots = [(0, 0), (22, 0), (0, 16), (22, 16), (7, 8), (8, 8)]
    for (u, v), s in zip(spots, specials):
        d[v, u] = s
    out = DF.filter_depth(d, *tables(radius=radius))
    bad = ~DF.usable(d)
    assert np.array_equal(out.view(np.uint32)[bad], d.view(np.uint32)[bad])
    assert DF.usable(out[~bad]).all()                     # nothing usable turns into a hole, nothing is filled in


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_a_half_metre_step_does_not_bleed(radius):
    """Two constant halves 0.5 m apart (16.7 sigma_range, far beyond the 3 sigma cut): each side stays within 4 ulp of its constant.
    The halves are 0.5 m and 1.0 m, powers of two: every product w * c is then exact, num is c * den to the bit and the quotient is c
    itself, so any excess over 0 ulp would be depth from the other side.  With constants that are not powers of two the rounding of the
    window's sum alone exceeds 4 ulp at radius >= 2 (the test below measures it): the 4 ulp hold where the products are exact, not in general."""
    d = np.empty((21, 30), f32)
    d[:, :15] = f32(0.5); d[:, 15:] = f32(1.0)
    out = DF.filter_depth(d, *tables(radius=radius))
    worst = max(ulps(out[:, :15], f32(0.5)).max(), ulps(out[:, 15:], f32(1.0)).max())
    print("radius %d: worst %d ulp" % (radius, worst))
    assert worst <= 4


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_a_half_metre_step_between_general_constants_stays_within_the_sums_rounding(radius):
    """The same step between 1.3 m and 1.8 m.  num and den are recursive fp32 sums of n <= (2r + 1)^2 terms, num's terms rounded products:
    |num / den - c| <= ((n) + (n - 1) + 1) u c to first order (n roundings in num -- its products and sums --, n - 1 in den, one in the
    quotient), and u c < ulp(c), so the output lies within 2 n ulp of c.  That is the bound asserted, with n = (2r + 1)^2: 18, 50, 98 and
    162 ulp.  Depth from the other half would show at a different scale: its smallest possible weight ratio is R[255] S[corner] > 1e-3 of
    one tap, times 0.5 m, more than 1e3 ulp.  Measured with the library's tables: 2, 5, 7 and 7 ulp at radius 1 .. 4."""
    d = np.empty((21, 30), f32)
    d[:, :15] = f32(1.3); d[:, 15:] = f32(1.8)
    out = DF.filter_depth(d, *tables(radius=radius))
    worst = max(ulps(out[:, :15], f32(1.3)).max(), ulps(out[:, 15:], f32(1.8)).max())
    print("radius %d: worst %d ulp (bound %d)" % (radius, worst, 2 * (2 * radius + 1) ** 2))
    assert worst <= 2 * (2 * radius + 1) ** 2


@pytest.mark.parametrize("radius", [1, 3])
def test_a_holes_neighbours_are_computed_without_it(radius):
    d = noisy_plane(17, 13, 3, holes=0.0)
    hole = d.copy(); hole[6, 8] = MINF
    args = tables(radius=radius)
    out = DF.filter_depth(hole, *args)
    for v in range(6 - radius, 6 + radius + 1):
        for u in range(8 - radius, 8 + radius + 1):
            if (u, v) != (8, 6):
                assert DF.filter_pixel(hole, u, v, *args).view(np.uint32) == out[v, u].view(np.uint32)
    # the pixel rule skips the hole: the same value comes out whatever unusable value stands there, and another when a depth does
    for other in (f32(np.nan), f32(0), f32(-3), f32(np.inf)):
        alt = hole.copy(); alt[6, 8] = other
        o2 = DF.filter_depth(alt, *args)
        keep = np.ones_like(d, bool); keep[6, 8] = False
        assert np.array_equal(o2.view(np.uint32)[keep], out.view(np.uint32)[keep])
    full = DF.filter_depth(d, *args)
    assert full[6, 7] != out[6, 7]


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_output_lies_within_the_usable_window_and_matches_the_pixel_rule(radius):
    d = noisy_plane(37, 29, 4)
    d[10:14, 20:30] += f32(0.05)                          # a 5 cm ledge: partly inside the range cut
    args = tables(radius=radius)
    out = DF.filter_depth(d, *args)
    lo, hi = DF.window_bounds(d, radius)
    ok = DF.usable(d)
    assert (out[ok] >= lo[ok]).all() and (out[ok] <= hi[ok]).all()
    r = np.random.default_rng(5)
    for u, v in zip(r.integers(0, 37, 60), r.integers(0, 29, 60)):
        a, b = DF.filter_pixel(d, int(u), int(v), *args), out[v, u]
        assert f32(a).view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), (u, v)


def test_camera_sequence_sigma_defaults_to_the_frames_as_ever():
    from icp_amd import synth
    K0, d0, c0, g0 = synth.camera_sequence(2, 40, 30)
    K1, d1, c1, g1 = synth.camera_sequence(2, 40, 30, sigma=0.0)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(c0, c1)
    _, d2, c2, _ = synth.camera_sequence(2, 40, 30, sigma=0.002)
    both = np.isfinite(d0) & np.isfinite(d2)                  # (the noise draws come before the holes': the holes move)
    assert both.sum() > 0.8 * d0.size and not np.array_equal(d0[both], d2[both]) and np.abs(d0[both] - d2[both]).max() < 0.02


def test_outcome_fixture_normals(orc):
    """On the fixture's noisy 320 x 240 frame (sigma in the JSON), default options at radius 3: the filtered normals lie strictly closer to
    the true ones and no pixel loses its normal.  Figures of the committed fixture (sigma 2 mm): raw 0.77797 rad with 47 658 pixels that
    keep a normal, filtered 0.77740 rad with 47 667; the noise-free frame reads 0.77365 rad -- the back-projection's normal is (-du, -dv, 1)
    normalised with du, dv in metres per pixel, not the surface normal, so most of the angle is that convention's and the noise's share,
    which is what the filter can take away, is small."""
    with open(XF.GOLDEN) as f:
        ref = json.load(f)
    assert ref["sigma_m"] == XF.SIGMA and ref["filter"] == XF.FILTER
    assert ref["raw"]["statuses"] == [0]                   # the sigma was chosen so: the unfiltered run tracks every frame
    K, depth, _, nrm_true = XF.noisy_frames(n_frames=1)
    filt = XF.restatement_filter(depth[0])
    n_raw = orc.backproject(depth[0], None, K, max_distance=XF.MAX_DISTANCE)[1]
    n_filt = orc.backproject(filt, None, K, max_distance=XF.MAX_DISTANCE)[1]
    a_raw, a_filt, k_raw, k_filt = XF.normal_measures(n_raw, n_filt, nrm_true)
    print("normals: raw %.4f rad over %d kept, filtered %.4f rad over %d kept" % (a_raw, k_raw, a_filt, k_filt))
    assert a_filt < a_raw and k_filt >= k_raw
    n = ref["normals"]
    assert (n["raw_kept"], n["filtered_kept"]) == (k_raw, k_filt)
    assert n["raw_mean_angle_rad"] == pytest.approx(a_raw, rel=1e-9) and n["filtered_mean_angle_rad"] == pytest.approx(a_filt, rel=1e-9)
