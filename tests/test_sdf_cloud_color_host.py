"""The photometric scan tracker without a device: that the inputs of tests/sdf_cloud_color_cases.py reach what they
are named for on the restatement (tests/sdf_cloud_color_restatement.py), that the photometric Jacobian is the derivative of r_c, that a
uniform colour field adds nothing to the geometric sums, that the hashed volume cut from the dense one gives the same terms, the outcome
fixture's separation, and the symbols, the Python surface and the refusals that need no device."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import sdf_cloud_cases as K
import sdf_cloud_color_cases as CK
import sdf_cloud_color_outcome_fixture as OF
import sdf_cloud_color_restatement as R
import sdf_cloud_restatement as SC
import sdf_color_restatement as PC
import sdf_restatement as SR
import support as S

f32, f64 = np.float32, np.float64
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_the_special_points_reach_what_they_are_named_for():
    """On the crafted model at START: the point over the Wc == 0 corner and the one over the inf are valid and not coloured, and without the
    crafting both are coloured; black, white and the twins are coloured; the twins' terms are equal; the points without a valid cell are
    not coloured whatever their bytes; a hashed volume gives the same counts and sums."""
    pts, rgba, names, crafted = CK.special()
    vol, plain = CK.special_model(), CK.colored_model(False, True)
    t, t0 = R.point_terms(vol, pts, rgba, CK.START), R.point_terms(plain, pts, rgba, CK.START)
    for name in ("wc_zero", "s_inf"):
        i = names[name]
        assert t["valid"][i] and not t["colored"][i] and t0["colored"][i], name
    assert not np.isfinite(t["S"][names["s_inf"]]) and np.isfinite(t["S"][names["wc_zero"]])
    # exactly one corner of wc_zero's cell has Wc == 0
    c = CK.cell_of(vol, t["q"][names["wc_zero"]])
    assert c == crafted["wc_zero"] and int((vol.wc[c[2]:c[2] + 2, c[1]:c[1] + 2, c[0]:c[0] + 2] == 0).sum()) == 1
    for name in ("black", "white", "alpha_00", "alpha_ff"):
        assert t["colored"][names[name]], name
    assert tuple(rgba[names["black"]][:3]) == (0, 0, 0) and tuple(rgba[names["white"]][:3]) == (255, 255, 255)
    a, b = names["alpha_00"], names["alpha_ff"]
    assert rgba[a][3] == 0x00 and rgba[b][3] == 0xFF and np.array_equal(rgba[a][:3], rgba[b][:3]) and S.same_bits(pts[a], pts[b])
    terms = R.terms_of(t)
    col = np.cumsum(t["valid"]) - 1
    assert np.array_equal(terms[:, col[a]].view(np.uint64), terms[:, col[b]].view(np.uint64)) and terms[28, col[a]] > 0
    for name in ("unobserved", "free", "below_x", "above_z", "nan", "inf"):
        i = names[name]
        assert not t["valid"][i] and not t["colored"][i], name
    assert rgba[names["free"]][:3].any() and t["considered"][names["free"]]
    counts, sums, mag = R.system(vol, pts, rgba, CK.START, weight=CK.WEIGHT)
    assert counts[0] == len(pts) - 3 and counts[2] < counts[1] < counts[0] and counts[2] > 100
    hcounts, hsums, _ = R.system(CK.special_model(True), pts, rgba, CK.START, weight=CK.WEIGHT)
    assert hcounts == counts and np.array_equal(hsums.view(np.uint64), sums.view(np.uint64))
    # flipping every fourth byte changes nothing
    flipped = rgba.copy(); flipped[:, 3] ^= 0xFF
    assert np.array_equal(R.system(vol, pts, flipped, CK.START, weight=CK.WEIGHT)[1].view(np.uint64), sums.view(np.uint64))


def test_the_photometric_jacobian_is_the_derivative_of_r_c():
    """J_c = (q x h, h) against central differences of r_c under a left-multiplied twist (the solve's parametrisation: q -> q + w x q + v), on
    the smooth colours, for points well inside a cell (the field is trilinear inside one)."""
    vol = CK.colored_model()
    pts = K.cloud(400, seed=21)
    rgba = CK.wall_colors(pts, seed=21)
    t = R.point_terms(vol, pts, rgba, K.EYE)
    frac = (t["q"].astype(f64) - vol.o.astype(f64)) / float(vol.s)
    frac -= np.floor(frac)
    inner = t["colored"] & ((frac > 0.2) & (frac < 0.8)).all(1)
    assert inner.sum() > 50
    q = t["q"][inner].astype(f64); rg = rgba[inner]
    J = SR.jacobian(t["q"][inner], t["h"][inner])
    eps = 2e-3                                           # (2 mm of a 100 mm cell: the moved point stays in its cell)
    worst = 0.0
    for a in range(6):
        d = np.zeros(6); d[a] = eps
        move = lambda sgn: (q + sgn * (np.cross(np.broadcast_to(d[:3], q.shape), q) + d[3:])).astype(f32)
        rp = R.point_terms(vol, move(+1), rg, K.EYE)["r_c"]; rm = R.point_terms(vol, move(-1), rg, K.EYE)["r_c"]
        fd = (rp - rm) / (2 * eps)
        worst = max(worst, float(np.abs(fd - J[:, a]).max() / max(np.abs(J[:, a]).max(), 1e-12)))
    print("worst |finite difference - J_c| / max |J_c| = %.3g" % worst)
    # fp32 positions (2^-24 of 4 m) over a 4 mm baseline against gradients of order 1 per metre, and the rotation's second-order term
    assert worst < 2e-3


def test_a_uniform_colour_field_adds_nothing():
    """Every voxel (90, 80, 70) and every point of that colour: r_c and h vanish, so the sums 0 .. 26 are the geometric restatement's within
    n_valid 2^-52 sum |term| (here: equal bits), entry 28 is 0, and every valid point is coloured."""
    import copy
    vol = copy.deepcopy(CK.colored_model())
    vol.rgb[:] = np.array([90, 80, 70], f32)
    pts = K.cloud(3000, seed=5)
    rgba = np.tile(np.array([90, 80, 70, 255], np.uint8), (len(pts), 1))
    counts, sums, _ = R.system(vol, pts, rgba, K.START, weight=CK.WEIGHT)
    gcounts, gsums, gabs = SC.system(K.model(), pts, K.START)
    assert counts == (gcounts[0], gcounts[1], gcounts[1]) and sums[28] == 0.0
    assert (np.abs(sums[:27] - gsums[:27]) <= gcounts[1] * 2.0 ** -52 * gabs[:27]).all()
    # and with another colour on the points the photometric cost is what moves
    rgba[:, 0] = 120
    assert R.system(vol, pts, rgba, K.START, weight=CK.WEIGHT)[1][28] > 0


def test_plane_volumes_and_the_alignment():
    """The coloured plane volumes: inside cells are valid and coloured, outside cells neither, on the hashed blocks, the covering box and
    the dense box; the photometric alignment of the wall from START converges towards the identity."""
    for vol, (inside, outside) in ((CK.plane_hashed(), K.straddle_cells()), (CK.plane_dense(), K.face_cells())):
        pin, pout = K.cell_points(vol, inside), K.cell_points(vol, outside, seed=1)
        rg = CK.wall_colors(np.concatenate([pin, pout]))
        counts = R.system(vol, np.concatenate([pin, pout]), rg, K.EYE)[0]
        assert counts == (len(pin) + len(pout), len(pin), len(pin))
    pin = K.cell_points(CK.plane_hashed(), K.straddle_cells()[0])
    rg = CK.wall_colors(pin)
    a, b = R.system(CK.plane_hashed(), pin, rg, K.EYE), R.system(CK.plane_cover(), pin, rg, K.EYE)
    assert a[0] == b[0] and np.allclose(a[1], b[1], rtol=1e-3, atol=1e-9)      # (another origin: other fp32 fractions, the same field)
    pts = K.cloud(3000, seed=5)
    pose, rec, trace = R.align(CK.colored_model(), pts, CK.wall_colors(pts, seed=5), K.START, weight=CK.WEIGHT)
    err0, err1 = np.abs(K.START - K.EYE).max(), np.abs(pose - K.EYE).max()
    assert rec["status"] == 0 and 1 < rec["iterations"] < 20 and err1 < 0.5 * err0 and rec["n_color_first"] > 1000
    assert rec["cost_color_last"] < rec["cost_color_first"]


def test_outcome_the_fixture_separates_the_two_trackers():
    """The flat textured wall tracked by both restatements: the photometric loop stays within a quarter of what the geometric one loses, every
    photometric alignment is ICP_OK, and tests/golden/sdf_cloud_color_outcome.json records these runs."""
    colored, geometric, truth = OF.restatement_tracks()
    ec, eg = OF.translation_errors(colored[0], truth), OF.translation_errors(geometric[0], truth)
    print("photometric worst %.4f m, geometric last %.4f m of %.3f m" % (max(ec), eg[-1], OF.TRAVEL))
    assert 2 * max(ec) < OF.TRAVEL / 2 < eg[-1]
    assert colored[3] == 0 and all(r["status"] == 0 for r in colored[1]) and all(n > 0 for n in colored[4])
    g = OF.golden()
    assert abs(g["colored_worst_translation_m"] - max(ec)) < 1e-6 and abs(g["geometric_last_translation_m"] - eg[-1]) < 1e-6
    assert g["lateral_travel_m"] == OF.TRAVEL and g["scans"] == OF.N_SCANS and g["points_per_scan"] == 11200
    assert os.path.getsize(OF.GOLDEN) < 4096 and json.dumps(g)


def test_symbols_python_surface_and_refusals_without_a_device():
    from icp_amd import binding, eth
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for sym in ("icp_tsdf_cloud_system_color", "icp_tsdf_align_cloud_color", "icp_track_scans_sdf_photometric"):
        assert sym in binding.EXPORTS and hasattr(lib, sym) and re.search(r"^int %s\(icp_ctx\* ctx, " % sym, hdr, flags=re.M), sym
    assert hasattr(lib, "icp_debug_sdf_cloud_color_time") and "icp_debug_sdf_cloud_color_time" not in hdr
    p = binding.pose_to_c(np.eye(4)); o = binding.sdf_options(); co = binding.sdf_color_options()
    sums = np.zeros(29); cnt = (ctypes.c_int32 * 3)(); ms = ctypes.c_float(0)
    assert lib.icp_tsdf_cloud_system_color(None, 1, binding._ptr(p), ctypes.byref(o), ctypes.byref(co), binding._ptr(sums), cnt) == 1
    assert lib.icp_tsdf_align_cloud_color(None, 1, ctypes.byref(o), ctypes.byref(co), binding._ptr(p), None, None) == 1
    assert lib.icp_track_scans_sdf_photometric(None, None, None, None, 1, ctypes.byref(o), ctypes.byref(co), binding._ptr(p), None, None, None) == 1
    assert lib.icp_debug_sdf_cloud_color_time(None, 1, binding._ptr(p), ctypes.byref(o), ctypes.byref(co), ctypes.byref(ms)) == 1
    # the keywords ride on the methods whose signatures other tests pin
    assert list(inspect.signature(binding.Context.tsdf_cloud_system).parameters) == ["self", "which", "pose", "huber"]
    assert list(inspect.signature(binding.Context.track_scans_sdf).parameters) == ["self", "scans", "pose", "options"]
    # the Python layer's refusals come before anything touches the context (None)
    scan, col = K.cloud(3), np.zeros((3, 4), np.uint8)
    with pytest.raises(ValueError):
        binding.Context.track_scans_sdf(None, [scan], np.eye(4), color_weight=0.1)                     # no colors
    with pytest.raises(ValueError):
        binding.Context.track_scans_sdf(None, [scan], np.eye(4), colors=[col], color_weight=-0.1)
    with pytest.raises(ValueError):
        binding.Context.tsdf_cloud_system(None, "source", color_weight=float("nan"))
    with pytest.raises(ValueError):
        binding.Context.tsdf_align_cloud(None, "source", color_weight=0.1, color_huber=-1.0)
    with pytest.raises(ValueError):
        binding.Context.tsdf_cloud_system(None, "source", pose=np.eye(3), color_weight=0.1)
    with pytest.raises(KeyError):
        binding.Context.tsdf_align_cloud(None, "neither", color_weight=0.1)
    with pytest.raises(TypeError):                       # the colour keywords do not open the options check to anything else
        binding.Context.track_scans_sdf(None, [scan], np.eye(4), colors=[col], color_weight=0.1, no_such_option=1)
    with pytest.raises(TypeError):
        binding.Context.track_scans_sdf(None, [scan], np.eye(4), color_weight=0.0, no_such_option=1)
    with pytest.raises(ValueError):
        binding.Context.track_scans_sdf(None, [scan], np.eye(4), colors=[col[:2]], color_weight=0.1)
    with pytest.raises(ValueError):
        eth.track_tsdf(None, [scan], np.eye(4), color_weight=0.1)
    with pytest.raises(ValueError):
        eth.reconstruct(None, [scan], np.eye(4), tracker="sdf", color_weight=0.1)
    with pytest.raises(ValueError):
        eth.reconstruct(None, [scan], np.eye(4), tracker="map", colors=[col], color_weight=0.1)
    assert lib.icp_sdf_color_options_check(ctypes.byref(binding.sdf_color_options(weight=0.0))) == 1
