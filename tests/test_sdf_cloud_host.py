"""A laser scan aligned to the TSDF volume without a device: the restatement (tests/sdf_cloud_restatement.py) against
one plain loop per point in numpy float32 scalars, its independence of the cloud's order, the dense volume against the hashed one, that
the inputs of tests/sdf_cloud_cases.py reach what they are named for, the outcome fixture's conditions, and the struct sizes, symbols,
Python surface and refusals that need no device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import sdf_cloud_cases as K
import sdf_cloud_outcome_fixture as OF
import sdf_cloud_restatement as SC
import sdf_restatement as SR
import tsdf_cloud_outcome_fixture as CF
from support import same_bits

f32, f64 = np.float32, np.float64
ROOT = K.ROOT


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def lerp(a, b, t):
    return f32(a + f32(t * f32(b - a)))


def loop_system(vol, pts, pose, huber=0.0):
    """icp_tsdf_cloud_system on a DENSE volume, one point at a time in numpy scalars, written from the header's words."""
    P = np.asarray(pose, f32)
    sums = np.zeros(28, f64); sabs = np.zeros(28, f64)
    n_depth = n_valid = 0
    o, s, tr = vol.o, f32(vol.s), f32(vol.trunc)
    with np.errstate(all="ignore"):
        for x, y, z in np.asarray(pts, f32):
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                continue
            n_depth += 1
            q = [f32(f32(P[r, 0] * x + f32(P[r, 1] * y + P[r, 2] * z)) + P[r, 3]) for r in range(3)]
            g = [f32(f32(q[a] - o[a]) / s) for a in range(3)]
            fl = [np.floor(v) for v in g]
            if not all(fl[a] >= 0 and fl[a] <= f32(n - 2) for a, n in enumerate((vol.nx, vol.ny, vol.nz))):
                continue
            t = [f32(g[a] - fl[a]) for a in range(3)]
            i, j, k = (int(v) for v in fl)
            c = [vol.tsdf[k + (m >> 2), j + ((m >> 1) & 1), i + (m & 1)] for m in range(8)]
            w = [vol.weight[k + (m >> 2), j + ((m >> 1) & 1), i + (m & 1)] for m in range(8)]
            if not all(v > 0 for v in w):
                continue
            tx, ty, tz = t
            F = lerp(lerp(lerp(c[0], c[1], tx), lerp(c[2], c[3], tx), ty), lerp(lerp(c[4], c[5], tx), lerp(c[6], c[7], tx), ty), tz)
            if not abs(F) < 1:
                continue
            n_valid += 1
            G = [lerp(lerp(f32(c[1] - c[0]), f32(c[3] - c[2]), ty), lerp(f32(c[5] - c[4]), f32(c[7] - c[6]), ty), tz),
                 lerp(lerp(f32(c[2] - c[0]), f32(c[3] - c[1]), tx), lerp(f32(c[6] - c[4]), f32(c[7] - c[5]), tx), tz),
                 lerp(lerp(f32(c[4] - c[0]), f32(c[5] - c[1]), tx), lerp(f32(c[6] - c[2]), f32(c[7] - c[3]), tx), ty)]
            r = f64(F) * f64(tr); sc = f64(tr) / f64(s)
            gg = [f64(v) * sc for v in G]; p = [f64(v) for v in q]
            J = [p[1] * gg[2] - p[2] * gg[1], p[2] * gg[0] - p[0] * gg[2], p[0] * gg[1] - p[1] * gg[0], gg[0], gg[1], gg[2]]
            wt = 1.0
            if f32(huber) > 0:
                wt = 1.0 if abs(r) <= f64(f32(huber)) else f64(f32(huber)) / abs(r)
            terms = []
            for a in range(6):
                for b in range(a, 6):
                    terms.append((wt * J[a]) * J[b])
            terms += [-((wt * J[a]) * r) for a in range(6)] + [(wt * r) * r]
            sums += terms; sabs += np.abs(terms)
    return (n_depth, n_valid), sums, sabs


def test_restatement_equals_a_plain_loop_on_the_special_points():
    """About 300 points, among them a NaN, two infinities, an unobserved cell, a cell that reads |F| == 1 exactly and one point outside the box on
    each face: counts equal, every sum within n_valid 2^-52 sum |term| (the terms are the same doubles; only their order differs)."""
    vol = K.model(False, True)
    pts, names = K.special()
    t = SC.point_terms(vol, pts, K.START)
    for n in ("nan", "inf", "minus_inf"):
        assert not t["considered"][names[n]]
    for n in names:
        assert not t["valid"][names[n]], n
    cell = SR._field_and_gradient(vol, *(t["q"][:, a].copy() for a in range(3)))
    assert not cell[0][names["unobserved"]] and t["considered"][names["unobserved"]]
    assert cell[0][names["free"]] and t["F"][names["free"]] == f32(1)                  # a valid cell, dropped by fabsf(F) < 1 alone
    for a in "xyz":
        assert not cell[0][names["below_" + a]] and not cell[0][names["above_" + a]]
    for huber in (0.0, 0.02):
        counts, sums, sabs = SC.system(vol, pts, K.START, huber=huber)
        lcounts, lsums, labs = loop_system(vol, pts, K.START, huber=huber)
        print("special points, huber %g: counts %s" % (huber, counts))
        assert counts == lcounts and counts[0] == len(pts) - 3 and 64 < counts[1] < counts[0] - len(names) + 3
        assert (np.abs(sums - lsums) <= counts[1] * 2.0 ** -52 * sabs).all() and np.allclose(sabs, labs, rtol=1e-12)
    assert SC.system(vol, pts, K.START, huber=0.02)[1][27] < SC.system(vol, pts, K.START)[1][27]


def test_order_independence_and_dense_equals_hashed():
    """A permutation and the reversal give the same counts and sums within n_valid 2^-52 sum |term|; the hashed volume cut from the dense
    one gives the dense volume's terms bit for bit, point for point."""
    vol, hv = K.model(False, True), K.model(True, True)
    pts, _ = K.special()
    counts, sums, sabs = SC.system(vol, pts, K.START)
    perm = np.random.default_rng(4).permutation(len(pts))
    for other in (pts[perm], pts[::-1].copy()):
        c2, s2, a2 = SC.system(vol, other, K.START)
        assert c2 == counts and (np.abs(s2 - sums) <= counts[1] * 2.0 ** -52 * sabs).all()
    td, th = SC.point_terms(vol, pts, K.START), SC.point_terms(hv, pts, K.START)
    assert np.array_equal(td["valid"], th["valid"]) and np.array_equal(td["considered"], th["considered"])
    m = td["valid"]
    assert np.array_equal(u64(td["r"][m]), u64(th["r"][m])) and np.array_equal(u64(td["g"][m]), u64(th["g"][m])) and same_bits(td["q"], th["q"])
    ch, sh, _ = SC.system(hv, pts, K.START)
    assert ch == counts and np.array_equal(u64(sh), u64(sums))
    # the wall cloud too, where most points are valid
    big = K.cloud(3000, seed=5)
    cd, sd, _ = SC.system(K.model(), big, K.START)
    chh, shh, _ = SC.system(K.model(True), big, K.START)
    assert cd == chh and np.array_equal(u64(sd), u64(shh)) and cd[1] > 1000


def test_cases_reach_what_they_are_named_for():
    """The crafted plane volumes: every point of an inside cell is valid, every point of an outside cell is not; the straddling cells read
    corners from more than one block; the alignment of the wall from START converges towards the identity."""
    dv, hv = K.plane_dense(), K.plane_hashed()
    inside, outside = K.face_cells()
    t = SC.point_terms(dv, K.cell_points(dv, inside), K.EYE)
    assert t["valid"].all() and len(t["valid"]) == 6 * 12
    assert not SC.point_terms(dv, K.cell_points(dv, outside), K.EYE)["valid"].any()
    inside, outside = K.straddle_cells()
    assert SC.point_terms(hv, K.cell_points(hv, inside), K.EYE)["valid"].all()
    assert not SC.point_terms(hv, K.cell_points(hv, outside), K.EYE)["valid"].any()
    assert sum(1 for c in inside if -1 in c) >= 5
    pose, rec, trace = SC.align(K.model(), K.cloud(3000, seed=5), K.START, n_iterations=20)
    err0, err1 = OF.pose_error(K.START, K.EYE), OF.pose_error(pose, K.EYE)
    print("wall from START: %d iterations, %.4f rad %.4f m -> %.4f rad %.4f m, %d valid of %d" % ((rec["iterations"],) + err0 + err1 + (rec["n_valid_last"], rec["n_depth"])))
    # (the model averages four copies of the wall displaced by up to 0.04 rad and 0.03 m, so its optimum is the identity only to within that:
    # the alignment has to stop early, move towards the identity on both measures and halve the distance)
    assert rec["status"] == 0 and rec["iterations"] < 20 and err1[0] < err0[0] and err1[1] < 0.5 * err0[1]
    # a failed alignment carries the pose; no considered point is NO_SOURCE
    pose, rec, _ = SC.align(K.model(), K.cloud(30, seed=5), K.START)
    assert rec["status"] == SC.ERR_NO_CORRESPONDENCES and same_bits(pose, K.START) and rec["iterations"] == 1
    pose, rec, _ = SC.align(K.model(), np.full((5, 3), np.nan, f32), K.START)
    assert rec["status"] == SC.ERR_NO_SOURCE and rec["n_depth"] == 0
    with pytest.raises(ValueError):
        SC.align(K.model(), K.cloud(30), K.START, stride=2)


def test_outcome_every_scan_aligns_within_half_a_voxel():
    """The twelve scans tracked by the restatement against the model they build: every scan aligns, the worst ends within 0.02 rad and
    0.05 m of its true pose (recorded: 0.0065 rad, 0.0132 m), and the model the tracked poses built is a surface by tsdf_cloud_outcome_fixture's
    own measure (recorded: 98.1 % valid, median 4.5 mm)."""
    vol, poses, recs, infos, status = OF.tracked()
    OF.assert_outcome(poses, recs, status)
    CF.assert_surface(vol)
    assert len(infos) == CF.N_SCANS and all(i["n_updated"] > 0 for i in infos)


def test_struct_symbol_python_surface_and_refusals_without_a_device():
    from icp_amd import binding, eth
    assert ctypes.sizeof(binding.IcpSdfOptions) == 24 and ctypes.sizeof(binding.IcpSdfFrame) == 104 and ctypes.sizeof(binding.IcpSdfIter) == 80
    assert ctypes.sizeof(binding.IcpTsdfCloudInfo) == 32
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for sym in ("icp_tsdf_cloud_system", "icp_tsdf_align_cloud", "icp_track_scans_sdf"):
        assert sym in binding.EXPORTS and hasattr(lib, sym) and re.search(r"^int %s\(icp_ctx\* ctx, " % sym, hdr, flags=re.M), sym
    assert hasattr(lib, "icp_debug_sdf_cloud_time") and "icp_debug_sdf_cloud_time" not in hdr
    p = binding.pose_to_c(np.eye(4)); o = binding.sdf_options()
    sums = np.zeros(28); cnt = (ctypes.c_int32 * 2)()
    assert lib.icp_tsdf_cloud_system(None, 1, binding._ptr(p), ctypes.byref(o), binding._ptr(sums), cnt) == 1
    assert lib.icp_tsdf_align_cloud(None, 1, ctypes.byref(o), binding._ptr(p), None, None) == 1
    assert lib.icp_track_scans_sdf(None, None, None, 1, ctypes.byref(o), binding._ptr(p), None, None) == 1
    par = inspect.signature(binding.Context.tsdf_cloud_system).parameters
    assert list(par) == ["self", "which", "pose", "huber"] and par["which"].default == "source" and par["huber"].default == 0.0
    par = inspect.signature(binding.Context.tsdf_align_cloud).parameters
    assert list(par) == ["self", "which", "pose", "n_iterations", "huber", "min_valid", "stop_rotation", "stop_translation", "trace"]
    assert [par[k].default for k in list(par)[1:]] == ["source", None, 20, 0.0, 64, 1e-5, 1e-5, False]
    assert list(inspect.signature(binding.Context.track_scans_sdf).parameters) == ["self", "scans", "pose", "options"]
    par = inspect.signature(eth.track_tsdf).parameters
    assert list(par) == ["ctx", "scans", "start_pose", "voxel_size", "truncation", "origin", "max_range", "block_capacity", "hashed", "dims", "sdf_options"]
    assert [par[k].default for k in list(par)[3:10]] == [0.05, None, (0.0, 0.0, 0.0), 30.0, 1 << 14, True, None]
    assert inspect.signature(eth.reconstruct).parameters["tracker"].default == "map"
    # refusals that need no device: the checks of the Python layer come before anything touches the context
    with pytest.raises(ValueError):
        binding.Context.tsdf_cloud_system(None, "source", pose=np.eye(3))
    with pytest.raises(KeyError):
        binding.Context.tsdf_align_cloud(None, "neither")
    with pytest.raises(TypeError):
        binding.Context.track_scans_sdf(None, [K.cloud(3)], np.eye(4), no_such_option=1)
    with pytest.raises(ValueError):
        binding.Context.track_scans_sdf(None, [np.zeros((3, 2), f32)], np.eye(4))
    with pytest.raises(ValueError):
        eth.track_tsdf(None, [K.cloud(3)], np.eye(4), hashed=False)
    with pytest.raises(ValueError):
        eth.track_tsdf(None, [K.cloud(3)], np.eye(4), dims=(8, 8, 8))
    with pytest.raises(ValueError):
        eth.reconstruct(None, [K.cloud(3)], np.eye(4), tracker="nonsense")
    # stride != 1 is an option the library itself refuses for a cloud, and the options check alone still accepts it for depth frames
    assert lib.icp_sdf_options_check(ctypes.byref(binding.sdf_options(stride=2))) == 0
