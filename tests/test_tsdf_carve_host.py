"""Free-space carving of the cloud fuses on the host side, no device: the numpy restatement of the contract
(tests/tsdf_carve_restatement.py) against one plain loop per ray and sample; with distance 0 against tsdf_cloud_restatement bit for bit;
what carving may never do (drop an observation the band makes, observe a voxel twice); every case of tests/tsdf_carve_cases.py reaching
the edge it is named for; the outcome fixture's conditions; and the structs, the symbols, the Python surface and the refusals that need
no device."""
import ctypes
import inspect
import os
import re
import numpy as np
import pytest

import htsdf_restatement as HR
import tsdf_carve_cases as K
import tsdf_carve_outcome_fixture as OF
import tsdf_carve_restatement as CV
import tsdf_cloud_outcome_fixture as CF
import tsdf_cloud_restatement as CR
from support import same_bits
from tsdf_cloud_cases import cloud, OPTS, TILTED, EYE

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
INF = float("inf")


def loop_walk(vol, pts, pose, origin, distance, min_range, resident=None):
    """The contract, one ray and one sample at a time, with numpy float32 scalars.  resident: the blocks a hashed volume holds after the
    touch (None: dense, `vol.dims` is the box).  -> (n_rays, n_samples, n_outside, n_carved, {voxel: [S, N]}, touched blocks)"""
    P = np.asarray(pose, f32); c = CR.sensor_centre(pose, origin)
    s, tr, mr = vol.s, vol.trunc, f32(min_range)
    J = CV.carve_steps(vol, distance)
    dense = resident is None
    lo = [f32(0)] * 3 if dense else [CR.VOX_LO] * 3
    hi = [f32(d - 1) for d in vol.dims] if dense else [CR.VOX_HI] * 3
    acc, touched = {}, set()
    n_rays = n_samples = n_outside = n_carved = 0
    pending = []                                        # the m < 0 observations of a hashed volume, applied once the touch's set is known
    with np.errstate(all="ignore"):
        for p in np.asarray(pts, f32):
            if not np.isfinite(p).all():
                continue
            d = [f32(f32(f32(P[r, 0] * p[0]) + f32(f32(P[r, 1] * p[1]) + f32(P[r, 2] * p[2]))) + P[r, 3]) - c[r] for r in range(3)]
            rr = np.sqrt(f32(f32(d[0] * d[0]) + f32(f32(d[1] * d[1]) + f32(d[2] * d[2]))))
            if not (np.isfinite(rr) and rr > 0 and rr <= vol.max_d):
                continue
            n_rays += 1
            u = [f32(d[a] / rr) for a in range(3)]
            prev = None
            for m in range(-J, CR.n_steps(vol) + 1):
                t = min(f32(f32(rr - tr) + f32(f32(m) * s)), f32(rr + tr))
                if not (t > 0 if m >= 0 else t > mr):
                    continue
                g = [np.floor(f32(f32(f32(f32(c[a] + f32(t * u[a])) - vol.o[a]) / s) + f32(0.5))) for a in range(3)]
                if not all(lo[a] <= g[a] <= hi[a] for a in range(3)):
                    n_outside += m >= 0
                    continue
                gi = tuple(int(x) for x in g)
                if m >= 0:
                    touched.add(tuple(x >> 3 for x in gi))          # (the touch is the call's own without carving: every in-range m >= 0 sample)
                if gi == prev:
                    continue
                prev = gi
                n_samples += m >= 0
                e = [f32(f32(vol.o[a] + f32(g[a] * s)) - c[a]) for a in range(3)]
                sdf = f32(rr - f32(f32(e[0] * u[0]) + f32(f32(e[1] * u[1]) + f32(e[2] * u[2]))))
                if sdf < -tr:
                    continue
                k = int(np.rint(f32(min(f32(1), f32(sdf / tr)) * f32(32768.0))))
                if m < 0 and not dense:
                    pending.append((gi, k))
                    continue
                n_carved += m < 0
                a_ = acc.setdefault(gi, [0, 0])
                a_[0] += k; a_[1] += 1
    for gi, k in pending:
        if tuple(x >> 3 for x in gi) in (resident | touched):
            n_carved += 1
            a_ = acc.setdefault(gi, [0, 0])
            a_[0] += k; a_[1] += 1
    return n_rays, n_samples, n_outside, n_carved, acc, touched


HOSTILE = cloud(300)
E = np.array([0.05, -0.02, 0.1], f32)
HOSTILE[3] = (np.nan, 0, 1); HOSTILE[5] = (0, np.inf, 1); HOSTILE[7] = E; HOSTILE[9] = (0, 0, 7.5); HOSTILE[11] = (0.05, 0.0, 0.2)


@pytest.mark.parametrize("carve", [dict(distance=INF, min_range=0.0), dict(distance=INF, min_range=0.35), dict(distance=1.0, min_range=0.0)], ids=["all_the_way", "min_range", "one_metre"])
@pytest.mark.parametrize("storage", ["hashed", "dense"])
def test_restatement_against_a_plain_loop(storage, carve):
    """300 points (a NaN, an inf, one at the sensor centre, one beyond max_depth, one nearer than the truncation: no carve sample) from a
    tilted pose and a non-zero sensor origin: counts, the touch's blocks, the accumulators of every voxel and the folded volume."""
    if storage == "hashed":
        vol = HR.HVolume(**OPTS); vol.allocate(K.WALL_BLOCKS)
        resident = set(vol.blocks)
    else:
        vol = CR.DVolume(K.INSIDE[1], **K.INSIDE[0]); resident = None
    n_rays, n_samples, n_outside, n_carved, acc, touched = loop_walk(vol, HOSTILE, TILTED, E, resident=resident, **carve)
    w = CV.walk(vol, HOSTILE, TILTED, E, **carve)
    assert (w["n_points"], w["n_rays"], w["n_samples"], w["n_outside"]) == (300, n_rays, n_samples, n_outside) and n_rays == 296
    assert set(map(tuple, w["touched"].tolist())) == touched
    uv, S, N, carved = CV.accumulate(vol, w)
    assert carved == n_carved > 0
    assert {tuple(v): [int(s), int(n)] for v, s, n in zip(uv.tolist(), S, N)} == acc
    near = CV.walk(vol, HOSTILE[11:12], TILTED, E, **carve)
    assert near["n_rays"] == 1 and (near["m"] >= 0).all()          # r < truncation: no carve sample
    info, st = CV.integrate(vol, HOSTILE, TILTED, E, **carve)
    assert info["n_updated"] == len(acc) and st == dict(n_steps=CV.carve_steps(vol, carve["distance"]), n_carved=n_carved)
    for g, (s, n) in acc.items():
        if storage == "hashed":
            b, l = tuple(x >> 3 for x in g), tuple(x & 7 for x in g)
            D, W = vol.blocks[b][0][l[2], l[1], l[0]], vol.blocks[b][1][l[2], l[1], l[0]]
        else:
            D, W = vol.tsdf[g[2], g[1], g[0]], vol.weight[g[2], g[1], g[0]]
        assert D == f32(s / (n * 32768.0)) and W == 1
    if storage == "hashed":
        assert set(vol.blocks) == resident | touched                # carving allocates nothing


@pytest.mark.parametrize("name", ["n257/hashed", "n257/dense", "target_with_origin/hashed", "box/sensor_outside", "lanes/runs/hashed"])
def test_distance_zero_is_the_plain_integrate(name):
    """With distance 0 the restatement equals tsdf_cloud_restatement.integrate bit for bit, infos included, whatever min_range says."""
    c = K.CASES[name]
    infos, stats, vol = K.replay(c, carve=dict(distance=0.0, min_range=0.7))
    ref = K.new_volume(c)
    assert infos == [CR.integrate(ref, p, T, e) for p, T, e, _ in c["steps"]] and all(st == dict(n_steps=0, n_carved=0) for st in stats)
    if c["dims"] is None:
        a, b = vol.sorted_blocks(), ref.sorted_blocks()
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and vol.n_out_of_range == ref.n_out_of_range
    else:
        assert same_bits(vol.tsdf, ref.tsdf) and same_bits(vol.weight, ref.weight)


def observations(w, keep=None):
    keep = np.ones(len(w["m"]), bool) if keep is None else keep
    return set(zip(w["rays"][keep].tolist(), map(tuple, w["voxels"][keep].tolist()), w["k"][keep].tolist()))


@pytest.mark.parametrize("name", ["n3000/hashed", "n3000/dense", "box/sensor_outside", "residency/straddle", "join/same_voxel"])
def test_carving_drops_no_observation_of_the_band(name):
    """Every (ray, voxel, k) observed with carving off is observed with it on -- the band's first sample may be skipped as a repeat of the
    m = -1 sample, whose observation is then the same k -- and no ray observes a voxel twice."""
    c = K.CASES[name]
    pts, pose, origin, _ = c["steps"][0]
    vol = K.new_volume(c)
    off, on = CV.walk(vol, pts, pose, origin), CV.walk(vol, pts, pose, origin, **c["carve"])
    applied = observations(on, CV.stored(vol, on))
    assert observations(off) <= applied and len(applied) > len(observations(off))
    rv = np.column_stack([on["rays"], on["voxels"]])
    assert len(np.unique(rv, axis=0)) == len(rv)
    assert on["n_samples"] <= off["n_samples"] and on["n_outside"] == off["n_outside"] and np.array_equal(on["touched"], off["touched"])


def test_no_ray_observes_a_voxel_twice_on_the_outcome_scans():
    clouds, poses, _ = OF.scans()
    vol = HR.HVolume(**CF.options())
    for k in (0, 5, 11):
        w = CV.walk(vol, clouds[k], poses[k], None, **OF.CARVE)
        rv = np.column_stack([w["rays"], w["voxels"]])
        assert len(np.unique(rv, axis=0)) == len(rv) and (w["m"] < 0).sum() > (w["m"] >= 0).sum() > 0


@pytest.mark.parametrize("name", list(K.CASES))
def test_every_case_reaches_its_edge(name):
    c = K.CASES[name]
    infos, stats, vol = K.reference(name)
    got = dict(infos[-1], **stats[-1])
    for key, v in c["expect"].items():
        assert got[key] == v, (name, key, got[key], v)
    pts, pose, origin, _ = c["steps"][0]
    w = CV.walk(K.new_volume(c), pts, pose, origin, **c["carve"])
    keep = CV.stored(K.new_volume(c), w)
    carve, band = w["m"] < 0, w["m"] >= 0
    kind = name.split("/")[0]
    if kind in ("n1", "n63", "n64", "n65", "n257", "n3000", "target_with_origin", "hostile_points", "lanes", "box", "exact_ones", "mixed_voxel") and "nearer" not in name:
        assert stats[0]["n_carved"] > 0
    if name in ("n257/hashed", "n3000/hashed"):
        assert (carve & ~keep).any() and (carve & keep).any()          # rays cross resident and missing blocks
    if name == "hostile_points/hashed":
        assert infos[0]["n_points"] == 75 and infos[0]["n_rays"] == 71
    if name == "dyadic/min_range_on_a_sample/hashed":
        vol0 = K.new_volume(c); _, u, r, _ = CR.rays(vol0, pts, pose)
        assert f32((r[0] - vol0.trunc) + f32(-3) * vol0.s) == f32(c["carve"]["min_range"])          # t_m == min_range exactly
    if name == "join/same_voxel":
        assert K.join_voxels(K.JOIN_SAME)[0] == K.join_voxels(K.JOIN_SAME)[1] and -1 in w["m"] and 0 not in w["m"]
        assert infos[0]["n_samples"] == CV.walk(K.new_volume(c), pts, pose)["n_samples"] - 1
    if name == "join/apart":
        assert K.join_voxels(K.JOIN_APART)[0] != K.join_voxels(K.JOIN_APART)[1] and -1 in w["m"] and 0 in w["m"]
    if name == "residency/alternate":
        blocks = (w["voxels"][carve & keep][:, 0] >> 3)
        assert sorted(set(blocks.tolist())) == [0, 2, 4, 5] and sorted(set((w["voxels"][carve & ~keep][:, 0] >> 3).tolist())) == [1, 3]
        assert infos[0]["n_blocks"] == 5
    if name.startswith("residency/across_zero"):
        n = int(name[-1])
        b = w["voxels"][carve & keep] >> 3
        for a in range(3):
            assert set(b[:, a].tolist()) == ({-1, 0} if a < n else {0}), (name, a)
    if name == "residency/beyond_the_range":
        assert len(w["m"]) == 0 and infos[0]["n_outside"] == 800 and sorted(vol.blocks) == sorted(map(tuple, K.WALL_BLOCKS.tolist()))
    if name == "residency/straddle":
        assert infos[0]["n_outside"] > 0 and infos[0]["n_samples"] > 0 and (carve & keep).any() and (carve & ~keep).any()
    if name == "box/sensor_outside":
        first = {}
        for ray, m in zip(w["rays"].tolist(), w["m"].tolist()):
            first.setdefault(ray, m)
        starts = np.array(list(first.values()))
        t0 = CV.walk(K.new_volume(c), pts, pose, origin)                 # (every ray has carve samples in front of the box that are not in it)
        assert (starts < 0).mean() > 0.5 and (starts > -CV.carve_steps(vol, INF)).all() and t0["n_outside"] > 0
    if name == "box/corner":
        assert (w["voxels"][-1] == np.array(K.CC.FACE_DIMS) - 1).all() and infos[0]["n_outside"] > 0 and stats[0]["n_carved"] > 0
    if name == "exact_ones":
        row = vol.tsdf[12, 2, 2:22], vol.weight[12, 2, 2:22]
        assert (row[0][1:13] == f32(1.0)).all() and (row[1][1:13] == 1).all() and row[1][0] == 0
    if name == "mixed_voxel":
        uv, S, N, _ = CV.accumulate(K.new_volume(c), w)
        sn = {int(v[0]) - 2: (int(s), int(n)) for v, s, n in zip(uv, S, N)}
        assert sn[1] == (65536, 2) and sn[5] == (65536, 2) and sn[8] == (32768, 2) and sn[11] == (0, 2) and sn[12] == (32768, 1) and sn[19] == (-32768, 1)
    if name.startswith("lanes/pile"):
        assert c["copies"] == (1 << 17) + 1 and infos[0]["n_rays"] == c["copies"] and stats[0]["n_carved"] == c["copies"] * int(carve[keep].sum())
        assert (w["k"][carve & keep] == 32768).all()                    # fbar == 1 in every carved voxel


def test_a_thousand_copies_fold_like_one():
    """The argument tsdf_carve_cases.replay uses for `copies`, literally: a thousand copies of a point give the folded volume of one copy
    bit for bit, and a thousand times its per-ray counts."""
    for name in ("lanes/pile/hashed", "lanes/pile/dense"):
        c = K.CASES[name]
        infos, stats, vol = K.reference(name)
        many = K.new_volume(c)
        info, st = CV.integrate(many, np.repeat(c["steps"][0][0], 1000, 0), c["steps"][0][1], None, **c["carve"])
        assert st["n_carved"] * c["copies"] == stats[0]["n_carved"] * 1000 and info["n_samples"] * c["copies"] == infos[0]["n_samples"] * 1000
        assert info["n_updated"] == infos[0]["n_updated"]
        if c["dims"] is None:
            a, b = vol.sorted_blocks(), many.sorted_blocks()
            assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
        else:
            assert same_bits(vol.tsdf, many.tsdf) and same_bits(vol.weight, many.weight)


def test_track_restatement():
    """The loop's restatement: with distance 0 it is sdf_cloud_restatement.track, poses, records, infos and volume; with carving on every
    fuse carves and the model differs."""
    import sdf_cloud_cases as SK
    import sdf_cloud_restatement as SC
    scans = SK.track_scans()
    va, vb, vc = (SC.Volume(SK.DIMS, **SK.OPTS) for _ in range(3))
    pa = SC.track(va, scans, SK.TRACK_POSES[0], n_iterations=5)
    pb = CV.track(vb, scans, SK.TRACK_POSES[0], n_iterations=5)
    assert all(same_bits(x, y) for x, y in zip(pa[0], pb[0])) and pa[2] == pb[2] and pa[3] == pb[3] == 0 and all(st == dict(n_steps=0, n_carved=0) for st in pb[4])
    assert same_bits(va.tsdf, vb.tsdf) and same_bits(va.weight, vb.weight)
    pc = CV.track(vc, scans, SK.TRACK_POSES[0], distance=1.5, min_range=0.3, n_iterations=5)
    assert pc[3] == 0 and all(st["n_steps"] == 15 and st["n_carved"] > 0 for st in pc[4]) and (vc.weight > 0).sum() > (va.weight > 0).sum()


def test_outcome_fixture_conditions():
    """The box that stood in four scans: in the model without carving, gone with it, the room untouched, no block added (recorded:
    476 of 752 valid inside probes negative without; none of 1377, and no face probe below 0.09, with; 483 blocks either way; the
    held-out scan 98.4 % valid at a median of 2.4 mm, against 97.8 % and 2.3 mm without)."""
    fo, fn, share, median = OF.assert_outcome()
    assert fn["inside_valid"] > fo["inside_valid"] and share > 0.9


def test_structs_symbols_python_surface_and_refusals_without_a_device():
    from icp_amd import binding, eth
    assert ctypes.sizeof(binding.IcpTsdfCarveOptions) == 8 and [f[0] for f in binding.IcpTsdfCarveOptions._fields_] == ["distance", "min_range"]
    assert ctypes.sizeof(binding.IcpTsdfCarveInfo) == 24 and binding.IcpTsdfCarveInfo.n_carved.offset == 8 and binding.IcpTsdfCarveInfo.n_carved_total.offset == 16
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    names = ("icp_tsdf_carve_options_default", "icp_tsdf_carve_options_check", "icp_set_tsdf_carve_options", "icp_get_tsdf_carve_options", "icp_tsdf_carve_stats")
    for n in names:
        assert n in binding.EXPORTS and hasattr(lib, n) and re.search(r"^int %s\(" % n, hdr, flags=re.M), n
    assert hasattr(lib, "icp_debug_tsdf_carve_time") and "icp_debug_tsdf_carve_time" not in hdr
    assert 'static_assert(sizeof(icp_tsdf_carve_info) == 24' in hdr and re.search(r"^\} icp_tsdf_carve_options;", hdr, flags=re.M)
    o = binding.IcpTsdfCarveOptions(3.0, 3.0)
    assert lib.icp_tsdf_carve_options_default(ctypes.byref(o)) == 0 and (o.distance, o.min_range) == (0.0, 0.0)
    assert lib.icp_tsdf_carve_options_default(None) == 1 and lib.icp_tsdf_carve_options_check(None) == 1
    check = lambda d, m: lib.icp_tsdf_carve_options_check(ctypes.byref(binding.IcpTsdfCarveOptions(d, m)))
    assert check(0.0, 0.0) == 0 and check(2.5, 0.3) == 0 and check(INF, 0.0) == 0 and check(0.0, 5.0) == 0
    assert check(-1.0, 0.0) == 1 and check(np.nan, 0.0) == 1 and check(-INF, 0.0) == 1
    assert check(1.0, -0.1) == 1 and check(1.0, INF) == 1 and check(1.0, np.nan) == 1
    assert lib.icp_set_tsdf_carve_options(None, ctypes.byref(o)) == 1 and lib.icp_get_tsdf_carve_options(None, ctypes.byref(o)) == 1
    assert lib.icp_tsdf_carve_stats(None, ctypes.byref(binding.IcpTsdfCarveInfo())) == 1
    # J beyond the cap, as the restatement refuses it (the library's refusal needs a volume: tests/test_gpu_tsdf_carve.py)
    far = HR.HVolume(**dict(OPTS, voxel_size=0.001, truncation=0.004, max_depth=65.537))
    with pytest.raises(ValueError):
        CV.carve_steps(far, INF)
    assert CV.carve_steps(far, 65.5) <= CV.MAX_STEPS and CV.carve_steps(far, 0.0) == 0 and CV.carve_steps(HR.HVolume(**OPTS), INF) == 60
    par = inspect.signature(binding.Context.set_tsdf_carve).parameters
    assert list(par) == ["self", "distance", "min_range"] and par["distance"].default == 0.0 and par["min_range"].default == 0.0
    assert hasattr(binding.Context, "tsdf_carve_options") and hasattr(binding.Context, "tsdf_carve_stats")
    # the runners take carve= as a keyword: set for the call, the previous setting put back, also behind an error; None touches nothing
    class Fake:
        def __init__(self):
            self.now, self.log = binding.IcpTsdfCarveOptions(0.75, 0.25), []

        def tsdf_carve_options(self):
            return self.now

        def set_tsdf_carve(self, distance=0.0, min_range=0.0):
            self.now = binding.IcpTsdfCarveOptions(distance, min_range); self.log.append((distance, min_range))

    for fn, args in ((eth.fuse_scans, ([cloud(3)], [])), (eth.track_tsdf, ([cloud(3)], np.eye(4))), (eth.reconstruct, ([cloud(3)], np.eye(4)))):
        assert fn.__kwdefaults__ == {"carve": None}
        kw = dict(hashed=False) if fn is not eth.reconstruct else dict(tracker="neither")          # refused by the runner itself: ValueError
        fake = Fake()
        with pytest.raises(ValueError):
            fn(fake, *args, carve=dict(distance=2.0, min_range=0.5), **kw)
        assert fake.log == [(2.0, 0.5), (0.75, 0.25)]
        with pytest.raises(ValueError):
            fn(fake, *args, carve=None, **kw)
        assert len(fake.log) == 2
