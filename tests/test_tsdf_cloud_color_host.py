"""The coloured laser-scan fuse on the host side, no device: the numpy restatement of the contract
(tests/tsdf_cloud_color_restatement.py) against one plain loop per ray and sample; what follows from the contract (the colours do not
depend on the carve options nor on the order of the points, coloured voxels are updated voxels, one ray from Wc = 0 leaves the point's
bytes); every case of tests/tsdf_cloud_color_cases.py reaching what it is named for; the limit's arithmetic; the outcome fixture's
conditions; and the symbols, the Python surface and the refusals that need no device."""
import ctypes
import inspect
import os
import re
import numpy as np
import pytest

import htsdf_color_restatement as HC
import htsdf_restatement as HR
import tsdf_carve_restatement as CV
import tsdf_cloud_cases as CC
import tsdf_cloud_color_cases as K
import tsdf_cloud_color_outcome_fixture as OF
import tsdf_cloud_color_restatement as KR
import tsdf_cloud_restatement as CR
from support import same_bits
from tsdf_cloud_cases import cloud, OPTS, TILTED, EYE

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def geometry_of(vol):
    return (vol.tsdf, vol.weight) if isinstance(vol, CR.DVolume) else vol.sorted_blocks()


def same_arrays(a, b):
    return len(a) == len(b) and all(same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a, b))


def voxels_with(vol, colour):
    out = set()
    if isinstance(vol, CR.DVolume):
        w = vol.wc if colour else vol.weight
        return set(map(tuple, np.argwhere(w > 0)[:, ::-1].tolist()))
    for b, blk in (vol.colors if colour else vol.blocks).items():
        for z, y, x in np.argwhere(blk[1] > 0):
            out.add((b[0] * 8 + int(x), b[1] * 8 + int(y), b[2] * 8 + int(z)))
    return out


def loop_colours(vol, pts, rgba, pose, origin):
    """The contract's colour walk, one ray and one sample at a time, with numpy float32 scalars: {voxel: [SR, SG, SB, NC]}."""
    P = np.asarray(pose, f32); c = CR.sensor_centre(pose, origin)
    s, tr = vol.s, vol.trunc
    dense = isinstance(vol, CR.DVolume)
    lo = [f32(0)] * 3 if dense else [CR.VOX_LO] * 3
    hi = [f32(d - 1) for d in vol.dims] if dense else [CR.VOX_HI] * 3
    acc = {}
    with np.errstate(all="ignore"):
        for p, col in zip(np.asarray(pts, f32), np.asarray(rgba, np.uint8)):
            if not np.isfinite(p).all():
                continue
            d = [f32(f32(f32(P[r, 0] * p[0]) + f32(f32(P[r, 1] * p[1]) + f32(P[r, 2] * p[2]))) + P[r, 3]) - c[r] for r in range(3)]
            rr = np.sqrt(f32(f32(d[0] * d[0]) + f32(f32(d[1] * d[1]) + f32(d[2] * d[2]))))
            if not (np.isfinite(rr) and rr > 0 and rr <= vol.max_d):
                continue
            u = [f32(d[a] / rr) for a in range(3)]
            prev = None
            for m in range(CR.n_steps(vol) + 1):
                t = min(f32(f32(rr - tr) + f32(f32(m) * s)), f32(rr + tr))
                if not t > 0:
                    continue
                g = [np.floor(f32(f32(f32(f32(c[a] + f32(t * u[a])) - vol.o[a]) / s) + f32(0.5))) for a in range(3)]
                if not all(lo[a] <= g[a] <= hi[a] for a in range(3)):
                    continue
                v = tuple(int(x) for x in g)
                if v == prev:
                    continue
                prev = v
                e = [f32(f32(vol.o[a] + f32(g[a] * s)) - c[a]) for a in range(3)]
                sdf = f32(rr - f32(f32(e[0] * u[0]) + f32(f32(e[1] * u[1]) + f32(e[2] * u[2]))))
                if sdf < -tr or sdf > tr:
                    continue
                a4 = acc.setdefault(v, [0, 0, 0, 0])
                for ch in range(3):
                    a4[ch] += int(col[ch])
                a4[3] += 1
    return acc


@pytest.mark.parametrize("name", ["n255/hashed", "n255/dense", "hostile_points/hashed", "leaving_the_box/dense", "oblique/dense", "beyond_truncation/hashed"])
def test_restatement_equals_the_plain_loop(name):
    c = K.CASES[name]
    _, pts, rgba, pose, origin = c["steps"][0]
    vol = K.new_volume(c)
    want = loop_colours(vol, pts, rgba, pose, origin)
    uv, S, N = KR.accumulate(*KR.color_walk(vol, pts, rgba, pose, origin))
    got = {tuple(int(x) for x in v): [int(s[0]), int(s[1]), int(s[2]), int(n)] for v, s, n in zip(uv, S, N)}
    assert got == want and len(got) > 0
    (info, _, nc), = K.reference(name)[0]
    assert nc == len(want) <= info["n_updated"]


def test_fold_is_the_contracts_arithmetic():
    """cbar in double from the integers, one fp32 rounding; the running mean and the clamp in fp32."""
    C = np.array([[10.5, 0.0, 255.0]], f32); Wc = np.array([2.0], f32)
    S = np.array([[1, 2, 764]], np.int64); N = np.array([3], np.int64)
    newC, newW = KR.fold_values(C, Wc, S, N, f32(2.5))
    cbar = [f32(1.0 / 3.0), f32(2.0 / 3.0), f32(764.0 / 3.0)]
    want = [f32(f32(f32(f32(2.0) * C[0, k]) + cbar[k]) / f32(3.0)) for k in range(3)]
    assert same_bits(newC[0], np.array(want, f32)) and newW[0] == f32(2.5)


def test_every_case_reaches_what_it_is_named_for():
    seen = {}
    for name, c in K.CASES.items():
        out, vol = K.reference(name)
        col, upd = voxels_with(vol, True), voxels_with(vol, False)
        assert col <= upd and len(col) > 0, name                                   # (3): coloured voxels are updated voxels
        assert all(o[2] <= o[0]["n_updated"] for o in out), name
        seen[name] = (out, vol, col, upd)
    for kind in ("hashed", "dense"):
        row = lambda v: (v, 0, 0) if kind == "hashed" else (2 + v, 2, 12)
        colour = lambda vol, v: color_at(vol, row(v))
        out, vol, col, upd = seen["one_point/" + kind]
        assert col == upd == {row(v) for v in range(5, 12)} and out[0][2] == 7
        for v in range(5, 12):                                                     # (4): the point's bytes exactly, Wc == 1
            assert colour(vol, v) == (200.0, 17.0, 5.0, 1.0)
        out, vol, col, upd = seen["two_rays_0_and_255/" + kind]
        assert all(colour(vol, v) == (127.5, 127.5, 127.5, 1.0) for v in range(5, 12))
        out, vol, col, upd = seen["three_rays_thirds/" + kind]
        third = (float(f32(1.0 / 3.0)), float(f32(2.0 / 3.0)), float(f32(764.0 / 3.0)), 1.0)
        assert all(colour(vol, v) == third for v in range(5, 12)) and third[0] != 1.0 / 3.0
        out, vol, col, upd = seen["beyond_truncation/" + kind]
        assert upd - col == {row(5)} and out[0][0]["n_updated"] == 7 and out[0][2] == 6          # at least one updated voxel is not coloured
        out, vol, col, upd = seen["behind_truncation/" + kind]
        assert row(11) not in upd and col == upd == {row(v) for v in range(5, 11)}
        # the oblique ray: fewer counted samples than samples in range
        c = K.CASES["oblique/" + kind]
        valid, g = CC.sample_voxels(c["opts"], c["steps"][0][1], EYE)
        assert valid.all() and out is not None
        info = seen["oblique/" + kind][0][0][0]
        assert info["n_samples"] + info["n_outside"] < valid.sum() and info["n_samples"] >= 3
        # sizes, hostile points, weights
        for n in K.SIZES:
            assert seen["n%d/%s" % (n, kind)][0][0][0]["n_points"] == n
        hinfo = seen["hostile_points/" + kind][0][0][0]
        assert hinfo["n_points"] - hinfo["n_rays"] == 6
        wmax = lambda vol: max(color_at(vol, v)[3] for v in voxels_with(vol, True))
        assert wmax(seen["twice/" + kind][1]) == 2.0 and wmax(seen["thrice_clamped/" + kind][1]) == 2.0
        assert seen["thrice_clamped/" + kind][0][2][2] == seen["twice/" + kind][0][1][2] > 0
    # alpha and order: the same colours as the twin (2)
    for a, b in K.SAME_COLOURS:
        assert same_arrays(KR.colors_of(seen[a][1]), KR.colors_of(seen[b][1])) and same_arrays(geometry_of(seen[a][1]), geometry_of(seen[b][1])), (a, b)
    a = K.CASES["alpha_varies/dense"]["steps"][0][2]; b = K.CASES["n257/dense"]["steps"][0][2]
    assert np.array_equal(a[:, :3], b[:, :3]) and (a[:, 3] != b[:, 3]).sum() > 200
    # storage
    assert seen["leaving_the_box/dense"][0][0][0]["n_outside"] > 0
    assert all(min(b) < 0 for b in seen["negative_blocks/hashed"][1].colors) and len(seen["negative_blocks/hashed"][1].colors) > 4
    for cap in (1, 2):
        assert len(seen["grows_inside/capacity_%d" % cap][1].blocks) >= 24 > K.CASES["grows_inside/capacity_%d" % cap]["capacity"]
    out = seen["accumulators_remade/hashed"][0]
    assert out[0][0]["n_blocks"] <= 4 < out[1][0]["n_blocks"]
    out, vol = seen["evict_between/hashed"][:2]
    assert out[1][0]["n_blocks"] < 2 * out[0][0]["n_blocks"] and set(vol.colors) <= set(vol.blocks)


def color_at(vol, v):
    if isinstance(vol, CR.DVolume):
        return tuple(float(x) for x in vol.rgb[v[2], v[1], v[0]]) + (float(vol.wc[v[2], v[1], v[0]]),)
    rgb, wc = vol.colors[tuple(x >> 3 for x in v)]
    l = tuple(x & 7 for x in v)
    return tuple(float(x) for x in rgb[l[2], l[1], l[0]]) + (float(wc[l[2], l[1], l[0]]),)


@pytest.mark.parametrize("name", K.CARVED)
def test_colours_do_not_depend_on_the_carve_options(name):
    """(1): under either carve setting the colours equal the uncarved coloured fuse, and the geometry equals the uncoloured carved fuse."""
    c = K.CASES[name]
    base_out, base = K.reference(name)
    for carve in K.CARVES:
        geo = []
        out, vol = K.replay(c, carve, after=lambda k, v, twin: geo.append(same_arrays(geometry_of(v), geometry_of(twin))))
        assert all(geo) and same_arrays(KR.colors_of(vol), KR.colors_of(base)), (name, carve)
        assert [o[2] for o in out] == [o[2] for o in base_out]
    assert any(o[1]["n_carved"] > 0 for o in out) or name.startswith("leaving")


def test_the_limit():
    """2^24 points of byte 255 in one voxel stay below 2^32 in a 32-bit sum; one more point is refused before anything is walked."""
    assert KR.MAX_POINTS == 1 << 24 and 255 * KR.MAX_POINTS < 1 << 32 and 256 * KR.MAX_POINTS == 1 << 32
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    assert "enum { ICP_TSDF_CLOUD_COLOR_MAX_POINTS = 1 << 24 };" in hdr
    many = np.broadcast_to(np.zeros((1, 3), f32), (KR.MAX_POINTS + 1, 3))
    with pytest.raises(ValueError):
        KR.integrate(KR.add_color(HR.HVolume(**OPTS)), many, None, EYE)
    # the packed 64-bit form: SR | SG << 32 at its largest leaves SG's field intact
    lo = 255 * KR.MAX_POINTS
    assert ((lo | (lo << 32)) >> 32) == lo and ((lo | (lo << 32)) & 0xFFFFFFFF) == lo


def test_outcome_fixture_colours():
    """The twelve coloured scans fused by the restatement (recorded: 99.6 % coloured, median error 15.1 against 34.0 for the mean colour)."""
    vol, out = OF.model()
    share, median, baseline = OF.assert_colours(vol)
    assert all(o[2] < o[0]["n_updated"] for o in out) and set(vol.colors) <= set(vol.blocks)


def test_symbols_python_surface_and_refusals_without_a_device():
    from icp_amd import binding, eth
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for sym in ("icp_tsdf_integrate_cloud_color", "icp_track_scans_sdf_color"):
        assert sym in binding.EXPORTS and hasattr(lib, sym) and re.search(r"^int %s\(icp_ctx\* ctx, " % sym, hdr, flags=re.M), sym
    assert hasattr(lib, "icp_debug_tsdf_cloud_color_time") and "icp_debug_tsdf_cloud_color_time" not in hdr
    p = binding.pose_to_c(np.eye(4)); info = binding.IcpTsdfCloudInfo(); nc = ctypes.c_int32(5)
    assert lib.icp_tsdf_integrate_cloud_color(None, 1, binding._ptr(p), None, ctypes.byref(info), ctypes.byref(nc)) == 1
    assert lib.icp_track_scans_sdf_color(None, None, None, None, 1, ctypes.byref(binding.sdf_options()), binding._ptr(p), None, None, None) == 1
    assert lib.icp_debug_tsdf_cloud_color_time(None, 1, binding._ptr(p), None, None) == 1
    # the keywords ride on the methods and runners whose signatures other tests pin
    assert list(inspect.signature(binding.Context.tsdf_integrate_cloud).parameters) == ["self", "which", "pose", "sensor_origin"]
    assert list(inspect.signature(binding.Context.track_scans_sdf).parameters) == ["self", "scans", "pose", "options"]
    for fn in (eth.fuse_scans, eth.track_tsdf, eth.reconstruct):
        assert fn.__kwdefaults__ == {"carve": None} and fn.__wrapped__.__kwdefaults__ == {"colors": None}
    with pytest.raises(ValueError):
        binding.Context.tsdf_integrate_cloud(None, "source", pose=np.eye(3), color=True)
    with pytest.raises(ValueError):
        binding.Context.track_scans_sdf(None, [cloud(3)], np.eye(4), colors=[])
    with pytest.raises(ValueError):
        binding.Context.track_scans_sdf(None, [cloud(3)], np.eye(4), colors=[np.zeros((3, 3), np.uint8)])
    with pytest.raises(ValueError):
        eth.fuse_scans(None, [cloud(3)], [np.eye(4)], colors=[])
    with pytest.raises(ValueError):
        eth.track_tsdf(None, [cloud(3)], np.eye(4), colors=[K.colours(3, 1)], hashed=False)
    with pytest.raises(ValueError):
        eth.reconstruct(None, [cloud(3)], np.eye(4), colors=[K.colours(3, 1)], tracker="neither")

    # the runners with colours: a coloured volume, every scan set with its colours, the coloured fuse; without: as before
    class Fake:
        def __init__(self):
            self.log = []

        def tsdf_create_hashed(self, **kw):
            self.log.append(("create", kw.get("color", False)))

        def set_source(self, xyz, normals=None, rgba=None):
            self.log.append(("source", rgba is not None))

        def tsdf_integrate_cloud(self, which, pose=None, color=False):
            self.log.append(("fuse", color)); return {}

        def track_scans_sdf(self, scans, pose, colors=None, **kw):
            self.log.append(("track", colors is not None)); return ([], [], [], 0) + (() if colors is None else ([],))

        def tsdf_carve_options(self):
            return binding.IcpTsdfCarveOptions(0.0, 0.0)

        def set_tsdf_carve(self, distance=0.0, min_range=0.0):
            self.log.append(("carve", distance))

    f = Fake()
    eth.fuse_scans(f, [cloud(3)], [np.eye(4)], colors=[K.colours(3, 1)], carve=dict(distance=1.0))
    assert f.log == [("carve", 1.0), ("create", True), ("source", True), ("fuse", True), ("carve", 0.0)]
    f = Fake()
    eth.fuse_scans(f, [cloud(3)], [np.eye(4)])
    assert f.log == [("create", False), ("source", False), ("fuse", False)]
    f = Fake()
    assert len(eth.track_tsdf(f, [cloud(3)], np.eye(4), colors=[K.colours(3, 1)])) == 5 and f.log == [("create", True), ("track", True)]
    f = Fake()
    assert len(eth.track_tsdf(f, [cloud(3)], np.eye(4))) == 4 and f.log == [("create", False), ("track", False)]
