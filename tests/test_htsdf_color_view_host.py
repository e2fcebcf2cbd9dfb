"""The coloured views of the hashed TSDF volume on the host side: the numpy restatement of the four contracts
(tests/htsdf_color_view_restatement.py) against the dense coloured restatement -- the ray-cast bit for bit on the volume densified from
voxel (0, 0, 0), the mesh colours as a set of triangles on the blocks' bounding box --, the classes of hits and vertices the cases must
contain, the symbols, the header, the Python surface and the argument checks of the wrappers and of tum."""
import ctypes
import inspect
import json
import os
import re
import numpy as np
import pytest

import htsdf_color_view_cases as VC
import htsdf_color_view_outcome_fixture as VOF
import htsdf_color_view_restatement as VR
import htsdf_raycast_cases as RC
import htsdf_raycast_restatement as RR
import tsdf_color_restatement as TC
import tsdf_mesh_restatement as TM
import tsdf_restatement as TS
from support import same_bits

f32 = np.float32
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("icp_tsdf_raycast_color_hashed", "icp_set_target_tsdf_color_hashed", "icp_track_depth_model_color_hashed", "icp_tsdf_mesh_color_hashed")


def dense_volume(d_opts, T, W, RGB, WC, cls=TS.Volume):
    keep = ("dims", "origin", "voxel_size", "truncation", "max_weight", "min_depth", "max_depth", "ray_step")
    vol = cls(**{k: v for k, v in d_opts.items() if k in keep})
    vol.tsdf, vol.weight, vol.rgb, vol.wc = T, W, RGB, WC
    return vol


@pytest.mark.parametrize("ci", range(len(VC.dense_equality_cases())), ids=[c[0] for c in VC.dense_equality_cases()])
def test_restated_cast_equals_the_dense_restatement(ci):
    """P, and A - D and G moved to non-negative block coordinates: the four arrays, both counts and the colour path of the restated coloured
    hashed ray-cast against tsdf_color_restatement.raycast_color on the dense coloured volume built from voxel (0, 0, 0) with the same
    origin, bit for bit, at every camera size and every pose."""
    case = VC.dense_equality_cases()[ci]
    dv = dense_volume(*VC.dense_lo0(case))
    total = 0
    for si, (cw, ch) in enumerate(VC.SIZES):
        for pi, P in enumerate(case[7]):
            got = VC.restated(ci, si, pi, "dense")
            want = TC.raycast_color(dv, RC.camera(cw, ch)[1], P)
            assert got[4:6] == want[4:6], (case[0], cw, ch, pi)
            for a, b in zip(got[:3], want[:3]):
                assert same_bits(a, b), (case[0], cw, ch, pi)
            assert np.array_equal(got[3], want[3]) and np.array_equal(got[6], want[6]), (case[0], cw, ch, pi)
            total += got[5]
    print("%s: %d coloured hits over %d casts" % (case[0], total, len(VC.SIZES) * len(case[7])))
    assert total > 100


DYADIC = ("NEG", "A", "B", "C without (0, 0, 0)", "D", "G")      # o + (float)lo s is exact: the dense box holds the same positions


@pytest.mark.parametrize("name", DYADIC)
def test_restated_mesh_colours_equal_the_dense_restatement_as_a_set_of_triangles(name):
    """Positions, normals and colours of every triangle corner: the restated coloured hashed mesh against tsdf_mesh_restatement.mesh and
    tsdf_color_restatement.mesh_colors on the dense coloured volume over the blocks' bounding box."""
    ci = [c[0] for c in VC.all_cases()].index(name)
    case = VC.all_cases()[ci]
    d_opts, T, W, RGB, WC = VC.dense_of(case)
    dv = TM.Volume(d_opts["dims"], d_opts["origin"], voxel_size=d_opts["voxel_size"])
    dv.tsdf, dv.weight, dv.rgb, dv.wc = T, W, RGB, WC
    for mw in VC.MIN_WEIGHTS:
        v, n, t, col, _ = VC.restated_mesh(ci, mw)
        dvv, dn, dt = TM.mesh(dv, mw)
        dcol = TC.mesh_colors(dv, mw)
        print("%s at min_weight %g: V %d, T %d" % (name, mw, len(v), len(t)))
        assert (len(v), len(t)) == (len(dvv), len(dt)) and len(col) == len(v) and len(dcol) == len(dvv)
        assert np.array_equal(VR.colored_triangle_rows(v, n, col, t), VR.colored_triangle_rows(dvv, dn, dcol, dt))
    assert len(VC.restated_mesh(ci, 0.0)[2]) > 100


def test_vertex_edges_follow_the_mesh_restatement_order():
    """vertex_edges restates which edges carry a vertex and in which order; the positions computed from its (owner, code) pairs equal
    htsdf_mesh_restatement.mesh's vertices bit for bit, row for row."""
    for name in ("P", "D", "G"):
        ci = [c[0] for c in VC.all_cases()].index(name)
        vol = VC.blocks_of(VC.all_cases()[ci])
        v = VC.restated_mesh(ci, 0.0)[0]
        g, code = VR.vertex_edges(VR.block_coords(vol), vol.F, vol.W, 0.0)
        assert len(g) == len(v) > 100
        d = np.stack([code & 1, (code >> 1) & 1, code >> 2], 1)
        e = g + d
        with np.errstate(all="ignore"):
            Fv = vol.voxel(g[:, 0], g[:, 1], g[:, 2])[0]; Fd = vol.voxel(e[:, 0], e[:, 1], e[:, 2])[0]
            ts = (Fv / (Fv - Fd)) * vol.s
            pos = np.stack([np.where(d[:, r] == 1, (vol.o[r] + g[:, r].astype(f32) * vol.s) + ts, vol.o[r] + g[:, r].astype(f32) * vol.s) for r in range(3)], 1).astype(f32)
        assert same_bits(pos, v), name


def test_the_cases_contain_every_class():
    """So that no test passes vacuously: hits coloured by the eight-corner lerp, by the nearest corner and left uncoloured; coloured hits
    whose cell spans 2, 4 and 8 blocks; a hit whose cell touches B's block with all Wc = 0; channel values clamped at both ends; mesh
    vertices with both ends coloured, one end and neither, and vertices whose far end lies in a neighbouring block."""
    cs = VC.all_cases()
    paths = {TC.PATH_NONE: 0, TC.PATH_NEAREST: 0, TC.PATH_EIGHT: 0}
    spans = {1: 0, 2: 0, 4: 0, 8: 0}
    zero_block_hits = 0
    lo = hi = 0
    for ci, case in enumerate(cs):
        vol = VC.blocks_of(case)
        zb = None
        if case[0] == "B":
            k = ((VC.ZERO_BLOCK[2] + RR.RANGE) << 42) | ((VC.ZERO_BLOCK[1] + RR.RANGE) << 21) | (VC.ZERO_BLOCK[0] + RR.RANGE)
            zb = int(np.searchsorted(vol.key, k))
            assert vol.key[zb] == k and (vol.Wc[zb] == 0).all() and (vol.W[zb] > 0).all()
        for si in range(len(VC.SIZES)):
            for pi in range(len(case[7])):
                r = VC.restated(ci, si, pi)
                path, tr = r[6], r[7]
                for p in paths:
                    paths[p] += int((path == p).sum())
                col = path >= TC.PATH_NEAREST
                for s in spans:
                    spans[s] += int(((tr["span"] == s) & col).sum())
                if zb is not None:
                    zero_block_hits += int((tr["blocks"] == zb).any(1).sum())
                lo += int((r[3][col, :3] == 0).sum()); hi += int((r[3][col, :3] == 255).sum())
                assert r[5] == int(col.sum()) and ((r[3] == 0).all(1) == ~col).all() and (r[3][col, 3] == 255).all()
    print("paths (none, nearest, eight):", paths, "spans of coloured hits:", spans, "hits on the uncoloured block:", zero_block_hits, "clamped bytes:", lo, hi)
    assert all(v > 50 for v in paths.values()) and all(v > 10 for v in spans.values()) and zero_block_hits > 50 and lo > 50 and hi > 50
    total = dict(both=0, one=0, neither=0, far_end_in_another_block=0)
    for ci, case in enumerate(cs):
        if case[0] in VC.MESH_CASES:
            st = VC.restated_mesh(ci, 0.0)[4]
            for k in total:
                total[k] += st[k]
    print("mesh vertices:", total)
    assert all(v > 100 for v in total.values())


def test_symbols_header_and_python_surface():
    from icp_amd import binding
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for sym in NEW:
        assert sym in binding.EXPORTS and hasattr(lib, sym) and re.search(r"^int %s\(icp_ctx\* ctx" % sym, hdr, flags=re.M), sym
    assert "_hashed_color" not in hdr and not hasattr(lib, "icp_tsdf_raycast_hashed_color")
    for dbg in ("icp_debug_htsdf_raycast_color_time", "icp_debug_htsdf_mesh_color_time"):
        assert hasattr(lib, dbg) and dbg not in hdr
    assert "no coloured ray-cast" not in hdr and "There is no coloured" not in hdr and "there is no *_color form" not in hdr
    n = ctypes.c_int32(7)
    assert lib.icp_tsdf_raycast_color_hashed(None, None, None, None, None, None, None, ctypes.byref(n), None) == 1      # a null context
    assert lib.icp_set_target_tsdf_color_hashed(None, None, None, ctypes.byref(n)) == 1
    assert lib.icp_track_depth_model_color_hashed(None, None, None, 0, None, None, None, None, None) == 1
    assert lib.icp_tsdf_mesh_color_hashed(None, ctypes.c_float(0), 0, 0, None, None, None, None, None, None) == 1
    C = binding.Context
    assert hasattr(C, "tsdf_raycast_color_hashed")
    assert list(inspect.signature(C.set_target_tsdf_hashed).parameters) == ["self", "cam", "pose", "check", "color"]
    assert inspect.signature(C.set_target_tsdf_hashed).parameters["color"].default is False
    assert inspect.signature(C.track_depth_model_hashed).parameters["rgbx_frames"].default is None
    par = inspect.signature(C.tsdf_mesh_hashed).parameters
    assert list(par) == ["self", "min_weight", "normals", "colors"] and par["colors"].default is False and par["normals"].default is True
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "icp_tsdf_raycast_color_hashed" in readme and "6zc" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_wrapper_and_tum_argument_checks():
    """The ValueErrors, raised before the context is touched (the context is None)."""
    from icp_amd import binding, tum
    cam = binding.depth_camera(np.eye(3), 4, 4)
    for bad in (np.eye(3), np.zeros(16), None):
        with pytest.raises(ValueError):
            binding.Context.tsdf_raycast_color_hashed(None, cam, bad)
        with pytest.raises(ValueError):
            binding.Context.set_target_tsdf_hashed(None, cam, bad, color=True)
    so = binding.depth_options(False, 2, fix_color_index=True)
    with pytest.raises(ValueError, match="4 bytes per pixel"):
        binding.Context.track_depth_model_hashed(None, np.zeros((3, 4, 4), f32), cam, so, rgbx_frames=np.zeros((3, 15, 4), np.uint8))
    with pytest.raises(ValueError, match="camera"):
        binding.Context.track_depth_model_hashed(None, np.zeros((3, 5, 4), f32), cam, so, rgbx_frames=np.zeros((3, 16, 4), np.uint8))
    with pytest.raises(ValueError, match="min_weight"):
        binding.Context.tsdf_mesh_hashed(None, min_weight=-1.0, colors=True)
    seq = dict(K=np.eye(3, dtype=f32), width=4, height=4, depth=np.zeros((1, 4, 4), f32), rgbx=np.zeros((1, 16, 4), np.uint8), gt=None, frames=[0])
    model = dict(hashed=True, origin=(0, 0, 0), voxel_size=0.1)
    with pytest.raises(ValueError, match="reads no colours") as e:
        tum.track(None, seq, model=dict(model, color=True, raycast=True))
    assert 'raycast="color"' in str(e.value)
    bad_models = [(dict(model, raycast="color"), None),                                     # without color=True
                  (dict(origin=(0, 0, 0), dims=(8, 8, 8), color=True, raycast="color"), None),      # without hashed=True
                  (dict(model, color=True, raycast="color"), {}),                                    # with sdf
                  (dict(model, color=True, raycast="color", keep_radius=3.0), None),                 # with keep_radius
                  (dict(model, color=True, raycast="colour"), None)]                                 # not a ray-cast loop
    for bad_model, sdf in bad_models:
        with pytest.raises(ValueError):
            tum.track(None, seq, model=bad_model, sdf=sdf)
        with pytest.raises(ValueError):
            tum.reconstruct_room(None, seq, model=bad_model, sdf=sdf)
    with pytest.raises(ValueError, match="colour frames"):
        tum.track(None, dict(seq, rgbx=None), model=dict(model, color=True, raycast="color"))
    assert "6zc" in tum.track.__doc__ and 'raycast="color"' in tum.track.__doc__


def test_recorded_outcome_separates_the_two_loops():
    """tests/golden/htsdf_color_view_outcome.json, written by tests/htsdf_color_view_outcome_fixture.py on the CPU: the coloured hashed
    model loop stays within 0.0022 m over the 0.11 m of travel, the geometric hashed ray-cast loop ends 0.1098 m off -- the condition the
    fixture script asserts before any device sees the fixture."""
    with open(VOF.GOLDEN) as f:
        ref = json.load(f)
    print(ref)
    travel = ref["lateral_travel_m"]
    assert ref["frames"] == 12 and (ref["width"], ref["height"]) == (160, 120) and ref["n_blocks"] > 10
    assert 0 < ref["colored_last_translation_m"] <= ref["colored_worst_translation_m"]
    assert 2 * ref["colored_worst_translation_m"] < travel / 2 < ref["geometric_last_translation_m"]
    m = VOF.hashed_model()
    assert m["hashed"] and m["color"] and m["raycast"] == "color" and "dims" not in m and VOF.hashed_model(False)["raycast"] is True
