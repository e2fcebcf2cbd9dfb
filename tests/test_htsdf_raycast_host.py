"""The ray-cast of the hashed TSDF volume on the host side: the numpy restatement of the contract (tests/htsdf_raycast_restatement.py)
against tsdf_restatement's ray-cast on the densified volume bit for bit, the classes of samples the cases must contain, the events of the
end rule on the crafted volume, the empty cases, the wrappers' argument checks, the symbols, the resource record of the new kernel
(compile only) and the recorded outcome reference."""
import ctypes
import json
import os
import re
import numpy as np
import pytest

import htsdf_raycast_cases as RC
import htsdf_raycast_outcome_fixture as ROF
import htsdf_raycast_restatement as RR
import tsdf_outcome_fixture as OF
import tsdf_restatement as TS
from device_asm import device_asm, kernel_resources
from support import same_bits

f32 = np.float32
MINF = f32(-np.inf)
BIG = len(RC.SIZES) - 1                                          # 64 x 48


def names(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("ci", range(len(RC.dense_equality_cases())), ids=names(RC.dense_equality_cases()))
def test_restatement_equals_the_dense_restatement(ci):
    """P, and A - D moved to non-negative block coordinates: depth, vertices, normals and hit count of the restated hashed ray-cast against
    tsdf_restatement.raycast on tsdf_blocks_to_dense(lo = 0) with the same origin, bit for bit, at every camera size and every pose."""
    name, opts, c, t, w, poses = RC.dense_equality_cases()[ci]
    d_opts, T, W = RC.dense_lo0(opts, c, t, w)
    dv = TS.Volume(**d_opts); dv.tsdf, dv.weight = T, W
    total = 0
    for si, (cw, ch) in enumerate(RC.SIZES):
        for pi, P in enumerate(poses):
            got = RC.restated(ci, si, pi, "dense")
            want = TS.raycast(dv, RC.camera(cw, ch)[1], P)
            assert got[3] == want[3], (name, cw, ch, pi)
            for a, b in zip(got[:3], want[:3]):
                assert same_bits(a, b), (name, cw, ch, pi)
            total += got[3]
    print("%s: %d hits over %d casts" % (name, total, len(RC.SIZES) * len(poses)))
    assert total > 100


def traces(prefix):
    out = []
    for ci, case in enumerate(RC.all_cases()):
        if case[0].startswith(prefix):
            out += [RC.restated(ci, BIG, pi)[4] for pi in range(len(case[5]))]
    return out


def test_the_cases_contain_every_class():
    """Every evaluated sample of B and C by the number of distinct blocks its cell touches: 1, 2, 4 and 8 each occur with valid and with
    invalid members, and so does the cell with exactly one corner's block missing (never valid: that corner reads W = 0).  A has no
    neighbour: no valid cell beyond its one block."""
    tot = {(t, v): 0 for t in (1, 2, 4, 8) for v in (True, False)}
    one = {True: 0, False: 0}
    for tr in traces("B") + traces("C"):
        for k in tot:
            tot[k] += tr["classes"][k]
        for k in one:
            one[k] += tr["one_missing"][k]
    print("B, C:", tot, "one missing:", one)
    for k, v in tot.items():
        assert v > 0, k
    assert one[False] > 0 and one[True] == 0
    b = traces("B")
    assert all(tr["one_missing"][False] == 0 for tr in b) and sum(tr["classes"][(8, True)] for tr in b) > 0
    assert sum(tr["hits"] for tr in b) > 100 and sum(tr["first_valid_nonpositive"] for tr in b) > 0      # seen from outside and from inside
    for tr in traces("A"):
        assert all(tr["classes"][(t, True)] == 0 for t in (2, 4, 8))
    # the fused volumes hold every class as well
    for prefix in ("P", "NEG"):
        for k in tot:
            assert sum(tr["classes"][k] for tr in traces(prefix)) > 0, (prefix, k)


def test_the_crafted_volume_meets_every_clause_of_the_end_rule():
    """D: a ray passes a NaN sample without ending; a ray's first valid sample is F <= 0 (no hit: prev_valid is false); a crossing directly
    behind an invalid sample is rejected; and rays still hit."""
    tr = traces("D")
    got = {k: sum(t[k] for t in tr) for k in ("nan_passed", "first_valid_nonpositive", "crossing_behind_invalid", "hits", "ended_without_hit")}
    print("D:", got)
    for k, v in got.items():
        assert v > 0, k
    assert got["ended_without_hit"] >= got["first_valid_nonpositive"] + got["crossing_behind_invalid"]
    # a NaN alone never ends a ray: one block of NaN with weight 1 in front of nothing
    nan_block = RR.Blocks([(0, 0, 0)], np.full((1, 8, 8, 8), np.nan, f32), np.ones((1, 8, 8, 8), f32), origin=(-0.5, -0.5, 0.5), voxel_size=0.125, truncation=0.5, max_depth=3.0)
    t = {}
    d, v, n, hits = RR.raycast(nan_block, RC.camera(7, 5)[1], np.eye(4, dtype=f32), trace=t)
    assert hits == 0 and t["nan_passed"] > 0 and t["ended_without_hit"] == 0 and (d == MINF).all()


def test_samples_beyond_the_storable_range_are_invalid_without_a_cast():
    tr = traces("F")
    print("F: out of range %s, hits %s" % ([t["out_of_range"] for t in tr], [t["hits"] for t in tr]))
    assert all(t["out_of_range"] > 0 for t in tr) and sum(t["hits"] for t in tr) > 100
    assert all(t["classes"][(1, True)] > 0 for t in tr)


def test_empty_cases_give_all_holes():
    """An empty volume, a pose looking away, and min_depth > max_depth (no sample at all): all holes and no hit."""
    name, opts, c, t, w, poses = RC.all_cases()[0]
    cam = RC.camera(17, 33)[1]
    away = RC.pose((0.0, np.pi, 0.0), (0.0, 0.0, -1.0))
    for what, vol, P in (("empty", RR.Blocks(np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), f32), np.zeros((0, 8, 8, 8), f32), **opts), poses[0]),
                         ("away", RR.Blocks(c, t, w, **opts), away),
                         ("no march", RR.Blocks(c, t, w, **dict(opts, min_depth=3.0, max_depth=2.4)), poses[0])):
        tr = {}
        d, v, n, hits = RR.raycast(vol, cam, P, trace=tr)
        assert hits == 0 and (d == MINF).all() and (v == MINF).all() and (n == MINF).all(), what
        if what == "no march":
            assert tr["samples"] == 0


def test_wrapper_argument_checks():
    """The three wrappers and tum.track refuse bad arguments before they touch the context."""
    from icp_amd import binding, tum
    cam = binding.depth_camera(np.eye(3), 4, 4)
    for bad in (np.eye(3), np.zeros(16), None):
        with pytest.raises(ValueError):
            binding.Context.tsdf_raycast_hashed(None, cam, bad)
        with pytest.raises(ValueError):
            binding.Context.set_target_tsdf_hashed(None, cam, bad)
    so = binding.depth_options(False, 2)
    with pytest.raises(ValueError, match="camera"):
        binding.Context.track_depth_model_hashed(None, np.zeros((3, 5, 4), f32), cam, so)
    with pytest.raises(ValueError, match="gt"):
        binding.Context.track_depth_model_hashed(None, np.zeros((3, 4, 4), f32), cam, so, gt=[np.eye(4)])
    with pytest.raises(ValueError, match="4x4"):
        binding.Context.track_depth_model_hashed(None, np.zeros((3, 4, 4), f32), cam, so, pose=np.eye(3))
    seq = dict(K=np.eye(3), width=4, height=4, depth=[], rgbx=[], frames=[], gt=[])
    model = dict(hashed=True, origin=(0, 0, 0), voxel_size=0.1)
    ray = dict(model, raycast=True)
    for bad_model, sdf in ((model, None), (dict(ray, dims=(8, 8, 8)), None), (dict(ray, color=True), None), (ray, {}), (ray, dict(stride=4)),
                           (dict(dims=(8, 8, 8), origin=(0, 0, 0), raycast=True), None), (dict(dims=(8, 8, 8), origin=(0, 0, 0), raycast=True), {})):
        with pytest.raises(ValueError):
            tum.track(None, seq, model=bad_model, sdf=sdf)
        with pytest.raises(ValueError):
            tum.reconstruct_room(None, seq, model=bad_model, sdf=sdf)
    with pytest.raises(ValueError, match="raycast"):
        tum.track(None, seq, model=ray, sdf={})
    with pytest.raises(ValueError, match="hashed"):
        tum.track(None, seq, model=dict(dims=(8, 8, 8), origin=(0, 0, 0), raycast=True))


def test_symbols_and_python_surface():
    from icp_amd import binding
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    lib = binding.load_library()
    hdr = open(os.path.join(root, "include", "icp_hip.h")).read()
    for sym in ("icp_tsdf_raycast_hashed", "icp_set_target_tsdf_hashed", "icp_track_depth_model_hashed"):
        assert sym in binding.EXPORTS and hasattr(lib, sym) and re.search(r"^int %s\(" % sym, hdr, flags=re.M), sym
    assert hasattr(lib, "icp_debug_htsdf_raycast_time") and "icp_debug_htsdf_raycast" not in hdr
    for name in ("tsdf_raycast_hashed", "set_target_tsdf_hashed", "track_depth_model_hashed"):
        assert hasattr(binding.Context, name)
    n = ctypes.c_int32(7)
    assert lib.icp_tsdf_raycast_hashed(None, None, None, None, None, None, ctypes.byref(n)) == 1      # a null context
    assert lib.icp_set_target_tsdf_hashed(None, None, None, ctypes.byref(n)) == 1
    assert lib.icp_track_depth_model_hashed(None, None, 0, None, None, None, None, None) == 1
    assert not hasattr(lib, "icp_tsdf_raycast_hashed_color") and "_hashed_color" not in hdr             # the hashed volume holds no colours


def test_kernel_resource_record():
    """k_htsdf_raycast<false> and <true> from the compiled code object: no scratch, no AGPRs, 92 VGPRs each -- pinned at 96, the
    allocation step above (five waves per SIMD; the dense k_tsdf_raycast takes 48) --, 16 bytes of LDS (the block sum), and no atomic
    but the integer add of the hit count."""
    text = device_asm()
    seen = kernel_resources(text)
    ks = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev15k_htsdf_raycastILb")}
    assert len(ks) == 2, list(ks)
    for name, f in ks.items():
        desc = text[text.index(".amdhsa_kernel " + name):]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        print("%s: %d VGPRs, %d AGPRs, scratch %d B, LDS %d B" % (name, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
        assert f["private_seg_size"] == 0, f
        assert f["num_vgpr"] <= 96 and f.get("num_agpr", 0) == 0, f
        assert lds <= 16, lds
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        atomics = re.findall(r"^\s*((?:global|flat|buffer|ds)_atomic\w*)", body, flags=re.M)
        assert atomics and all(re.fullmatch(r"(global|flat)_atomic_add(_u32)?", a) for a in atomics), atomics


def test_outcome_reference():
    """tests/golden/htsdf_raycast_outcome.json, written by tests/htsdf_raycast_outcome_fixture.py (CPU: the restated hashed integrate and
    ray-cast, the oracle's ICP): the 41-frame pan at the dense fixture's voxel size, truncation and ray step.  The reference itself must
    have held the track -- the pan turns 1.05 rad and travels 0.4 m, a lost track ends tenths off; 0.05 rad / 0.15 m is a twentieth of the
    turn -- since the device's bound is twice these figures."""
    with open(ROF.GOLDEN) as f:
        ref = json.load(f)
    print(ref)
    assert (ref["frames"], ref["width"], ref["height"]) == (OF.N_FRAMES, OF.W, OF.H)
    assert (ref["voxel_size"], ref["truncation"], ref["ray_step"]) == (OF.VOLUME["voxel_size"], OF.VOLUME["truncation"], OF.VOLUME["ray_step"])
    assert 0 < ref["last_rotation_rad"] <= ref["worst_rotation_rad"] < 0.05 and 0 < ref["last_translation_m"] <= ref["worst_translation_m"] < 0.15
    assert ref["n_blocks"] > ref["n_blocks_first"] > 100 and ref["min_hits"] > 1000 and ref["n_out_of_range"] == 0
    m = ROF.hashed_model()
    assert m["hashed"] and m["raycast"] and "dims" not in m
