"""Reciprocal (mutual nearest-neighbour) rejection on the host side: the restatement (tests/reciprocal_restatement.py) against a plain fp64
mutual test and on constructed ties and duplicates, the option and stats records, the new symbols and header declarations, argument
validation without a device, and the resource record of k_reciprocal (compile only)."""
import ctypes
import os
import re
import numpy as np

import reciprocal_restatement as RC
from device_asm import device_asm, kernel_resources
from support import pose_of as rigid

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def test_restatement_against_fp64_on_separated_points():
    """Points on a jittered lattice (spacing 0.1, jitter 0.02: every distance margin is far above fp32 rounding), the source a moved, noisy
    copy of part of the target plus extra points: the fp32 test in the source's frame equals the fp64 test in the target's frame."""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.1
    tgt = (g + rng.uniform(-0.02, 0.02, g.shape)).astype(f32)
    T = rigid((0.3, -0.2, 0.5), (0.05, -0.1, 0.2))
    Ti = np.linalg.inv(T.astype(np.float64))
    pick = rng.permutation(len(tgt))[:200]
    extra = rng.uniform(-0.1, 0.8, (150, 3))
    s_world = np.concatenate([tgt[pick] + rng.uniform(-0.015, 0.015, (200, 3)), extra])
    src = (s_world @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)
    from gicp_restatement import transform
    recs = RC.match_brute(transform(T, src), tgt, 1.0)
    assert (recs["idx"] >= 0).all()
    r = RC.reciprocal(recs, T, src, tgt)
    ref = RC.mutual_fp64(T, src, tgt, recs["idx"])
    assert np.array_equal(r["mutual"], ref)
    assert 0 < r["stats"]["n_mutual"] < r["stats"]["n_matched"] == len(src)      # both outcomes occur
    assert np.array_equal(r["recs"]["idx"] >= 0, ref) and (r["recs"]["weight"][~ref] == 0).all() and (r["recs"]["weight"][ref] == 1).all()
    # the engine form agrees with the brute force (here the engine is the brute-force argmin itself)
    def nearest(q):
        D = RC.d2_f32(q[:, None, :], src[None, :, :])
        return np.argmin(D, 1)
    assert np.array_equal(RC.reciprocal(recs, T, src, tgt, nearest=nearest)["mutual"], ref)


def test_restatement_operation_order():
    """q is the transpose of the 3x3 block applied to t - T, each product and sum rounded to fp32 in the stated order."""
    T = rigid((0.7, 0.1, -0.4), (1.5, -2.25, 0.75))
    t = np.array([[0.3, 0.2, 0.1], [1e3, -2e3, 5e2]], f32)
    q = RC.to_source_frame(T, t)
    for k in range(2):
        d = [f32(t[k, a] - T[a, 3]) for a in range(3)]
        for r in range(3):
            want = f32(f32(f32(T[0, r] * d[0]) + f32(T[1, r] * d[1])) + f32(T[2, r] * d[2]))
            assert q[k, r].view(np.uint32) == want.view(np.uint32)
    back = q.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3]
    assert np.abs(back - t).max() <= 1e-3 * 2


def test_ties_and_duplicates():
    eye = np.eye(4, dtype=f32)
    def run(src, tgt, idx):
        recs = np.zeros(len(idx), RC.MATCH_DTYPE); recs["idx"] = idx; recs["weight"] = 1
        return RC.reciprocal(recs, eye, np.asarray(src, f32), np.asarray(tgt, f32))
    # exact duplicates: only the lowest index is mutual
    r = run([[0, 0, 0], [5, 5, 5], [0, 0, 0], [0, 0, 0]], [[0.1, 0, 0]], [0, 0, 0, 0])
    assert r["mutual"].tolist() == [True, False, False, False] and r["stats"] == dict(n_matched=4, n_mutual=1)
    # an exact distance tie between two different points: the lower index wins
    r = run([[1, 0, 0], [-1, 0, 0], [0, 3, 0]], [[0, 0, 0]], [0, 0, 0])
    assert r["mutual"].tolist() == [True, False, False]
    r = run([[0, 3, 0], [-1, 0, 0], [1, 0, 0]], [[0, 0, 0]], [0, 0, 0])
    assert r["mutual"].tolist() == [False, True, False]
    # unmatched records are not judged and stay as they are; non-finite source points are never rivals; a pair whose own d2 is NaN has
    # nothing below it (mutual), one whose own d2 is +inf loses to any finite distance
    recs = np.zeros(4, RC.MATCH_DTYPE); recs["idx"] = [-1, 0, 0, 0]; recs["weight"] = [0, 1, 1, 1]
    src = np.array([[np.nan, 0, 0], [2, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], f32)
    r = RC.reciprocal(recs, eye, src, np.zeros((1, 3), f32))
    assert r["stats"] == dict(n_matched=3, n_mutual=2)
    assert r["recs"]["idx"].tolist() == [-1, 0, 0, -1]
    # orig: the judged index is the original one, not the position in the query set
    src = np.array([[0, 0, 0], [0, 0, 0], [4, 0, 0]], f32)
    recs = np.zeros(2, RC.MATCH_DTYPE); recs["idx"] = 0; recs["weight"] = 1
    r = RC.reciprocal(recs, eye, src, np.zeros((1, 3), f32), orig=[1, 2])
    assert r["mutual"].tolist() == [False, False]
    r = RC.reciprocal(recs, eye, src, np.zeros((1, 3), f32), orig=[0, 2])
    assert r["mutual"].tolist() == [True, False]


def test_structs_defaults_symbols_and_header():
    from icp_amd import binding
    assert ctypes.sizeof(binding.IcpReciprocalOptions) == 4 and ctypes.sizeof(binding.IcpReciprocalStats) == 8
    assert binding.IcpReciprocalStats.n_matched.offset == 0 and binding.IcpReciprocalStats.n_mutual.offset == 4
    lib = binding.load_library()
    o = binding.IcpReciprocalOptions(1)
    assert lib.icp_reciprocal_options_default(ctypes.byref(o)) == 0 and o.enabled == 0
    assert lib.icp_reciprocal_options_default(None) == 1
    names = ("icp_reciprocal_options_default", "icp_set_reciprocal_options", "icp_get_reciprocal_options", "icp_get_reciprocal_stats")
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for name in names:
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert re.search(r"typedef struct icp_reciprocal_options \{\s*int32_t enabled;", hdr)
    assert re.search(r"typedef struct icp_reciprocal_stats \{[^}]*int32_t n_matched;[^}]*int32_t n_mutual;", hdr)
    assert "RIGID" in hdr and "Parity unpinned" in hdr
    assert "setUseReciprocalCorrespondences(bool on)" in open(os.path.join(ROOT, "include", "icp_hip_adaptor.hpp")).read()
    assert hasattr(binding.LinearICPOptimizer, "setUseReciprocalCorrespondences")
    assert hasattr(binding.Context, "set_reciprocal_options") and hasattr(binding.Context, "reciprocal_stats")
    import inspect
    from icp_amd import eth, tum
    for fn in (eth.align, tum.track, tum.reconstruct_room):
        assert inspect.signature(fn).parameters["reciprocal"].default is None, fn


def test_null_context_and_arguments_refused():
    from icp_amd import binding
    lib = binding.load_library()
    o = binding.IcpReciprocalOptions(1)
    st = (binding.IcpReciprocalStats * 2)(); n = ctypes.c_int32(0)
    assert lib.icp_set_reciprocal_options(None, ctypes.byref(o)) == 1
    assert lib.icp_set_reciprocal_options(None, None) == 1
    assert lib.icp_get_reciprocal_options(None, ctypes.byref(o)) == 1
    assert lib.icp_get_reciprocal_stats(None, st, 2, ctypes.byref(n)) == 1


def test_kernel_resource_record():
    """k_reciprocal from the compiled code object: no scratch; the per-lane walk state, the query and the leaf arithmetic fit in 64 VGPRs
    (8 waves per SIMD, what the latency-bound walk wants); static LDS is the block reduction only (32 B), the traversal stack is dynamic
    (2 B x (depth + 1) per lane: 8.5 KB per block at 370 k points).  Recorded: see DESIGN.md section 6l."""
    text = device_asm()
    seen = kernel_resources(text)
    ks = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev12k_reciprocal")}
    assert len(ks) == 1, list(ks)
    (name, f), = ks.items()
    desc = text[text.index(".amdhsa_kernel " + name):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
    print("k_reciprocal: %d VGPRs, %d AGPRs, scratch %d B, static LDS %d B" % (f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
    assert f["private_seg_size"] == 0, f
    assert f["num_vgpr"] <= 64 and f.get("num_agpr", 0) == 0, f
    assert lds <= 64, lds
