"""The hashed voxel map on the host side: the new struct, symbols, signatures and Python surface, the argument checks that need no device,
the key packing and the home-slot function of the numpy restatement (tests/hmap_restatement.py), that restatement against
vmap_restatement's dense map cell for cell, and the resource record of the new kernels (compile only)."""
import ctypes
import inspect
import os
import re
import numpy as np
import pytest

import hmap_restatement as HR
import vmap_restatement as MR
from device_asm import device_asm, kernel_resources
from support import pose_of
from test_vmap_host import POSE_A, POSE_B, small_cloud

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32, f64 = np.float32, np.float64


def test_struct_symbols_and_python_surface():
    from icp_amd import binding, eth
    assert ctypes.sizeof(binding.IcpVoxelHashMapInfo) == 32
    assert [f[0] for f in binding.IcpVoxelHashMapInfo._fields_] == ["voxel_size", "capacity", "n_occupied", "n_grown", "n_unplaced", "reserved"]
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    sig = {"icp_voxel_map_create_hashed": r"icp_ctx\* ctx, float voxel_size, int32_t capacity",
           "icp_voxel_map_reserve": r"icp_ctx\* ctx, int32_t capacity",
           "icp_get_voxel_map_hashed": r"icp_ctx\* ctx, icp_voxel_hash_map_info\* info_out, int32_t max_entries, int32_t\* coords_out, int32_t\* counts_out,\s+int64_t\* sums_out, float\* cells_out",
           "icp_voxel_map_upload_hashed": r"icp_ctx\* ctx, int32_t n, const int32_t\* coords, const int32_t\* counts, const int64_t\* sums"}
    for name, args in sig.items():
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(%s\);" % (name, args), hdr, flags=re.M), name
    assert re.search(r"^\} icp_voxel_hash_map_info;", hdr, flags=re.M) and 'static_assert(sizeof(icp_voxel_hash_map_info) == 32' in hdr
    for m in ("voxel_map_create_hashed", "voxel_map_reserve", "voxel_map_hashed", "voxel_map_upload_hashed"):
        assert hasattr(binding.Context, m), m
    assert inspect.signature(binding.Context.voxel_map_create_hashed).parameters["capacity"].default == 1 << 16
    par = inspect.signature(eth.track_map).parameters
    assert par["hashed"].default is False and par["capacity"].default == 1 << 16 and par["extent"].default is None and par["margin"].default == 2.0
    with pytest.raises(ValueError):                 # a hashed map has no extent: refused before the context is touched
        eth.track_map(None, [], np.eye(4), hashed=True, extent=((0, 0, 0), (1, 1, 1)))


def test_argument_checks_without_a_device():
    """Every new entry point refuses a null context; the capacity a request becomes (rounded UP to a power of two, 2^8 at least, refused
    outside 1 .. 2^26) as the restatement states it."""
    from icp_amd import binding
    lib = binding.load_library()
    assert lib.icp_voxel_map_create_hashed(None, ctypes.c_float(0.25), 256) == 1 and lib.icp_voxel_map_reserve(None, 256) == 1
    assert lib.icp_get_voxel_map_hashed(None, None, 0, None, None, None, None) == 1 and lib.icp_voxel_map_upload_hashed(None, 0, None, None, None) == 1
    assert [HR.capacity_for(c) for c in (1, 255, 256, 257, 1000, 1 << 16, (1 << 16) + 1, 1 << 26)] == [256, 256, 256, 512, 1024, 1 << 16, 1 << 17, 1 << 26]
    for bad in (0, -1, (1 << 26) + 1):
        with pytest.raises(HR.BadOptions):
            HR.capacity_for(bad)
    for vs in (0.0, -0.25, float("nan"), float("inf")):
        with pytest.raises(HR.BadOptions):
            HR.create(vs)
    m = HR.create(0.25, 300)
    assert m["capacity"] == 512 and m["n_grown"] == 0
    HR.reserve(m, 512); HR.reserve(m, 100)
    assert m["capacity"] == 512 and m["n_grown"] == 0
    HR.reserve(m, 513)
    assert m["capacity"] == 1024 and m["n_grown"] == 1


def test_key_pack_unpack_and_home():
    R = HR.RANGE
    edge = (-R, -1, 0, R - 1)
    seen = set()
    for x in edge:
        for y in edge:
            for z in edge:
                k = HR.pack((x, y, z))
                assert 0 <= k < (1 << 63) and k != HR.EMPTY and HR.unpack(k) == (x, y, z)
                seen.add(k)
    assert len(seen) == 64
    assert HR.pack((-R, -R, -R)) == 0 and HR.pack((R - 1, R - 1, R - 1)) == (1 << 63) - 1
    assert HR.pack((0, 0, 0)) == (R << 42) | (R << 21) | R and HR.pack((1, 0, 0)) == HR.pack((0, 0, 0)) + 1
    assert HR.pack((0, 0, 1)) > HR.pack((0, 1, 0)) > HR.pack((1, 0, 0))      # key order: z, then y, then x
    assert list(HR.storable([[R, 0, 0], [0, -R - 1, 0], [R - 1, -R, 0], [0, 0, 1 << 30]])) == [False, False, True, False]
    for cap in (256, 1 << 13, 1 << 26):
        hs = [HR.home(HR.pack((x, y, 3)), cap) for x in range(-8, 8) for y in range(-8, 8)]
        assert all(0 <= h < cap for h in hs) and len(set(hs)) > 100
    assert HR.home(0, 256) == 0 and HR.home(1, 256) == 0x9E and HR.home(HR.EMPTY >> 1, 1 << 26) == ((HR.EMPTY >> 1) * HR.MUL % (1 << 64)) >> 38
    # the figures of the design note: the shell cells of the 29 x 37 x 15 room in 2^13 slots
    shell = [(x, y, z) for x in range(29) for y in range(37) for z in range(15) if x in (0, 28) or y in (0, 36) or z in (0, 14)]
    assert len(shell) == 3810
    table = {}
    probes = []
    for c in shell:
        s = HR.home(HR.pack((c[0] - 14, c[1] - 18, c[2] - 2)), 1 << 13); n = 1
        while s in table:
            s = (s + 1) & ((1 << 13) - 1); n += 1
        table[s] = c; probes.append(n)
    print("shell of the room in 2^13 slots: longest probe %d, mean %.2f" % (max(probes), float(np.mean(probes))))
    assert max(probes) <= 32 and np.mean(probes) < 2.0


def test_restatement_equals_the_dense_map():
    """200 points at two poses: the hashed restatement equals vmap_restatement's dense map over a covering extent cell for cell, bit for
    bit; insert orders A, B and B, A and shuffled clouds all agree; the info records agree field for field."""
    pts, nrm = small_cloud()
    A, B = pose_of(*POSE_A), pose_of(*POSE_B)
    for vs in (0.25, 0.3):
        lo, dims = (-12, -12, -12), (24, 24, 24)
        d = MR.create(vs, lo, dims)
        ab, ba, sh = HR.create(vs, 256), HR.create(vs, 256), HR.create(vs, 1 << 12)
        want = [MR.insert(d, pts, nrm, A), MR.insert(d, pts[:120], nrm[:120], B)]
        got = [HR.insert(ab, pts, nrm, A), HR.insert(ab, pts[:120], nrm[:120], B)]
        assert got == want and want[0]["n_outside"] == 0 and want[1]["n_cells_new"] > 0
        HR.insert(ba, pts[:120], nrm[:120], B); HR.insert(ba, pts, nrm, A)
        perm = np.random.default_rng(2).permutation(200)
        HR.insert(sh, pts[perm], nrm[perm], A); HR.insert(sh, pts[:120][::-1], nrm[:120][::-1], B)
        ref = HR.dense_entries(d)
        assert len(ref[0]) == d["n_occupied"] > 20
        for m in (ab, ba, sh):
            e = HR.entries(m)
            assert np.array_equal(e[0], ref[0]) and np.array_equal(e[1], ref[1]) and np.array_equal(e[2], ref[2])
            assert np.array_equal(e[3].view(np.uint32), ref[3].view(np.uint32))
        assert ab["capacity"] == 512 and ab["n_grown"] == 1 and sh["n_grown"] == 0      # 2 (0 + 200) > 256
        # a step against the hashed restatement is a step against the dense map
        src = (pts * f32(1.05)).astype(f32)
        a = HR.system(ab, src, nrm, B, 1e-3); b = MR.system(d, src, nrm, B, 1e-3)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        # upload of the entries reproduces the records
        up = HR.create(vs, 256)
        HR.upload(up, *ref[:3])
        assert np.array_equal(HR.entries(up)[3].view(np.uint32), ref[3].view(np.uint32))
    with pytest.raises(HR.BadOptions):
        HR.upload(HR.create(0.25), [[0, 0, 0], [0, 0, 0]], [1, 1], np.zeros((2, 9)))
    with pytest.raises(HR.BadOptions):
        HR.upload(HR.create(0.25), [[HR.RANGE, 0, 0]], [1], np.zeros((1, 9)))
    with pytest.raises(HR.BadOptions):
        HR.upload(HR.create(0.25), [[0, 0, 0]], [-1], np.zeros((1, 9)))


def test_kernel_resource_record():
    """The new kernels from the compiled code object: no scratch, no AGPRs, VGPRs within the budget of eight waves per SIMD (64) for the
    insert and the records as for their dense counterparts, and within k_vgicp_accumulate's own figure plus the key and the probe state
    for k_hmap_accumulate (budget 128: four waves per SIMD, as that kernel).  Static LDS: the pose and the normal matrix (100 bytes) for
    k_hmap_insert; k_vgicp_accumulate's fold buffer for k_hmap_accumulate; none for the others.  Recorded: DESIGN.md section 6u."""
    text = device_asm()
    seen = kernel_resources(text)
    ref = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev18k_vgicp_accumulate")}
    assert len(ref) == 1
    (ref_name, ref_f), = ref.items()
    ref_desc = text[text.index(".amdhsa_kernel " + ref_name):]
    ref_lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", ref_desc).group(1))
    budget = {"_ZN6icpdev13k_hmap_insert": (64, 25 * 4), "_ZN6icpdev14k_hmap_records": (64, 0), "_ZN6icpdev17k_hmap_accumulate": (128, ref_lds),
              "_ZN6icpdev13k_hmap_rehash": (64, 0), "_ZN6icpdev12k_hmap_place": (64, 0)}
    for prefix, (cap, lds_cap) in budget.items():
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        desc = text[text.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        print("%s: %d VGPRs, %d AGPRs, scratch %d B, static LDS %d B" % (prefix, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
        assert f["private_seg_size"] == 0, f
        assert f["num_vgpr"] <= cap and f.get("num_agpr", 0) == 0, f
        assert lds <= lds_cap, lds
    print("k_vgicp_accumulate: %d VGPRs, static LDS %d B" % (ref_f["num_vgpr"], ref_lds))
    # the dense path keeps its kernels: still exactly one of each
    for prefix in ("_ZN6icpdev18k_vgicp_accumulate", "_ZN6icpdev13k_vmap_insert", "_ZN6icpdev14k_vmap_records", "_ZN6icpdev11k_sdf_solve"):
        assert len([n for n in seen if n.startswith(prefix)]) == 1, prefix
