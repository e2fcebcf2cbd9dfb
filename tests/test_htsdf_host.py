"""The hashed TSDF volume on the host side: the new struct, symbols, signatures and Python surface, the argument checks that need no
device, the numpy restatement (tests/htsdf_restatement.py) against tsdf_restatement's dense volume voxel for voxel and sample for sample,
and the resource record of the new kernels (compile only)."""
import ctypes
import inspect
import os
import re
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_restatement as HR
import sdf_restatement as SR
import tsdf_restatement as TS
from device_asm import device_asm, kernel_resources
from support import same_bits

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def test_struct_symbols_and_python_surface():
    from icp_amd import binding, tum
    assert ctypes.sizeof(binding.IcpTsdfHashedInfo) == 24
    assert [f[0] for f in binding.IcpTsdfHashedInfo._fields_] == ["n_blocks", "capacity", "n_grown", "n_unplaced", "n_out_of_range"]
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    sig = {"icp_tsdf_create_hashed": r"icp_ctx\* ctx, const icp_tsdf_options\* opt, int32_t block_capacity",
           "icp_tsdf_reserve_blocks": r"icp_ctx\* ctx, int32_t block_capacity",
           "icp_tsdf_allocate_blocks": r"icp_ctx\* ctx, int32_t n, const int32_t\* coords",
           "icp_get_tsdf_hashed": r"icp_ctx\* ctx, icp_tsdf_hashed_info\* info_out, int32_t max_blocks, int32_t\* coords_out, float\* tsdf_out, float\* weight_out",
           "icp_tsdf_upload_hashed": r"icp_ctx\* ctx, int32_t n, const int32_t\* coords, const float\* tsdf, const float\* weight"}
    for name, args in sig.items():
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(%s\);" % (name, args), hdr, flags=re.M), name
    assert re.search(r"^\} icp_tsdf_hashed_info;", hdr, flags=re.M)
    for m in ("tsdf_create_hashed", "tsdf_reserve_blocks", "tsdf_allocate_blocks", "tsdf_blocks", "tsdf_upload_blocks"):
        assert hasattr(binding.Context, m), m
    assert inspect.signature(binding.Context.tsdf_create_hashed).parameters["block_capacity"].default == 1 << 12
    assert hasattr(binding, "tsdf_blocks_to_dense") and hasattr(tum, "densify_hashed_model")


def test_argument_checks_without_a_device():
    """Every new entry point refuses a null context; tum.track refuses a hashed model without sdf, with dims or with colour before it
    touches the context."""
    from icp_amd import binding, tum
    lib = binding.load_library()
    o = binding.tsdf_options(origin=(0, 0, 0))
    assert lib.icp_tsdf_create_hashed(None, ctypes.byref(o), 16) == 1 and lib.icp_tsdf_reserve_blocks(None, 16) == 1
    assert lib.icp_tsdf_allocate_blocks(None, 0, None) == 1 and lib.icp_get_tsdf_hashed(None, None, 0, None, None, None) == 1
    assert lib.icp_tsdf_upload_hashed(None, 0, None, None, None) == 1
    seq = dict(K=np.eye(3, dtype=f32), width=4, height=4, depth=np.zeros((1, 4, 4), f32), rgbx=None, gt=None)
    model = dict(hashed=True, origin=(0, 0, 0), voxel_size=0.1)
    for bad_model, sdf in ((model, None), (dict(model, dims=(8, 8, 8)), {}), (dict(model, color=True), {})):
        with pytest.raises(ValueError):
            tum.track(None, seq, model=bad_model, sdf=sdf)
    # M = ceil(2 truncation / s) in double of the fp32 values: 2 * 0.3f / 0.1f = 6.0000001, so 7 steps; 0.25 and 0.0625 are exact
    assert HR.n_steps(HR.HVolume(**HC.STRADDLE)) == 7 and HR.n_steps(HR.HVolume(**HC.NEG)) == 8
    assert HR.n_steps(HR.HVolume(origin=(0, 0, 0), voxel_size=0.05, truncation=0.25)) == 10


def test_blocks_to_dense_and_back():
    """binding.tsdf_blocks_to_dense: blocks land at 8 b - lo, x fastest; what no block covers is (0, 0); what leaves dims is dropped."""
    from icp_amd import binding
    rng = np.random.default_rng(3)
    coords = np.array([[-1, 0, 2], [0, 0, 2], [1, -2, -1]], np.int32)
    t = rng.uniform(-1, 1, (3, 8, 8, 8)).astype(f32); w = rng.integers(1, 9, (3, 8, 8, 8)).astype(f32)
    lo = (-8, -16, -8)
    T, Wt = binding.tsdf_blocks_to_dense(coords, t, w, lo, (24, 24, 32))
    assert T.shape == (32, 24, 24)
    assert same_bits(T[24:32, 16:24, 0:8], t[0]) and same_bits(T[24:32, 16:24, 8:16], t[1]) and same_bits(Wt[0:8, 0:8, 16:24], w[2])
    assert (Wt > 0).sum() == 3 * 512 and T[Wt == 0].max() == 0 and T[Wt == 0].min() == 0
    assert T[24 + 3, 16 + 2, 1] == t[0][3, 2, 1]
    T2, W2 = HR.blocks_to_dense(coords, t, w, lo, (24, 24, 32))
    assert same_bits(T, T2) and same_bits(Wt, W2)
    Tc, Wc = binding.tsdf_blocks_to_dense(coords, t, w, (-4, -16, -8), (8, 24, 32))      # cuts blocks 0 and 1 in half, drops block 2
    assert same_bits(Tc[24:32, 16:24, 0:4], t[0][:, :, 4:]) and same_bits(Tc[24:32, 16:24, 4:8], t[1][:, :, :4]) and (Wc > 0).sum() == 512


@pytest.mark.parametrize("case", ["box", "negative"])
def test_restated_integrate_equals_the_dense_restatement(case):
    """With every block of a box allocated first, three frames integrated into the restated hashed volume equal tsdf_restatement.integrate
    on the dense box bit for bit, voxel for voxel, and so does the count of every frame.  box: the box at non-negative coordinates, the same
    origin.  negative: blocks at negative coordinates on every axis, voxel 1/16 m and an origin that is a multiple of it, the dense origin
    shifted by whole voxels (exact)."""
    opts, lo, nb = (HC.BOX, (0, 0, 0), tuple(d // 8 for d in HC.BOX_DIMS)) if case == "box" else (HC.NEG, HC.NEG_LO, HC.NEG_BLOCKS)
    _, rcam = HC.camera()
    hv = HR.HVolume(**opts)
    hv.allocate(HC.box_coords(lo, nb))
    dv = TS.Volume(**HC.dense_options(opts, lo, nb))
    if case == "negative":
        o = np.asarray(opts["origin"], np.float64); s = opts["voxel_size"]
        assert all(float(dv.o[a]) == o[a] + 8 * lo[a] * s for a in range(3))      # the shift is exact
    for depth, pose in zip(HC.frames(), HC.POSES):
        n_h = HR.integrate_allocated(hv, depth, rcam, pose)
        n_d = TS.integrate(dv, depth, rcam, pose)
        assert n_h == n_d and n_d > 1000, (case, n_h, n_d)
    coords, t, w = hv.sorted_blocks()
    T, Wt = HR.blocks_to_dense(coords, t, w, np.asarray(lo) * 8, (dv.nx, dv.ny, dv.nz))
    assert same_bits(T, dv.tsdf) and same_bits(Wt, dv.weight)
    assert Wt.max() == 3 and (Wt > 0).sum() > 3000
    if case == "negative":
        assert (coords.min(0) < 0).all() and (coords.max(0) > 0).all()
    # the key order: z, then y, then x
    key = (coords[:, 2].astype(np.int64) << 42) + (coords[:, 1].astype(np.int64) << 21) + coords[:, 0]
    assert (np.diff(key) > 0).all()


def test_restated_touch():
    """The touch of the tilted crafted frame into the straddling volume: blocks on both sides of 0 on every axis; every voxel the
    integrate writes within the truncation band lies in a touched block's neighbourhood (the integrate over the touched blocks writes the
    voxels a covering box would write in them); a second touch asks for nothing new; an unusable frame asks for nothing."""
    _, rcam = HC.camera()
    hv = HR.HVolume(**HC.STRADDLE)
    d = HC.crafted_frame()
    blocks, oor = HR.touch(hv, d, rcam, HC.TILTED)
    b = np.array(sorted(blocks))
    print("touch: %d blocks, min %s, max %s, %d samples out of range" % (len(b), b.min(0), b.max(0), oor))
    assert oor == 0 and 20 < len(b) < 400 and (b.min(0) < 0).all() and (b.max(0) >= 0).all()
    n = HR.integrate(hv, d, rcam, HC.TILTED)
    assert n > 1000 and set(hv.blocks) == blocks
    again, _ = HR.touch(hv, d, rcam, HC.TILTED)
    assert again == blocks
    # against a dense box over the touched blocks' bounding box: the same values in the touched blocks
    lo = b.min(0); nb = b.max(0) - lo + 1
    full = HR.HVolume(**HC.STRADDLE)
    full.allocate(HC.box_coords(lo, nb))
    HR.integrate_allocated(full, d, rcam, HC.TILTED)
    for c in blocks:
        assert same_bits(full.blocks[c][0], hv.blocks[c][0]) and same_bits(full.blocks[c][1], hv.blocks[c][1])
    empty, oor = HR.touch(hv, np.full((HC.H, HC.W), HC.MINF, f32), rcam, HC.TILTED)
    assert empty == set() and oor == 0
    # beyond the storable range: every sample counted, nothing asked for
    far = HC.TILTED.copy(); far[0, 3] = f32(2.0e6)
    blocks_far, oor_far = HR.touch(hv, d, rcam, far)
    usable = np.isfinite(d) & (d > 0) & (d <= 2.4)
    assert blocks_far == set() and oor_far == int(usable.sum()) * (HR.n_steps(hv) + 1)


def test_restated_sample_equals_the_dense_restatement():
    """sdf_restatement.sample on the restated hashed volume against the same call on the densified volume, bit for bit: the straddling
    volume after three frames, densified over the bounding box of its blocks with the box's first voxel as origin, on the 1/16 m grid so
    that the shifted origin is exact, at points on a 2^-10 lattice (q - o is exact under either origin)."""
    _, rcam = HC.camera()
    hv = HR.HVolume(**HC.NEG)
    for depth, pose in zip(HC.frames(), HC.POSES):
        HR.integrate(hv, depth, rcam, pose)
    coords, t, w = hv.sorted_blocks()
    lo = coords.min(0); nb = coords.max(0) - lo + 1
    dv = TS.Volume(**HC.dense_options(HC.NEG, lo, nb))
    dv.tsdf, dv.weight = HR.blocks_to_dense(coords, t, w, lo.astype(np.int64) * 8, (dv.nx, dv.ny, dv.nz))
    rng = np.random.default_rng(5)
    pts = (np.stack([rng.integers(-1300, 1300, 6000), rng.integers(-1000, 1000, 6000), rng.integers(700, 2800, 6000)], 1).astype(f32) / f32(1024)).astype(f32)
    pts[:4] = [[np.nan, 0, 1], [np.inf, 0, 1], [0, -np.inf, 1], [1e9, 0, 1]]
    F, G, ok = SR.sample(hv, pts)
    Fd, Gd, okd = SR.sample(dv, pts)
    print("sample: %d of %d points valid" % (ok.sum(), len(pts)))
    assert np.array_equal(ok, okd) and same_bits(F, Fd) and same_bits(G, Gd)
    assert 300 < ok.sum() < 5000 and not ok[:4].any()
    # one step's sums too, where the two volumes share their origin (a frame's points are on no lattice): the box at non-negative
    # coordinates, densified from voxel (0, 0, 0)
    hb = HR.HVolume(**HC.BOX)
    for depth, pose in zip(HC.frames(), HC.POSES):
        HR.integrate(hb, depth, rcam, pose)
    cb, tb, wb = hb.sorted_blocks()
    assert cb.min() >= 0
    db = TS.Volume(**dict(HC.BOX, dims=tuple(int(x) for x in (cb.max(0) + 1) * 8)))
    db.tsdf, db.weight = HR.blocks_to_dense(cb, tb, wb, (0, 0, 0), (db.nx, db.ny, db.nz))
    d = HC.crafted_frame()
    ch, sh, _ = SR.system(hb, d, rcam, HC.POSES[2])
    cd, sd, _ = SR.system(db, d, rcam, HC.POSES[2])
    assert ch == cd and ch[1] > 500 and np.array_equal(sh.view(np.uint64), sd.view(np.uint64))
    # and a dense Volume still goes through the dense cell
    assert TS._cell.__name__ == "_either_cell"


def test_kernel_resource_record():
    """The new kernels from the compiled code object: no scratch (private_seg_size 0), no AGPRs, VGPRs within eight waves per SIMD (64)
    for all but the accumulate, which stays within k_sdf_accumulate's budget of four waves per SIMD (128) and its static LDS."""
    text = device_asm()
    seen = kernel_resources(text)
    budget = {"_ZN6icpdev13k_htsdf_touch": 64, "_ZN6icpdev13k_htsdf_alloc": 64, "_ZN6icpdev14k_htsdf_rehash": 64, "_ZN6icpdev13k_htsdf_place": 64,
              "_ZN6icpdev17k_htsdf_integrate": 64, "_ZN6icpdev14k_htsdf_sample": 64, "_ZN6icpdev17k_hsdf_accumulate": 128}
    for prefix, cap in budget.items():
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        print("%s: %d VGPRs, %d AGPRs, scratch %d B" % (prefix, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"]))
        assert f["private_seg_size"] == 0, (name, f)
        assert f["num_vgpr"] <= cap and f.get("num_agpr", 0) == 0, (name, f)
    lds = {}
    for prefix in ("_ZN6icpdev16k_sdf_accumulate", "_ZN6icpdev17k_hsdf_accumulate"):
        (name,) = [n for n in seen if n.startswith(prefix) and "color" not in n]
        desc = text[text.index(".amdhsa_kernel " + name):]
        lds[prefix] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
    assert lds["_ZN6icpdev17k_hsdf_accumulate"] == lds["_ZN6icpdev16k_sdf_accumulate"], lds
    # no floating-point atomics in the new kernels
    for prefix in budget:
        (name,) = [n for n in seen if n.startswith(prefix)]
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert not re.search(r"atomic_(add|pk_add|fadd|fmin|fmax)_(f32|f64|f16)", body), name
