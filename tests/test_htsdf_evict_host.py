"""Streaming the hashed TSDF volume on the host side: the new struct, symbols, signatures and Python surface, the ValueErrors, the evict
predicate on a lattice that is exact in fp32, evict-then-insert as the identity in the restatement, the fixture of the local loop (chosen
here on the restatement alone and recorded in tests/golden/htsdf_evict_outcome.json) with the conditions it must satisfy and the restated
local loop against the restated unbounded one bit for bit, and the resource record of the five new kernels (compile only)."""
import ctypes
import inspect
import json
import os
import re
import numpy as np
import pytest

import htsdf_restatement as HR
import htsdf_evict_restatement as ER
import htsdf_evict_fixture as EF
import tsdf_restatement as TS
from device_asm import device_asm, kernel_resources
from support import same_bits

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32

# the lattice: 9 x 9 x 9 blocks, b in -4 .. 4, voxel 1/16 m (a block is 0.5 m), a dyadic origin; the centre of block (0, 0, 0)
LATTICE = dict(origin=(0.5, -0.25, 1.0), voxel_size=0.0625, truncation=0.25)
LATTICE_CENTRE = tuple(o + 3.5 * 0.0625 for o in LATTICE["origin"])


def lattice_coords():
    g = np.arange(-4, 5)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.int32)


def lattice_volume(seed=5):
    """The lattice as an HVolume with crafted contents (every block distinct)."""
    rng = np.random.default_rng(seed)
    hv = HR.HVolume(**LATTICE)
    cc = lattice_coords()
    hv.allocate(cc)
    for b in cc:
        hv.blocks[tuple(int(v) for v in b)] = [rng.uniform(-1, 1, (8, 8, 8)).astype(f32), rng.integers(0, 5, (8, 8, 8)).astype(f32)]
    return hv, cc


def test_struct_symbols_and_python_surface():
    from icp_amd import binding, tsdf_local, tum
    T = binding.IcpTsdfStreamInfo
    assert ctypes.sizeof(T) == 32 and T.capacity.offset == 12 and T.n_held.offset == 16 and T.n_present.offset == 24
    assert [f[0] for f in T._fields_] == list(ER.INFO)
    assert ctypes.sizeof(binding.IcpTsdfHashedInfo) == 24      # (keeps its layout)
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    sig = {"icp_tsdf_evict_blocks": r"icp_ctx\* ctx, const float centre\[3\], float radius, int32_t hold, icp_tsdf_stream_info\* info_out",
           "icp_tsdf_evicted_blocks": r"icp_ctx\* ctx, int32_t max_blocks, int32_t\* coords_out, float\* tsdf_out, float\* weight_out",
           "icp_tsdf_insert_blocks": r"icp_ctx\* ctx, int32_t n, const int32_t\* coords, const float\* tsdf, const float\* weight, icp_tsdf_stream_info\* info_out"}
    for name, args in sig.items():
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(%s\);" % (name, args), hdr, flags=re.M), name
    assert re.search(r"^\} icp_tsdf_stream_info;", hdr, flags=re.M) and "static_assert(sizeof(icp_tsdf_stream_info) == 32" in hdr
    assert list(inspect.signature(binding.Context.tsdf_evict_blocks).parameters) == ["self", "centre", "radius", "hold"]
    assert inspect.signature(binding.Context.tsdf_evict_blocks).parameters["hold"].default is True
    assert list(inspect.signature(binding.Context.tsdf_insert_blocks).parameters) == ["self", "coords", "tsdf", "weight"]
    assert list(inspect.signature(binding.tsdf_view_reach).parameters) == ["cam", "options"]
    par = inspect.signature(tsdf_local.track_depth_sdf_local).parameters
    assert list(par)[:6] == ["ctx", "frames", "cam", "keep_radius", "pose", "store"] and par["pose"].default is None and par["store"].default is None
    assert list(inspect.signature(tsdf_local.restore).parameters) == ["ctx", "store"]
    for m in ("add", "take_within", "blocks", "__len__", "nbytes"):
        assert hasattr(tsdf_local.BlockStore, m), m
    assert "keep_radius" in tum.track.__doc__
    # a null context is refused by every new entry point
    ce = np.zeros(3, f32)
    assert lib.icp_tsdf_evict_blocks(None, binding._ptr(ce), ctypes.c_float(1.0), 1, None) == 1
    assert lib.icp_tsdf_evicted_blocks(None, 0, None, None, None) == 1
    assert lib.icp_tsdf_insert_blocks(None, 0, None, None, None, None) == 1


def test_value_errors_and_reach():
    from icp_amd import binding, tsdf_local, tum
    from icp_amd.synth import tum_K
    cam = binding.depth_camera(tum_K(EF.W), EF.W, EF.H)
    rcam = TS.Camera(tum_K(EF.W), EF.W, EF.H)
    reach = binding.tsdf_view_reach(cam, dict(EF.VOLUME))
    assert reach == pytest.approx(ER.view_reach(rcam, HR.HVolume(**EF.VOLUME)), rel=1e-6)
    # by hand: a_max = max(cx, W - 1 - cx) / fx, b_max likewise; (1.3 + 0.2) sqrt(1 + a^2 + b^2) + 0.4 sqrt(3)
    K = tum_K(EF.W).astype(np.float64)
    a = max(K[0, 2], EF.W - 1 - K[0, 2]) / K[0, 0]; b = max(K[1, 2], EF.H - 1 - K[1, 2]) / K[1, 1]
    assert reach == pytest.approx(1.5 * np.sqrt(1 + a * a + b * b) + 0.4 * np.sqrt(3.0), rel=1e-6)
    assert np.isinf(binding.tsdf_view_reach(cam, dict(EF.VOLUME, max_depth=np.inf)))

    class Ctx:                                      # only what track_depth_sdf_local reads before it refuses
        pass
    c = Ctx(); c.tsdf_hashed_options = binding.tsdf_options(**EF.VOLUME)
    frames = np.zeros((2, EF.H, EF.W), f32)
    for r in (reach * 0.999, 0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            tsdf_local.track_depth_sdf_local(c, frames, cam, r)
    c.tsdf_hashed_options = binding.tsdf_options(**dict(EF.VOLUME, max_depth=np.inf))
    with pytest.raises(ValueError, match="max_depth"):
        tsdf_local.track_depth_sdf_local(c, frames, cam, 1e6)
    seq = dict(depth=frames, rgbx=None, gt=None, K=tum_K(EF.W), width=EF.W, height=EF.H)
    dense = dict(dims=(16, 16, 16), origin=(0, 0, 0), keep_radius=5.0)
    with pytest.raises(ValueError, match="keep_radius"):
        tum.track(None, seq, model=dense, sdf={})
    with pytest.raises(ValueError, match="keep_radius"):
        tum.track(None, seq, model=dict(EF.VOLUME, hashed=True, raycast=True, keep_radius=5.0))
    # the store: add, take, sorted, and the key it holds already
    st = tsdf_local.BlockStore()
    cc = lattice_coords()[::-1]
    t = np.arange(len(cc) * 512, dtype=f32).reshape(-1, 8, 8, 8); w = t + 1
    st.add(cc, t, w)
    assert len(st) == 729 and st.nbytes == 729 * 4096
    with pytest.raises(KeyError):
        st.add(cc[:1], t[:1], w[:1])
    sc, stt, sw = st.blocks()
    order = np.lexsort((cc[:, 0], cc[:, 1], cc[:, 2]))
    assert np.array_equal(sc, cc[order]) and same_bits(stt, t[order]) and same_bits(sw, w[order])
    tc, tt, tw = st.take_within(LATTICE_CENTRE, 1.5, LATTICE["origin"], LATTICE["voxel_size"])
    assert len(tc) == 123 and len(st) == 606 and ((tc.astype(np.int64) ** 2).sum(1) <= 9).all()
    for bad in ((np.nan, 0, 0), ):
        with pytest.raises(ValueError):
            st.take_within(bad, 1.0, LATTICE["origin"], LATTICE["voxel_size"])
    with pytest.raises(ValueError):
        st.take_within(LATTICE_CENTRE, -1.0, LATTICE["origin"], LATTICE["voxel_size"])
    assert np.array_equal(tsdf_local.block_centres_kept(cc, LATTICE_CENTRE, 1.5, LATTICE["origin"], LATTICE["voxel_size"]),
                          ER.kept(cc, LATTICE["origin"], LATTICE["voxel_size"], LATTICE_CENTRE, 1.5))


def test_predicate_on_exact_cases():
    """Radius 1.5 m = three blocks: the kept set is exactly dx^2 + dy^2 + dz^2 <= 9 in blocks, the blocks ON the sphere included ((+-3, 0, 0),
    (2, 2, 1) and their kin): 123 of 729, section 6v's count; radius 0 keeps the centre block alone; radius 2e19 (r2 infinite) keeps all."""
    cc = lattice_coords()
    o, s = LATTICE["origin"], LATTICE["voxel_size"]
    p = np.asarray(o) + (8.0 * cc + 3.5) * s
    assert np.array_equal((np.asarray(o, f32) + ((8 * cc).astype(f32) + f32(3.5)) * f32(s)).astype(np.float64), p)      # exact in fp32
    k = ER.kept(cc, o, s, LATTICE_CENTRE, 1.5)
    want = (cc.astype(np.int64) ** 2).sum(1) <= 9
    assert np.array_equal(k, want) and k.sum() == 123
    got = {tuple(int(v) for v in b) for b in cc[k]}
    assert {(3, 0, 0), (-3, 0, 0), (0, 0, 3), (2, 2, 1), (-2, -2, -1), (1, 2, 2)} <= got and (3, 1, 0) not in got
    assert [tuple(b) for b in cc[ER.kept(cc, o, s, LATTICE_CENTRE, 0.0)]] == [(0, 0, 0)]
    with np.errstate(over="ignore"):
        assert ER.kept(cc, o, s, LATTICE_CENTRE, 2e19).all() and not np.isfinite(f32(2e19) * f32(2e19))
    hv, _ = lattice_volume()
    n, out = ER.evict(hv, LATTICE_CENTRE, 1.5)
    assert n == 606 and len(hv.blocks) == 123 and set(hv.blocks) == got and not (set(out) & set(hv.blocks))
    for centre, radius in (((np.nan, 0, 0), 1.0), ((0, np.inf, 0), 1.0), ((0, 0, 0), -1.0), ((0, 0, 0), np.nan), ((0, 0, 0), np.inf)):
        with pytest.raises(ER.BadOptions):
            ER.evict(hv, centre, radius)


def test_evict_then_insert_is_the_identity():
    hv, cc = lattice_volume()
    before = hv.sorted_blocks()
    for radius in (0.0, 0.9, 1.5, 2e19):
        n, out = ER.evict(hv, LATTICE_CENTRE, radius)
        assert n == len(out) == 729 - len(hv.blocks)
        with pytest.raises(ER.BadOptions):
            ER.insert(hv, {next(iter(hv.blocks)): [np.zeros((8, 8, 8), f32)] * 2})
        ER.insert(hv, out)
        after = hv.sorted_blocks()
        assert np.array_equal(after[0], before[0]) and same_bits(after[1], before[1]) and same_bits(after[2], before[2])
    with pytest.raises(ER.BadOptions):
        ER.insert(hv, {(1 << 20, 0, 0): [np.zeros((8, 8, 8), f32)] * 2})


def test_fixture_of_the_local_loop():
    """The out-and-back slide along the wavy wall (tests/htsdf_evict_fixture.py) on the restatement: blocks leave on at least three frames
    and come back on at least three; the peak resident count (after a frame's integrate, before its evict) is <= 2^7 < the number of
    blocks of the whole model; keep_radius is the reach plus twice the step and every tracked step stays below that margin; and the local
    loop's poses, records and the union of resident and stored blocks equal the unbounded loop's bit for bit.  The recorded outcome
    (tests/golden/htsdf_evict_outcome.json) is what this run gives."""
    run = EF.restatement_runs()
    out = EF.outcome(run)
    with open(EF.GOLDEN) as f:
        gold = json.load(f)
    print("local loop: evicted %s, inserted %s, peak %d, total %d, margin %.2e m" % (out["n_evicted"], out["n_inserted"], out["peak_resident"], out["total_blocks"], out["margin_m"]))
    for k in ("frames", "width", "height", "n_evicted", "n_inserted", "n_resident", "n_stored", "peak_resident", "total_blocks", "statuses"):
        assert out[k] == gold[k], k
    assert out["frames"] == 2 * EF.N_OUT + 1 and EF.W <= 64 and EF.H <= 48
    assert sum(1 for n in out["n_evicted"] if n) >= 3 and sum(1 for n in out["n_inserted"] if n) >= 3
    assert out["peak_resident"] <= 2 ** 7 < out["total_blocks"]
    reach = ER.view_reach(run["cam"], run["loc"])
    assert run["keep_radius"] == pytest.approx(reach + 2 * EF.STEP, rel=1e-6) and out["largest_step_m"] < 2 * EF.STEP and out["statuses"] == [0]
    assert out["margin_m"] > 1e-4                      # (no block centre near the sphere: a device run's poses, a few ulps away, give the same counts)
    assert len(run["lposes"]) == len(run["fposes"]) == out["frames"]
    for a, b in zip(run["lposes"], run["fposes"]):
        assert same_bits(a, b)
    for a, b in zip(run["lrecs"], run["frecs"]):
        assert a.keys() == b.keys()
        for key in a:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    u, full = ER.union_blocks(run["loc"], run["store"]), run["full"].sorted_blocks()
    assert np.array_equal(u[0], full[0]) and same_bits(u[1], full[1]) and same_bits(u[2], full[2])
    assert not (set(run["loc"].blocks) & set(run["store"]))


NEW_KERNELS = ("_ZN6icpdev18k_htsdf_evict_mark", "_ZN6icpdev17k_htsdf_evict_out", "_ZN6icpdev18k_htsdf_evict_plan", "_ZN6icpdev18k_htsdf_evict_move",
               "_ZN6icpdev15k_htsdf_present")


def test_kernel_resource_record():
    """The five new kernels from the compiled code object: no scratch, no AGPRs, no static LDS, VGPRs within the budget of eight waves per
    SIMD (64).  Recorded: DESIGN.md section 6za."""
    text = device_asm()
    seen = kernel_resources(text)
    for prefix in NEW_KERNELS:
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        desc = text[text.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        print("%s: %d VGPRs, %d AGPRs, scratch %d B, static LDS %d B" % (prefix, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
        assert f["private_seg_size"] == 0 and f.get("num_agpr", 0) == 0 and lds == 0, f
        assert f["num_vgpr"] <= 64, f
    for prefix in ("_ZN6icpdev14k_htsdf_rehash", "_ZN6icpdev13k_htsdf_place", "_ZN6icpdev13k_htsdf_alloc"):
        assert len([n for n in seen if n.startswith(prefix)]) == 1, prefix
