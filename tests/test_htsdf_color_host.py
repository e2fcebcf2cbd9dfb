"""The coloured hashed TSDF volume on the host side, on a box of pre-allocated blocks: the restated hashed colour
fusion against tsdf_color_restatement.integrate_color on the dense box voxel for voxel; the restated intensity sample and joint sums
against the dense restatement on the densified blocks; the BlockStore round trip with colours; tsdf_block_colors_to_dense; the
ValueErrors; the symbols and the Python surface; and the recorded outcome (tests/golden/htsdf_color_outcome.json)."""
import ctypes
import inspect
import json
import os
import re
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_color_outcome_fixture as HCO
import htsdf_color_restatement as HCR
import htsdf_restatement as HR
import sdf_color_restatement as SC
import tsdf_color_restatement as TC
import tsdf_restatement as TS
from icp_amd.synth import wavy_depth
from support import same_bits, pose_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def colour_frame(w, h, k=0):
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.ascontiguousarray(np.stack([(37 * u + 11 * v + 5 * k) % 256, (91 * u + 53 * v + 17 * k + 128) % 256, (29 * u + 113 * v + 64) % 256,
                                          (u * 7 + v * 13) % 255 + 1], -1).reshape(-1, 4).astype(np.uint8))


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fused():
    """Three coloured frames fused by both restatements over HC.BOX: the hashed one into pre-allocated blocks, the dense one into the box.
    Computed once and left unchanged."""
    _, rcam = HC.camera()
    hv = HCR.add_color(HR.HVolume(**HC.BOX))
    nb = tuple(d // 8 for d in HC.BOX_DIMS)
    hv.allocate(HC.box_coords((0, 0, 0), nb))
    dv = TC.add_color(TS.Volume(dims=HC.BOX_DIMS, **HC.BOX))
    counts = []
    for k, (depth, pose) in enumerate(zip(HC.frames(), HC.POSES)):
        rgbx = colour_frame(HC.W, HC.H, k)
        counts.append((HCR.integrate_color_allocated(hv, depth, rgbx, rcam, pose), TC.integrate_color(dv, depth, rgbx, rcam, pose)))
    return hv, dv, rcam, counts


def test_restated_fusion_equals_the_dense_restatement(fused):
    """Voxel for voxel: the blocks' four arrays, densified, are the dense restatement's, and both counts agree per frame."""
    from icp_amd import binding
    hv, dv, _, counts = fused
    for h, d in counts:
        assert h == d and h[0] > h[1] > 500
    coords, t, w = hv.sorted_blocks()
    rgb, cw = HCR.sorted_colors(hv)
    T, W = binding.tsdf_blocks_to_dense(coords, t, w, (0, 0, 0), HC.BOX_DIMS)
    Cd, Wc = binding.tsdf_block_colors_to_dense(coords, rgb, cw, (0, 0, 0), HC.BOX_DIMS)
    assert same_bits(T, dv.tsdf) and same_bits(W, dv.weight) and same_bits(Cd, dv.rgb) and same_bits(Wc, dv.wc)
    assert dv.wc.max() == 3 and ((dv.weight == 3) & (dv.wc < 3)).any()


def test_restated_sample_and_sums_equal_the_dense_restatement(fused):
    """The intensity sample (validity exactly, values bit for bit) and the 29 sums and three counts of a joint step, hashed restatement
    against dense restatement on the densified blocks; inside the box both read the same voxels."""
    hv, dv, rcam64, _ = fused
    rng = np.random.default_rng(7)
    o, s = np.asarray(HC.BOX["origin"], f32), f32(HC.BOX["voxel_size"])
    pts = (o + rng.uniform(0.0, 46.9, (5000, 3)).astype(f32) * s).astype(f32)
    a, b = HCR.sample_color(hv, pts), SC.sample_color(dv, pts)
    assert np.array_equal(a[2], b[2]) and same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and 50 < a[2].sum() < 5000
    from icp_amd.synth import tum_K
    rcam = TS.Camera(tum_K(40), 40, 30)
    depth = HC.crafted_frame(40, 30); rgbx = colour_frame(40, 30, 3)
    for pose in (np.eye(4, dtype=f32), pose_of((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))):
        for kw in (dict(stride=1), dict(stride=3, huber=0.05, color_huber=0.1)):
            ca, sa, _ = HCR.system(hv, depth, rgbx, rcam, pose, weight=0.1, **kw)
            cb, sb, _ = SC.system(dv, depth, rgbx, rcam, pose, weight=0.1, **kw)
            assert ca == cb and np.array_equal(u64(sa), u64(sb)) and ca[2] > 30, (kw, ca, cb)
    # a block that does not exist makes the sample invalid, as an uncoloured voxel does
    gone = HCR.add_color(HR.HVolume(**HC.BOX))
    gone.blocks = dict(hv.blocks); gone.colors = dict(hv.colors)
    q = pts[np.nonzero(a[2])[0][0]]
    b0 = tuple(int(x) for x in (np.floor((q - o) / s).astype(int) >> 3))
    del gone.blocks[b0]; del gone.colors[b0]
    assert HCR.sample_color(gone, q[None])[2][0] == 0 and HCR.sample_color(hv, q[None])[2][0] == 1


def test_block_colors_to_dense():
    from icp_amd import binding
    rng = np.random.default_rng(3)
    coords = np.array([[0, 0, 0], [1, 0, 0], [-1, 2, 1]], np.int32)
    rgb = rng.uniform(0, 255, (3, 8, 8, 8, 3)).astype(f32); cw = rng.integers(1, 4, (3, 8, 8, 8)).astype(f32)
    lo = np.array([-8, 0, 0]); dims = (24, 24, 12)
    Cd, W = binding.tsdf_block_colors_to_dense(coords, rgb, cw, lo, dims)
    assert Cd.shape == (12, 24, 24, 3) and W.shape == (12, 24, 24)
    assert same_bits(Cd[0:8, 0:8, 8:16], rgb[0]) and same_bits(W[0:8, 0:8, 16:24], cw[1])
    assert same_bits(Cd[8:12, 16:24, 0:8], rgb[2][:4]) and same_bits(W[8:12, 16:24, 0:8], cw[2][:4])      # cut at dims
    assert W.sum() == cw[0].sum() + cw[1].sum() + cw[2][:4].sum() and not Cd[0:8, 8:16].any()
    with pytest.raises(ValueError):
        binding.tsdf_block_colors_to_dense(coords, rgb[:2], cw, lo, dims)


def test_block_store_round_trip_with_colors():
    from icp_amd import tsdf_local
    rng = np.random.default_rng(11)
    coords = HC.box_coords((-2, -2, -2), (4, 4, 4))
    n = len(coords)
    arrs = (rng.uniform(-1, 1, (n, 8, 8, 8)).astype(f32), rng.integers(0, 4, (n, 8, 8, 8)).astype(f32),
            rng.uniform(0, 255, (n, 8, 8, 8, 3)).astype(f32), rng.integers(0, 3, (n, 8, 8, 8)).astype(f32))
    store = tsdf_local.BlockStore()
    assert store.colored is None and len(store.blocks()) == 3
    perm = rng.permutation(n)
    store.add(coords[perm], *[a[perm] for a in arrs])
    assert store.colored is True and len(store) == n and store.nbytes == n * 12288
    got = store.blocks()
    assert len(got) == 5 and np.array_equal(got[0], coords) and all(same_bits(g, a) for g, a in zip(got[1:], arrs))
    centre = np.array(HC.BOX["origin"], f32)
    taken = store.take_within(centre, 1.0, HC.BOX["origin"], HC.BOX["voxel_size"])
    keep = tsdf_local.block_centres_kept(coords, centre, 1.0, HC.BOX["origin"], HC.BOX["voxel_size"])
    assert 0 < keep.sum() < n and np.array_equal(taken[0], coords[keep]) and all(same_bits(g, a[keep]) for g, a in zip(taken[1:], arrs))
    assert len(store) == n - keep.sum() and len(store.take_within(centre, 0.0, HC.BOX["origin"], HC.BOX["voxel_size"])) == 5
    with pytest.raises(KeyError):
        store.add(coords[~keep][:1], *[a[~keep][:1] for a in arrs])
    with pytest.raises(ValueError):
        store.add(coords[keep][:1], arrs[0][keep][:1], arrs[1][keep][:1])               # blocks without colours into a coloured store
    with pytest.raises(ValueError):
        store.add(coords[keep][:1], arrs[0][keep][:1], arrs[1][keep][:1], rgb=arrs[2][keep][:1])
    plain = tsdf_local.BlockStore()
    plain.add(coords[:2], arrs[0][:2], arrs[1][:2])
    assert plain.colored is False and plain.nbytes == 2 * 4096 and len(plain.blocks()) == 3
    with pytest.raises(ValueError):
        plain.add(coords[2:3], *[a[2:3] for a in arrs])


def test_value_errors_symbols_and_python_surface():
    from icp_amd import binding, tsdf_local, tum
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    new = ("icp_tsdf_create_color_hashed", "icp_tsdf_hashed_has_color", "icp_get_tsdf_color_hashed", "icp_tsdf_upload_color_hashed", "icp_tsdf_evicted_blocks_color",
           "icp_tsdf_insert_blocks_color")
    for sym in new:
        assert sym in binding.EXPORTS and hasattr(lib, sym) and re.search(r"^int %s\(icp_ctx\* ctx" % sym, hdr, flags=re.M), sym
    o = binding.tsdf_options(origin=(0, 0, 0))
    assert lib.icp_tsdf_create_color_hashed(None, ctypes.byref(o), 16) == 1 and lib.icp_tsdf_hashed_has_color(None, None) == 1
    assert lib.icp_get_tsdf_color_hashed(None, None, 0, None, None, None, None, None) == 1 and lib.icp_tsdf_upload_color_hashed(None, 0, None, None, None, None, None) == 1
    assert lib.icp_tsdf_evicted_blocks_color(None, 0, None, None, None, None, None) == 1 and lib.icp_tsdf_insert_blocks_color(None, 0, None, None, None, None, None, None) == 1
    assert ctypes.sizeof(binding.IcpTsdfHashedInfo) == 24                   # (keeps its layout)
    assert inspect.signature(binding.Context.tsdf_create_hashed).parameters["color"].default is False
    assert inspect.signature(binding.Context.tsdf_blocks).parameters["colors"].default is False
    assert list(inspect.signature(binding.Context.tsdf_upload_blocks).parameters) == ["self", "coords", "tsdf", "weight", "rgb", "cweight"]
    assert list(inspect.signature(binding.Context.tsdf_evict_blocks_color).parameters) == ["self", "centre", "radius", "hold"]
    assert list(inspect.signature(binding.Context.tsdf_insert_blocks_color).parameters) == ["self", "coords", "tsdf", "weight", "rgb", "cweight"]
    assert hasattr(binding.Context, "tsdf_has_color") and "tsdf_view_reach" in dir(binding)
    par = inspect.signature(tsdf_local.track_depth_sdf_local).parameters
    assert par["rgbx_frames"].default is None and par["color_weight"].default == 0.0
    assert "colour" in binding.tsdf_view_reach.__doc__ and "6zb" in tum.track.__doc__
    # the ValueErrors of tum.track, raised before the context is touched
    seq = dict(K=np.eye(3, dtype=f32), width=4, height=4, depth=np.zeros((1, 4, 4), f32), rgbx=np.zeros((1, 16, 4), np.uint8), gt=None)
    model = dict(hashed=True, origin=(0, 0, 0), voxel_size=0.1)
    with pytest.raises(ValueError, match="coloured model"):
        tum.track(None, seq, model=model, sdf=dict(color_weight=0.1))              # color_weight > 0 on an uncoloured hashed model
    with pytest.raises(ValueError, match="reads no colours"):
        tum.track(None, seq, model=dict(model, color=True, raycast=True))          # color=True with raycast=True
    with pytest.raises(ValueError, match="colour frames"):
        tum.track(None, dict(seq, rgbx=None), model=dict(model, color=True), sdf={})
    with pytest.raises(ValueError):
        tum.track(None, seq, model=dict(model, color=True, keep_radius=3.0, raycast=True))


def test_recorded_outcome_separates_the_two_trackers():
    """tests/golden/htsdf_color_outcome.json, written by tests/htsdf_color_outcome_fixture.py on the CPU: the coloured hashed restatement
    stays within 0.0018 m over the 0.11 m of travel, the geometric one ends 0.088 m off -- the condition the fixture script asserts."""
    with open(HCO.GOLDEN) as f:
        ref = json.load(f)
    travel = ref["lateral_travel_m"]
    assert ref["stride"] == HCO.OPTIONS["stride"] and ref["n_iterations"] == HCO.OPTIONS["n_iterations"] and ref["weight"] == HCO.COLOR_OPTIONS["weight"]
    assert ref["frames"] == 12 and (ref["width"], ref["height"]) == (160, 120) and ref["colored_statuses"] == [0]
    assert 2 * ref["colored_worst_translation_m"] < travel / 2 < ref["geometric_last_translation_m"]
    assert len(ref["colored_iterations"]) == 11 and max(ref["colored_iterations"]) < 20
