"""The coloured hashed TSDF volume on the device (icp_tsdf_create_color_hashed and the coloured calls that work on either storage;
DESIGN.md section 6zb) against the numpy restatement (tests/htsdf_color_restatement.py) and against the dense coloured volume: colour
fusion voxel for voxel, growth, save and restore, the intensity sample in every class of cell, the sums of a joint step, the tracking loop
against a composition of public calls, streaming with colours, the outcome on the textured wall, and the refusals."""
import ctypes as C
import json
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_color_outcome_fixture as HCO
import htsdf_color_restatement as HCR
import htsdf_evict_fixture as EF
import htsdf_evict_restatement as ER
import htsdf_restatement as HR
import sdf_color_restatement as SC
import tsdf_color_outcome_fixture as CF
import tsdf_color_restatement as TC
import tsdf_restatement as TS
from icp_amd.synth import camera_sequence, wavy_depth
from support import same_bits, pose_of

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_SOURCE = 1, 4
INT_KEYS = ("n_depth", "n_valid_first", "n_valid_last", "n_color_first", "n_color_last", "iterations", "status")
F64_KEYS = ("cost_first", "cost_last", "cost_color_first", "cost_color_last")


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_record(a, b):
    return set(a) == set(b) and all(a[k] == b[k] for k in INT_KEYS) and all(u64(a[k]) == u64(b[k]) for k in F64_KEYS) and same_bits(a["pose"], b["pose"])


def same_cblocks(a, b):
    """Two (coords, tsdf, weight, rgb, cweight) in icp_get_tsdf_color_hashed's layout, bit for bit."""
    return np.array_equal(a[0], b[0]) and all(same_bits(x, y) for x, y in zip(a[1:5], b[1:5]))


def crafted_rgbx(w=HC.W, h=HC.H, k=0):
    """A colour frame whose neighbouring pixels differ in every channel (odd multipliers mod 256), with bytes 0 and 255 present, and a
    fourth byte that is junk and never zero: a kernel that reads it shows."""
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    r = (37 * u + 11 * v + 5 * k) % 256; g = (91 * u + 53 * v + 17 * k + 128) % 256; b = (29 * u + 113 * v + 71 * k + 64) % 256
    x = ((u * 7 + v * 13 + k) % 255) + 1
    out = np.stack([r, g, b, x], -1).reshape(-1, 4).astype(np.uint8)
    out[3, :3] = (0, 255, 0); out[w + 5, :3] = (255, 0, 255)
    assert (out[:, 3] != 0).all() and (np.diff(out[:, :3].reshape(h, w, 3).astype(int), axis=1) != 0).all()
    return np.ascontiguousarray(out)


def rgbx_frames():
    return [crafted_rgbx(k=k) for k in range(3)]


def sort5(coords, *arrs):
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    order = np.lexsort((coords[:, 0], coords[:, 1], coords[:, 2]))
    return (coords[order],) + tuple(np.asarray(a, f32)[order] for a in arrs)


def assert_equals_restatement(ctx, hv, what):
    info, coords, t, w, rgb, cw = ctx.tsdf_blocks(colors=True)
    rc, rt, rw = hv.sorted_blocks()
    rrgb, rcw = HCR.sorted_colors(hv)
    assert info["n_blocks"] == len(rc) and info["n_unplaced"] == 0 and info["n_out_of_range"] == hv.n_out_of_range, (what, info, len(rc))
    assert same_cblocks((coords, t, w, rgb, cw), (rc, rt, rw, rrgb, rcw)), what
    return info


# ---- 1. fusion equals the dense coloured volume
@pytest.mark.parametrize("case", ["box", "negative"])
def test_color_fusion_equals_the_dense_colored_volume(gpu_ctx_factory, case):
    """Three coloured frames into pre-allocated blocks and into a dense coloured volume over the same box: tsdf_blocks(colors=True) equals
    tsdf_volume() and tsdf_color_volume() bit for bit, n_updated and n_colored per frame are equal, and some voxel has geometry weight 3
    with Wc < 3 (updated in the free space in front of the band, where nothing is painted)."""
    from icp_amd import binding
    opts, lo, nb = (HC.BOX, (0, 0, 0), tuple(d // 8 for d in HC.BOX_DIMS)) if case == "box" else (HC.NEG, HC.NEG_LO, HC.NEG_BLOCKS)
    cam, _ = HC.camera()
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    h.tsdf_create_hashed(block_capacity=64, color=True, **opts)
    assert h.tsdf_has_color()
    box = HC.box_coords(lo, nb)
    h.tsdf_allocate_blocks(box)
    d.tsdf_create(color=True, **HC.dense_options(opts, lo, nb))
    for depth, rgbx, pose in zip(HC.frames(), rgbx_frames(), HC.POSES):
        nh = h.tsdf_integrate(depth, cam, pose, rgbx=rgbx); nd = d.tsdf_integrate(depth, cam, pose, rgbx=rgbx)
        print("integrate_color %s: %s voxels written / coloured (dense %s)" % (case, nh, nd))
        assert nh == nd and nh[0] > nh[1] > 500
    info, coords, t, w, rgb, cw = h.tsdf_blocks(colors=True)
    assert info["n_blocks"] == len(box) and np.array_equal(coords, box) and info["n_grown"] > 0
    dims = tuple(8 * n for n in nb)
    T, Wt = binding.tsdf_blocks_to_dense(coords, t, w, np.asarray(lo) * 8, dims)
    Cd, Wc = binding.tsdf_block_colors_to_dense(coords, rgb, cw, np.asarray(lo) * 8, dims)
    Td, Wd = d.tsdf_volume(); Cdd, Wcd = d.tsdf_color_volume()
    assert same_bits(T, Td) and same_bits(Wt, Wd) and same_bits(Cd, Cdd) and same_bits(Wc, Wcd)
    assert Wd.max() == 3 and Wcd.max() == 3 and ((Wd == 3) & (Wcd < 3)).any() and Cdd.max() > 200
    # geometry-only fusion on a coloured volume leaves the colours alone
    n = h.tsdf_integrate(HC.frames()[0], cam, HC.POSES[0])
    after = h.tsdf_blocks(colors=True)
    assert n > 1000 and after[3].max() == 4 and same_bits(after[4], rgb) and same_bits(after[5], cw)


# ---- 2. without pre-allocation
def test_color_fusion_without_preallocation_matches_restatement(gpu_ctx_factory):
    """Three coloured frames into an empty coloured hashed volume: blocks and all four arrays equal the restatement bit for bit after
    every frame, and so do both counts."""
    cam, rcam = HC.camera()
    for opts in (HC.STRADDLE, HC.NEG):
        ctx = gpu_ctx_factory()
        ctx.tsdf_create_hashed(color=True, **opts)
        hv = HCR.add_color(HR.HVolume(**opts))
        for k, (depth, rgbx, pose) in enumerate(zip(HC.frames(), rgbx_frames(), HC.POSES)):
            n = ctx.tsdf_integrate(depth, cam, pose, rgbx=rgbx)
            assert n == HCR.integrate_color(hv, depth, rgbx, rcam, pose), k
            info = assert_equals_restatement(ctx, hv, k)
        print("three coloured frames: %d blocks, last counts %s" % (info["n_blocks"], n))
        assert info["n_blocks"] > 40 and n[1] > 500
        ctx.tsdf_reset()
        i0, c0, *_ = ctx.tsdf_blocks(colors=True)
        assert i0["n_blocks"] == 0
        ctx.tsdf_allocate_blocks(info_coords := np.array(sorted(hv.blocks), np.int32)[:5])
        z = ctx.tsdf_blocks(colors=True)
        assert len(info_coords) == 5 and not z[4].any() and not z[5].any() and not z[2].any()      # reset cleared the colour pool too


# ---- 3. growth
def test_color_growth_from_one_block(gpu_ctx_factory):
    """block_capacity=1: after several growths over two coloured frames the blocks and colours equal those of a volume created with room."""
    cam, _ = HC.camera()
    small, roomy = gpu_ctx_factory(), gpu_ctx_factory()
    small.tsdf_create_hashed(block_capacity=1, color=True, **HC.STRADDLE)
    roomy.tsdf_create_hashed(block_capacity=1 << 10, color=True, **HC.STRADDLE)
    for depth, rgbx, pose in list(zip(HC.frames(), rgbx_frames(), HC.POSES))[:2]:
        assert small.tsdf_integrate(depth, cam, pose, rgbx=rgbx) == roomy.tsdf_integrate(depth, cam, pose, rgbx=rgbx)
    si, *sb = small.tsdf_blocks(colors=True); ri, *rb = roomy.tsdf_blocks(colors=True)
    print("coloured growth: %d blocks after %d growths, capacity %d" % (si["n_blocks"], si["n_grown"], si["capacity"]))
    assert same_cblocks(sb, rb) and si["n_grown"] >= 5 and ri["n_grown"] == 0 and sb[4].max() == 2
    small.tsdf_reserve_blocks(4 * si["capacity"])
    assert same_cblocks(small.tsdf_blocks(colors=True)[1:], rb)


# ---- 4. upload / download round trip
def test_color_upload_download_round_trip(gpu_ctx_factory):
    """0 blocks, 1 block, and 150 blocks into a pool of 2 that must grow: what comes back is what went in, sorted by key; the
    geometry-only upload on a coloured volume leaves cweight (and rgb) all zero; NULL outputs are honoured."""
    from icp_amd import binding
    rng = np.random.default_rng(5)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(block_capacity=2, color=True, **HC.STRADDLE)
    for n in (0, 1, 150):
        coords = (HC.box_coords((-3, -3, -3), (6, 6, 6))[rng.permutation(216)[:n]]).astype(np.int32)
        t = rng.uniform(-1, 1, (n, 8, 8, 8)).astype(f32); w = rng.integers(0, 4, (n, 8, 8, 8)).astype(f32)
        rgb = rng.uniform(0, 255, (n, 8, 8, 8, 3)).astype(f32); cw = rng.integers(0, 3, (n, 8, 8, 8)).astype(f32)
        rgb.view(np.uint32)[rng.random(rgb.shape) < 0.002] = 0x7FC54321
        ctx.tsdf_upload_blocks(coords, t, w, rgb, cw)
        info, *got = ctx.tsdf_blocks(colors=True)
        assert info["n_blocks"] == n and same_cblocks(got, sort5(coords, t, w, rgb, cw)), n
        assert same_cblocks(ctx.tsdf_blocks()[1:] + tuple(got[3:]), got)              # the geometry-only read agrees
    assert info["n_grown"] >= 1 and info["capacity"] >= 150      # (the pool of 2 had to grow for the 150)
    only = np.zeros((150, 8, 8, 8), f32)
    assert ctx.lib.icp_get_tsdf_color_hashed(ctx.h, None, 150, None, None, None, None, binding._ptr(only)) == 0 and same_bits(only, got[4])
    ctx.tsdf_upload_blocks(coords, t, w)
    info, *plain = ctx.tsdf_blocks(colors=True)
    assert same_cblocks(plain[:3] + [np.zeros_like(rgb), np.zeros_like(cw)], sort5(coords, t, w, np.zeros_like(rgb), np.zeros_like(cw)))
    assert not plain[3].any() and not plain[4].any()
    with pytest.raises(ValueError):
        ctx.tsdf_upload_blocks(coords, t, w, rgb=rgb)


# ---- 5. the intensity sample in every class of cell
def test_sample_color_in_every_class_of_cell(gpu_ctx_factory):
    """test_gpu_htsdf.py's construction with colours: a 4 x 4 x 4 box of blocks around the origin of a dyadic grid with ONE block missing,
    crafted colours, 2 % of the colour weights 0 -- and every geometry weight 0, which must play no part.  tsdf_sample_color on the hashed
    volume equals the dense call on a dense coloured volume uploaded from the blocks and the restatement: validity exactly, values bit
    for bit.  Classes: inside one block, across a face, an edge, a corner; cells at negative coordinates; exactly one corner's block
    missing; all eight blocks there but one corner with Wc == 0."""
    from icp_amd import binding
    opts = dict(origin=(0.5, -0.25, 1.0), voxel_size=0.125, truncation=0.375)
    rng = np.random.default_rng(19)
    lo_b = np.array([-2, -2, -2]); missing = (-1, 0, 0)
    box = HC.box_coords(lo_b, (4, 4, 4))
    coords = box[~(box == np.array(missing)).all(1)]
    t = rng.uniform(-1.5, 1.5, (63, 8, 8, 8)).astype(f32); w = np.zeros((63, 8, 8, 8), f32)
    rgb = rng.uniform(0, 255, (63, 8, 8, 8, 3)).astype(f32); cw = rng.choice(np.array([1, 2.5, 7], f32), (63, 8, 8, 8))
    cw[rng.random(cw.shape) < 0.02] = 0
    rgb.view(np.uint32)[rng.random(rgb.shape) < 0.002] = 0x7FC12345
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    h.tsdf_create_hashed(block_capacity=8, color=True, **opts)
    h.tsdf_upload_blocks(coords, t, w, rgb, cw)
    lo = lo_b * 8
    o, s = np.array(opts["origin"], f32), f32(0.125)
    d_origin = tuple(float(o[a] + f32(lo[a]) * s) for a in range(3))
    d.tsdf_create(dims=(32, 32, 32), origin=d_origin, voxel_size=0.125, truncation=0.375, color=True)
    d.tsdf_upload(*binding.tsdf_blocks_to_dense(coords, t, w, lo, (32, 32, 32)))
    d.tsdf_color_upload(*binding.tsdf_block_colors_to_dense(coords, rgb, cw, lo, (32, 32, 32)))
    hv = HCR.add_color(HR.HVolume(**opts))
    for c, tt, ww, cc, cww in zip(coords, t, w, rgb, cw):
        hv.blocks[tuple(int(x) for x in c)] = [tt, ww]; hv.colors[tuple(int(x) for x in c)] = [cc, cww]
    cells = [rng.integers(lo - 3, lo + 35, (6000, 3))]
    for n_cross in range(4):
        f = rng.integers(lo, lo + 32, (400, 3))
        f = (f & ~7) + rng.integers(0, 7, (400, 3))
        for i in range(400):
            f[i, rng.permutation(3)[:n_cross]] |= 7
        cells.append(f)
    m0 = np.array(missing) * 8
    around = np.array([[x, y, z] for x in (-1, 3, 7) for y in (-1, 3, 7) for z in (-1, 3, 7)]) + m0
    cells.append(np.repeat(around, 4, 0))
    cells = np.concatenate(cells)
    frac = rng.integers(0, 64, cells.shape).astype(f32) / f32(64)
    pts = (o + (cells.astype(f32) + frac) * s).astype(f32)
    assert np.array_equal(np.floor((pts - o) / s), cells.astype(f32))
    special = np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [3e6, 0, 1], [0, -3e6, 1], [0, 0, 1.1e6], [1.048570e6, 0, 1]], f32)
    pts = np.concatenate([pts, special]).astype(f32)
    S, Hh, ok = h.tsdf_sample_color(pts)
    Sd, Hd, okd = d.tsdf_sample_color(pts)
    Sr, Hr, okr = HCR.sample_color(hv, pts)
    assert np.array_equal(ok, okd) and same_bits(S, Sd) and same_bits(Hh, Hd)
    assert np.array_equal(ok.astype(bool), okr.astype(bool)) and same_bits(S, Sr) and same_bits(Hh, Hr)
    n = len(cells)
    okc = ok[:n].astype(bool)
    n_cross = ((cells & 7) == 7).sum(1)
    in_box = ((cells >= lo) & (cells + 1 < lo + 32)).all(1)
    for k in range(4):
        m = (n_cross == k) & in_box
        print("sample_color: %d cells across %d block boundaries, %d valid" % (m.sum(), k, okc[m].sum()))
        assert okc[m].sum() >= 30 and (~okc[m]).sum() >= 1, k
    blocks_of = lambda f: {tuple(((f + np.array([k & 1, (k >> 1) & 1, k >> 2])) >> 3).tolist()) for k in range(8)}
    have = {tuple(c) for c in coords.tolist()}
    one_missing = np.array([len(blocks_of(f) - have) == 1 and len(blocks_of(f)) > 1 for f in cells])
    assert one_missing.sum() >= 40 and not okc[one_missing].any() and {len(blocks_of(f)) for f in cells[one_missing]} == {2, 4, 8}
    # all eight blocks exist, exactly one corner uncoloured
    Cd, Wcd = binding.tsdf_block_colors_to_dense(coords, rgb, cw, lo, (32, 32, 32))
    all_there = np.array([blocks_of(f) <= have for f in cells])
    loc = cells - lo
    zero_corners = np.zeros(n, int)
    for k in range(8):
        j = loc + np.array([k & 1, (k >> 1) & 1, k >> 2])
        inside = ((j >= 0) & (j < 32)).all(1)
        jj = np.where(inside[:, None], j, 0)
        zero_corners += np.where(inside, Wcd[jj[:, 2], jj[:, 1], jj[:, 0]] == 0, 0)
    one_zero = all_there & in_box & (zero_corners == 1)
    print("sample_color: %d cells with one corner's block missing, %d with all blocks and one corner uncoloured, %d valid at negative coordinates"
          % (one_missing.sum(), one_zero.sum(), (okc & (cells < 0).all(1)).sum()))
    assert one_zero.sum() >= 40 and not okc[one_zero].any() and (n_cross[one_zero] > 0).any() and (n_cross[one_zero] == 0).any()
    assert (okc & (cells < 0).all(1)).sum() >= 20 and (okc & (cells >= 0).all(1)).sum() >= 20
    assert not ok[n:].any() and (S[~ok.astype(bool)] == 0).all() and np.isnan(S[ok.astype(bool)]).sum() > 0
    assert not h.tsdf_sample(pts)[2].any()                # (the geometry is unobserved everywhere: it played no part)


# ---- 6. the sums of one joint step
SHARES = []


def check_system(h, d, hv, cam, rcam, depth, rgbx, pose, what, stride=1, huber=0.0, color_huber=0.0, color_weight=0.1):
    kw = dict(rgbx=rgbx, stride=stride, huber=huber, color_weight=color_weight, color_huber=color_huber)
    sums, counts = h.tsdf_sdf_system(depth, cam, pose, **kw)
    dsums, dcounts = d.tsdf_sdf_system(depth, cam, pose, **kw)
    rcounts, rsums, rabs = HCR.system(hv, depth, rgbx, rcam, pose, stride=stride, huber=huber, weight=color_weight, color_huber=color_huber)
    bound = (rcounts[1] + rcounts[2]) * 2.0 ** -52 * rabs      # tests/test_gpu_sdf_color.py's bound
    err = np.abs(sums - rsums)
    share = float((err / np.maximum(bound, 1e-300)).max())
    SHARES.append(share)
    equal = np.array_equal(u64(sums), u64(dsums))
    print("system %s stride %d huber %g colour huber %g: counts %s, worst |sum - restatement| / bound = %.3g, bit-equal to the dense call: %s"
          % (what, stride, huber, color_huber, tuple(counts), share, equal))
    assert sums.shape == (29,) and tuple(counts) == tuple(dcounts) == tuple(rcounts), (what, counts, dcounts, rcounts)
    assert (err <= bound).all(), (what, err, bound)
    again, counts2 = h.tsdf_sdf_system(depth, cam, pose, **kw)
    assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts), what
    return counts, sums, equal


def test_color_system_matches_dense_and_restatement(gpu_ctx_factory):
    """The volume: two coloured frames fused on the device, all blocks at non-negative coordinates.  40 x 30 at strides 1 and 3, the
    geometric and the colour Huber off and on, two poses; 70 x 50 at stride 1 (partial tiles on both axes).  The three counts equal the
    dense call's (a dense coloured volume uploaded from the blocks) and the restatement's; the 29 sums are within
    tests/test_gpu_sdf_color.py's bound of the restatement's; two calls are bit-identical; bit-equality with the dense call is reported.
    color_weight=0 gives the geometric call's 28 sums."""
    from icp_amd import binding
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    cam64, rcam64 = HC.camera()
    h.tsdf_create_hashed(color=True, **HC.BOX)
    hv = HCR.add_color(HR.HVolume(**HC.BOX))
    for depth, rgbx, pose in list(zip(HC.frames(), rgbx_frames(), HC.POSES))[:2]:
        h.tsdf_integrate(depth, cam64, pose, rgbx=rgbx)
        HCR.integrate_color(hv, depth, rgbx, rcam64, pose)
    assert_equals_restatement(h, hv, "model")
    _, coords, t, w, rgb, cw = h.tsdf_blocks(colors=True)
    assert coords.min() >= 0 and (coords.max(0) < np.array(HC.BOX_DIMS) // 8).all()
    d.tsdf_create(color=True, dims=HC.BOX_DIMS, **HC.BOX)
    d.tsdf_upload(*binding.tsdf_blocks_to_dense(coords, t, w, (0, 0, 0), HC.BOX_DIMS))
    d.tsdf_color_upload(*binding.tsdf_block_colors_to_dense(coords, rgb, cw, (0, 0, 0), HC.BOX_DIMS))
    cam, rcam = HC.camera(40, 30)
    frame = HC.crafted_frame(40, 30); rgbx = crafted_rgbx(40, 30, 3)
    near = pose_of((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))
    equal = []
    for pose in (np.eye(4, dtype=f32), near):
        for stride in (1, 3):
            for huber in (0.0, 0.05):
                for color_huber in (0.0, 0.1):
                    counts, sums, eq = check_system(h, d, hv, cam, rcam, frame, rgbx, pose, "40 x 30", stride, huber, color_huber)
                    equal.append(eq)
                    if stride == 1:
                        assert 300 < counts[2] <= counts[1] <= counts[0] < 40 * 30 and 0 < sums[28] < sums[27]
    cam70, rcam70 = HC.camera(70, 50)
    counts, sums, eq = check_system(h, d, hv, cam70, rcam70, wavy_depth(70, 50), crafted_rgbx(70, 50, 4), near, "70 x 50")
    equal.append(eq)
    assert counts[2] > 1000
    print("colour system: %d of %d calls bit-equal to the dense volume's; worst share of the bound %.3g" % (sum(equal), len(equal), max(SHARES)))
    g, gc = h.tsdf_sdf_system(frame, cam, near, stride=1)
    z, zc = h.tsdf_sdf_system(frame, cam, near, rgbx=rgbx, stride=1, color_weight=0.0)
    assert np.array_equal(u64(g), u64(z)) and tuple(gc) == tuple(zc) and len(g) == 28


def test_color_system_in_every_class_of_cell(gpu_ctx_factory):
    """The joint step's cell of BOTH pools where it crosses a face, an edge and the corner: 2 x 2 x 2 blocks with crafted voxels and
    colours, a 16 x 16 frame (one work-group) behind a camera whose rays are one voxel apart at the frame's depth, pose identity -- pixel
    (u, w) falls into cell (u, w, 7 or 3), so column 7, row 7 and every other pixel's depth put local coordinate 7 on one, two and three
    axes, and column and row 15 reach for blocks that do not exist.  The frame as a whole and the pixels of each class alone (the rest
    MINF, so a class's terms cannot hide among the others'): check_system's comparisons with the dense call and the restatement."""
    from icp_amd import binding
    s = f32(1 / 64)
    opts = dict(origin=(float(-8.3 * s), float(-8.3 * s), float(4 - 7.4 * s)), voxel_size=float(s), truncation=float(3 * s), max_weight=64.0, min_depth=0.3, max_depth=4.5)
    rng = np.random.default_rng(23)
    coords = HC.box_coords((0, 0, 0), (2, 2, 2))
    t = rng.uniform(-0.9, 0.9, (8, 8, 8, 8)).astype(f32); w = np.ones((8, 8, 8, 8), f32)
    rgb = rng.uniform(0, 255, (8, 8, 8, 8, 3)).astype(f32); cw = rng.choice(np.array([1, 2.5, 7], f32), (8, 8, 8, 8))
    w[rng.random(w.shape) < 0.01] = 0; cw[rng.random(cw.shape) < 0.01] = 0
    for e, c in enumerate(coords):                            # the one cell across the corner, (7, 7, 7), is observed and coloured
        z, y, x = (7 if c[a] == 0 else 0 for a in (2, 1, 0))
        w[e, z, y, x] = 1; cw[e, z, y, x] = 2.5
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    h.tsdf_create_hashed(block_capacity=8, color=True, **opts)
    h.tsdf_upload_blocks(coords, t, w, rgb, cw)
    d.tsdf_create(color=True, dims=(16, 16, 16), **opts)
    d.tsdf_upload(*binding.tsdf_blocks_to_dense(coords, t, w, (0, 0, 0), (16, 16, 16)))
    d.tsdf_color_upload(*binding.tsdf_block_colors_to_dense(coords, rgb, cw, (0, 0, 0), (16, 16, 16)))
    hv = HCR.add_color(HR.HVolume(**opts))
    for c, tt, ww, cc, cww in zip(coords, t, w, rgb, cw):
        hv.blocks[tuple(int(x) for x in c)] = [tt, ww]; hv.colors[tuple(int(x) for x in c)] = [cc, cww]
    K = np.array([[256, 0, 8], [0, 256, 8], [0, 0, 1]], f32)
    cam, rcam = binding.depth_camera(K, 16, 16), TS.Camera(K, 16, 16)
    v, u = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    depth = np.where((u + v) % 2 == 0, f32(4), f32(4) - f32(4) * s).astype(f32)
    pts = np.stack([(u.astype(f32) - f32(8)) / f32(256) * depth, (v.astype(f32) - f32(8)) / f32(256) * depth, depth], -1).reshape(-1, 3).astype(f32)
    cells = np.floor((pts - np.array(opts["origin"], f32)) / s).astype(int)
    assert np.array_equal(cells, np.stack([u, v, np.where((u + v) % 2 == 0, 7, 3)], -1).reshape(-1, 3))
    n_cross = ((cells & 7) == 7).sum(1)
    ok = h.tsdf_sample(pts)[2].astype(bool)
    assert not ok[(cells[:, :2] == 15).any(1)].any()          # a corner's block is missing
    rgbx = crafted_rgbx(16, 16, 5)
    eye = np.eye(4, dtype=f32)
    frame = depth.copy(); frame[0, 1], frame[1, 0] = MINF, np.nan
    counts, sums, _ = check_system(h, d, hv, cam, rcam, frame, rgbx, eye, "16 x 16, every class", color_huber=0.1)
    assert counts[0] == 254 and 100 < counts[2] < counts[1] < 225
    for k in range(4):
        only = np.where((n_cross == k).reshape(16, 16), depth, MINF).astype(f32)
        counts, sums, _ = check_system(h, d, hv, cam, rcam, only, rgbx, eye, "16 x 16, cells across %d block boundaries" % k, huber=0.01 * k)
        assert counts[0] == (n_cross == k).sum() and counts[1] == (ok & (n_cross == k)).sum() and 0 < counts[2] <= counts[1] and sums[28] > 0, (k, counts)
    # (local coordinate 7 is also cell 15's: of the 4 cells across three boundaries only (7, 7, 7) has its eight blocks)
    assert [(ok & (n_cross == k)).sum() for k in range(4)] == [85, 104, 12, 1] and ok[(cells == 7).all(1)].all()


# ---- 7. align and loop
def python_loop(ctx, depth, cam, rgbx, **kw):
    """icp_track_depth_sdf_color as a composition of public calls (the volume exists)."""
    pose = np.eye(4, dtype=f32)
    ctx.tsdf_integrate(depth[0], cam, pose, rgbx=rgbx[0])
    recs = []
    for k in range(1, len(depth)):
        pose, rec, rc = ctx.tsdf_align_depth(depth[k], cam, pose, rgbx=rgbx[k], **kw)
        if rc == 0:
            ctx.tsdf_integrate(depth[k], cam, pose, rgbx=rgbx[k])
        recs.append(rec)
    return pose, recs


def test_track_depth_sdf_color_matches_composition_of_public_calls(gpu_ctx_factory):
    """5 frames of 40 x 30 of the synthetic room with their colour frames, frame 2 all MINF, on a coloured hashed volume that starts with
    16 blocks and grows in the loop: records, poses and the final blocks with colours, bit for bit.  The geometric loop given colour frames
    fuses them too."""
    from icp_amd import binding
    K, depth, rgbx, gt = camera_sequence(5, 40, 30)
    depth[2][:] = MINF
    cam = binding.depth_camera(K, 40, 30)
    opts = dict(origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
    a, b, g = gpu_ctx_factory(), gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b, g):
        c.tsdf_create_hashed(block_capacity=16, color=True, **opts)
    kw = dict(stride=1, n_iterations=12, color_weight=0.1, color_huber=0.2)
    pose, recs, rc = a.track_depth_sdf(depth, cam, rgbx_frames=rgbx, **kw)
    ref_pose, ref = python_loop(b, depth, cam, rgbx, **kw)
    print("track_depth_sdf_color (hashed): statuses %s, iterations %s, n_valid %s, n_color %s" % ([r["status"] for r in recs], [r["iterations"] for r in recs],
                                                                                                  [r["n_valid_last"] for r in recs], [r["n_color_last"] for r in recs]))
    assert len(recs) == 4 and rc == ERR_NO_SOURCE
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert same_record(r, h), (k, r, h)
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    assert [r["status"] for r in recs] == [0, ERR_NO_SOURCE, 0, 0] and same_bits(recs[1]["pose"], recs[0]["pose"])
    assert all(r["n_color_last"] > 100 for r in recs if r["status"] == 0)
    ai, *ab = a.tsdf_blocks(colors=True); bi, *bb = b.tsdf_blocks(colors=True)
    assert same_cblocks(ab, bb) and ab[2].max() == 4 and ab[4].max() == 4 and ai["n_grown"] == bi["n_grown"] > 0 and ai["n_unplaced"] == 0
    # icp_track_depth_sdf given colour frames fuses them: the geometric records, coloured blocks
    gpose, grecs, grc = g.track_depth_sdf(depth, cam, rgbx_frames=rgbx, stride=1, n_iterations=12)
    gb = g.tsdf_blocks(colors=True)
    assert grc == ERR_NO_SOURCE and "n_color_last" not in grecs[0] and gb[5].max() == 4 and gb[4].max() > 100


# ---- 8. streaming
CENTRE = (0.25, 0.15, 1.3)
RADIUS = 9.0
PATTERNS = ("all kept", "all evicted", "last evicted", "first evicted", "alternating")


@pytest.fixture(scope="module")
def scene(gpu_ctx_factory):
    """test_gpu_htsdf_evict.py's scene with colours: three coloured frames fused in HC.STRADDLE, then crafted filler blocks near (kept)
    and far (evicted).  Computed once and left unchanged: three lists of (coords, t, w, rgb, cw)."""
    ctx = gpu_ctx_factory()
    cam, _ = HC.camera()
    ctx.tsdf_create_hashed(color=True, **HC.STRADDLE)
    for depth, rgbx, pose in zip(HC.frames(), rgbx_frames(), HC.POSES):
        ctx.tsdf_integrate(depth, cam, pose, rgbx=rgbx)
    _, sc, st, sw, srgb, scw = ctx.tsdf_blocks(colors=True)
    ctx.tsdf_release()
    have = {tuple(b) for b in sc.tolist()}
    rng = np.random.default_rng(29)
    near = [b for b in HC.box_coords((-5, -5, -5), (10, 10, 10)).tolist() if tuple(b) not in have][:300]
    far = (HC.box_coords((-5, -5, -5), (10, 10, 10))[:300] + np.array([100, 0, 0])).tolist()
    k = ER.kept(np.array(near + far), HC.STRADDLE["origin"], HC.STRADDLE["voxel_size"], CENTRE, RADIUS)
    assert k[:len(near)].all() and not k[len(near):].any()
    assert ER.kept(sc, HC.STRADDLE["origin"], HC.STRADDLE["voxel_size"], CENTRE, RADIUS).all()

    def crafted(n):
        cw = rng.integers(1, 3, (n, 8, 8, 8)).astype(f32)
        cw[rng.random(cw.shape) < 0.02] = 0               # (mostly coloured, so that most colour samples in the filler are valid)
        return (rng.uniform(-1, 1, (n, 8, 8, 8)).astype(f32), rng.integers(0, 4, (n, 8, 8, 8)).astype(f32), rng.uniform(0, 255, (n, 8, 8, 8, 3)).astype(f32), cw)
    blocks = lambda cc, arrs: [(tuple(c),) + tuple(a[i] for a in arrs) for i, c in enumerate(cc)]
    return blocks(sc.tolist(), (st, sw, srgb, scw)), blocks(near, crafted(len(near))), blocks(far, crafted(len(far)))


def pool_layout(scene, n, pattern):
    sc, near, far = scene
    if pattern == "all kept":
        keep = np.ones(n, bool)
    elif pattern == "all evicted":
        keep = np.zeros(n, bool)
    elif pattern == "last evicted":
        keep = np.arange(n) < n - max(1, n // 3)
    elif pattern == "first evicted":
        keep = np.arange(n) >= max(1, n // 3)
    else:
        keep = np.arange(n) % 2 == 1
    kept_src = iter(sc + near); gone_src = iter(far)
    return [next(kept_src) if k else next(gone_src) for k in keep], keep


def sample_points(kept_coords, rng):
    o, s = np.array(HC.STRADDLE["origin"], f32), f32(HC.STRADDLE["voxel_size"])
    if len(kept_coords) == 0:
        kept_coords = np.zeros((1, 3), np.int32)
    base = kept_coords[rng.integers(0, len(kept_coords), 400)].astype(np.int64) * 8
    cells = base + rng.integers(0, 7, (400, 3))
    for i in range(400):
        cells[i, rng.permutation(3)[:i % 4]] |= 7
    frac = rng.integers(0, 64, cells.shape).astype(f32) / f32(64)
    return (o + (cells.astype(f32) + frac) * s).astype(f32)


def pack(layout, keep, want):
    sel = [b for b, k in zip(layout, keep) if k == want]
    shapes = ((3,), (8, 8, 8), (8, 8, 8), (8, 8, 8, 3), (8, 8, 8))
    return sort5(*[np.array([b[j] for b in sel]).reshape((-1,) + s) for j, s in enumerate(shapes)])


def assert_same_colored_state(a, b, what):
    """Blocks with colours, the intensity sample, the colour sums and one more coloured integrate: identical bits on both contexts."""
    cam, _ = HC.camera()
    ai, *ab = a.tsdf_blocks(colors=True); bi, *bb = b.tsdf_blocks(colors=True)
    assert same_cblocks(ab, bb) and ai["n_blocks"] == bi["n_blocks"] and ai["n_unplaced"] == bi["n_unplaced"] == 0, what
    pts = sample_points(ab[0], np.random.default_rng(3))
    fa, fb = a.tsdf_sample_color(pts), b.tsdf_sample_color(pts)
    assert same_bits(fa[0], fb[0]) and same_bits(fa[1], fb[1]) and np.array_equal(fa[2], fb[2]), what
    ga, gb = a.tsdf_sample(pts), b.tsdf_sample(pts)
    assert same_bits(ga[0], gb[0]) and np.array_equal(ga[2], gb[2]), what
    frame, rgbx = HC.crafted_frame(), crafted_rgbx(k=7)
    for stride in (1, 3):
        sa, ca = a.tsdf_sdf_system(frame, cam, HC.TILTED, rgbx=rgbx, color_weight=0.1, stride=stride)
        sb, cb = b.tsdf_sdf_system(frame, cam, HC.TILTED, rgbx=rgbx, color_weight=0.1, stride=stride)
        assert np.array_equal(u64(sa), u64(sb)) and tuple(ca) == tuple(cb), what
    na = a.tsdf_integrate(wavy_depth(HC.W, HC.H, 1.4), cam, HC.POSES[2], rgbx=rgbx); nb = b.tsdf_integrate(wavy_depth(HC.W, HC.H, 1.4), cam, HC.POSES[2], rgbx=rgbx)
    assert na == nb and same_cblocks(a.tsdf_blocks(colors=True)[1:], b.tsdf_blocks(colors=True)[1:]), what
    return int(fa[2].sum()), ca


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_color_evict_equals_a_fresh_upload_of_the_kept_blocks(gpu_ctx_factory, scene, n):
    """test_gpu_htsdf_evict.py's identity with colours, over its five patterns: after the evict the context equals a fresh coloured one
    that tsdf_upload_blocks(..., rgb, cweight) filled with the kept blocks -- blocks with colours, tsdf_sample_color, the colour sums and
    one more coloured integrate, bit for bit; the outbox holds the evicted blocks with their colours; the geometry-only outbox call agrees."""
    ctx, ref = gpu_ctx_factory(), gpu_ctx_factory()
    for pattern in PATTERNS:
        layout, keep = pool_layout(scene, n, pattern)
        ctx.tsdf_create_hashed(block_capacity=16, color=True, **HC.STRADDLE)
        for c, t, w, rgb, cw in layout:
            ctx.tsdf_insert_blocks_color([c], t[None], w[None], rgb[None], cw[None])
        assert ctx.tsdf_blocks()[0]["n_blocks"] == n
        info, *ev = ctx.tsdf_evict_blocks_color(CENTRE, RADIUS)
        n_keep = int(keep.sum())
        kept, gone = pack(layout, keep, True), pack(layout, keep, False)
        assert info["n_evicted"] == n - n_keep == info["n_held"] and info["n_blocks"] == n_keep, (pattern, info)
        assert info["n_moved"] == (int(keep[n_keep:].sum()) if n_keep < n else 0), (pattern, info)
        assert same_cblocks(ev, gone), pattern
        c2 = np.zeros_like(ev[0]); t2 = np.zeros_like(ev[1]); w2 = np.zeros_like(ev[2])
        if len(c2):
            from icp_amd import binding
            assert ctx.lib.icp_tsdf_evicted_blocks(ctx.h, len(c2), binding._ptr(c2), binding._ptr(t2), binding._ptr(w2)) == 0
            assert np.array_equal(c2, ev[0]) and same_bits(t2, ev[1]) and same_bits(w2, ev[2]), pattern
        ref.tsdf_create_hashed(block_capacity=16, color=True, **HC.STRADDLE)
        ref.tsdf_upload_blocks(*kept)
        valid, counts = assert_same_colored_state(ctx, ref, (n, pattern))
        print("n %d, %s: %d evicted, %d moved; %d valid colour samples, counts %s" % (n, pattern, info["n_evicted"], info["n_moved"], valid, tuple(counts)))
        if n >= 64 and pattern != "all evicted":
            assert valid > 20
        if n >= 257 and pattern == "all kept":
            assert counts[2] > 0                            # (the whole scene is among the kept blocks: some pixel has a colour row)


def test_color_clean_tail_and_insert(gpu_ctx_factory):
    """Evict, then a coloured frame that allocates evicted keys again: blocks and colours equal the restatement's (an evicted key holds
    what ONE frame paints, not its old colours), also after a growth.  Insert with colours puts the evicted blocks back bit for bit,
    refuses a resident key with nothing modified, and the geometry-only insert leaves the new blocks uncoloured."""
    from icp_amd import binding
    cam, rcam = HC.camera()
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(block_capacity=64, color=True, **HC.STRADDLE)
    hv = HCR.add_color(HR.HVolume(**HC.STRADDLE))
    fr = list(zip(HC.frames(), rgbx_frames(), HC.POSES))
    for depth, rgbx, pose in fr[:2]:
        ctx.tsdf_integrate(depth, cam, pose, rgbx=rgbx); HCR.integrate_color(hv, depth, rgbx, rcam, pose)
    binfo, *before = ctx.tsdf_blocks(colors=True)
    info, *ev = ctx.tsdf_evict_blocks_color(CENTRE, 1.0)
    n_ev, out = ER.evict(hv, CENTRE, 1.0)
    HCR.drop_colors(hv)
    assert 5 < info["n_evicted"] == n_ev < binfo["n_blocks"] - 5 and ev[3].any()
    kept = ctx.tsdf_blocks(colors=True)[1:]
    assert_equals_restatement(ctx, hv, "after the evict")
    # a resident key refuses the coloured insert: nothing modified
    mixed = np.concatenate([ev[0][:4], kept[0][:3]])
    z = np.zeros((7, 8, 8, 8), f32); z3 = np.zeros((7, 8, 8, 8, 3), f32)
    st = binding.IcpTsdfStreamInfo()
    P = binding._ptr
    rc = ctx.lib.icp_tsdf_insert_blocks_color(ctx.h, 7, P(mixed), P(z), P(z), P(z3), P(z), C.byref(st))
    msg = ctx.lib.icp_last_error(ctx.h).decode()
    assert rc == ERR_INVALID_ARG and st.n_present == 3 and "3 of the 7" in msg and "icp_tsdf_insert_blocks_color" in msg, (rc, msg)
    assert same_cblocks(ctx.tsdf_blocks(colors=True)[1:], kept)
    # the clean tail: the next coloured frame allocates evicted keys again, in a pool that grows
    ctx.tsdf_reserve_blocks(4 * info["capacity"])
    depth, rgbx, pose = fr[2]
    assert ctx.tsdf_integrate(depth, cam, pose, rgbx=rgbx) == HCR.integrate_color(hv, depth, rgbx, rcam, pose)
    assert_equals_restatement(ctx, hv, "after the next frame")
    back = set(out) & set(hv.blocks)
    assert len(back) >= 1 and all(hv.colors[b][1].max() <= 1 for b in back if b in hv.colors)
    # insert with colours: the evicted blocks back beside the kept ones, the original volume bit for bit
    back_ctx = gpu_ctx_factory()
    back_ctx.tsdf_create_hashed(block_capacity=2, color=True, **HC.STRADDLE)
    back_ctx.tsdf_insert_blocks_color(*kept)
    iinfo = back_ctx.tsdf_insert_blocks_color(*[a[::-1] for a in ev])
    assert iinfo["n_inserted"] == n_ev and iinfo["n_grown"] >= 4 and same_cblocks(back_ctx.tsdf_blocks(colors=True)[1:], before)
    # the geometry-only insert on a coloured volume: the new blocks uncoloured, the others untouched
    plain = gpu_ctx_factory()
    plain.tsdf_create_hashed(block_capacity=64, color=True, **HC.STRADDLE)
    plain.tsdf_insert_blocks_color(*kept)
    plain.tsdf_insert_blocks(*ev[:3])
    got = dict(zip(map(tuple, plain.tsdf_blocks(colors=True)[1].tolist()), range(10 ** 6)))
    pb = plain.tsdf_blocks(colors=True)
    for c in ev[0].tolist():
        i = got[tuple(c)]
        assert not pb[4][i].any() and not pb[5][i].any()
    assert same_cblocks([a[[got[tuple(c)] for c in kept[0].tolist()]] for a in pb[1:]], kept) and kept[4].any()


def wall_colors(K, depth, poses):
    """Colour frames for tests/htsdf_evict_fixture.py's slide: a smooth texture of the world point every pixel sees (so the photometric
    term agrees with the motion), junk in the fourth byte."""
    out = []
    h, w = depth[0].shape
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    a = (u - float(K[0, 2])) / float(K[0, 0]); b = (v - float(K[1, 2])) / float(K[1, 1])
    for d, T in zip(depth, poses):
        x = float(T[0, 3]) + a * d; y = b * d
        r = 128 + 100 * np.sin(5.0 * x + 1.3 * y); g = 128 + 90 * np.cos(4.1 * y - 2.2 * x); bl = 128 + 80 * np.sin(3.3 * x + 4.7 * y + 1.0)
        f = np.stack([r, g, bl, np.full_like(r, 77)], -1).reshape(-1, 4)
        out.append(np.clip(np.floor(f + 0.5), 0, 255).astype(np.uint8))
    return np.stack(out)


def test_local_colored_loop_matches_the_unbounded_one(gpu_ctx_factory):
    """The out-and-back slide of tests/htsdf_evict_fixture.py with colour frames, keep_radius = reach + twice the step: the local coloured
    loop's poses and records equal the unbounded coloured loop's bit for bit, `restore` gives its blocks with colours bit for bit, and the
    store and the device never hold the same block."""
    from icp_amd import binding, tsdf_local
    K, depth, poses = EF.frames()
    rgbx = wall_colors(K, depth, poses)
    cam = binding.depth_camera(K, EF.W, EF.H)
    keep = EF.model()["keep_radius"]
    kw = dict(color_weight=0.1, **EF.OPTIONS)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.tsdf_create_hashed(block_capacity=16, color=True, **EF.VOLUME)
    pose, recs, rc = a.track_depth_sdf(depth, cam, rgbx_frames=rgbx, **kw)
    lpose, lrecs, lrc, evs, store = tsdf_local.track_depth_sdf_local(b, depth, cam, keep, rgbx_frames=rgbx, **kw)
    peak = max(e["n_resident"] + e["n_evicted"] for e in evs)
    total = a.tsdf_blocks()[0]["n_blocks"]
    print("local coloured loop: evicted %d, inserted %d in all, peak %d of %d blocks; n_color %s" %
          (sum(e["n_evicted"] for e in evs), sum(e["n_inserted"] for e in evs), peak, total, [r["n_color_last"] for r in recs][:6]))
    assert rc == lrc == 0 and same_bits(pose, lpose) and len(recs) == len(lrecs) == len(depth) - 1
    for k, (r, h) in enumerate(zip(recs, lrecs)):
        assert same_record(r, h), (k, r, h)
    assert sum(e["n_evicted"] for e in evs) > 50 and sum(e["n_inserted"] for e in evs) > 50 and peak < total and store.colored
    assert all(r["n_color_last"] > 100 for r in recs)
    resident = {tuple(x) for x in b.tsdf_blocks()[1].tolist()}
    assert not (resident & {tuple(x) for x in store.blocks()[0].tolist()}) and len(resident) + len(store) == total
    assert tsdf_local.restore(b, store) == total
    assert same_cblocks(b.tsdf_blocks(colors=True)[1:], a.tsdf_blocks(colors=True)[1:]) and a.tsdf_blocks(colors=True)[5].max() > 1
    with pytest.raises(ValueError):
        plain = gpu_ctx_factory()
        plain.tsdf_create_hashed(**EF.VOLUME)
        tsdf_local.track_depth_sdf_local(plain, depth[:2], cam, keep, rgbx_frames=rgbx[:2])


# ---- 9. the outcome
def test_outcome_on_the_textured_wall_hashed(gpu_ctx_factory, tmp_path):
    """The textured wall of tests/tsdf_color_outcome_fixture.py (12 frames of 160 x 120, 1 cm of lateral travel per frame, 0.11 m in all)
    through tum.track with model=dict(hashed=True, color=True, ...) and sdf=dict(stride=2, n_iterations=20, color_weight=0.1), and through
    the geometric hashed loop.  Figures (translation error [m]):
      restatement, coloured (tests/golden/htsdf_color_outcome.json): worst 0.0018, last 0.0007, 3 - 5 iterations per frame, 75 blocks
      restatement, geometric: worst 0.0930, last 0.0883, all 20 iterations on 10 of 11 frames
      device: printed below next to the bounds
    Asked of the device: status 0 on every frame; the worst error within TWICE the golden's and every frame's iteration count within
    twice the golden's (the margin DESIGN.md section 6m gives a chain of frames; test_outcome_on_the_textured_wall applies the same); the
    geometric hashed loop ends more than half the travel away.  Then reconstruct_room(densify=True) writes a coloured mesh of the model."""
    from icp_amd import meshio, tum
    with open(HCO.GOLDEN) as f:
        ref = json.load(f)
    K, depth, rgbx, gt = CF.fixture()
    seq = dict(depth=depth, rgbx=rgbx, gt=gt, K=K, width=CF.W, height=CF.H, frames=list(range(len(depth))))
    ctx = gpu_ctx_factory()
    sdf = dict(color_weight=HCO.COLOR_OPTIONS["weight"], **HCO.OPTIONS)
    poses, recs, rc = tum.track(ctx, seq, with_gt=False, model=HCO.hashed_model(), sdf=sdf)
    err = CF.translation_errors([np.eye(4)] + [r["pose"] for r in recs], gt)
    its = [r["iterations"] for r in recs]
    print("golden: worst %.4f m, iterations %s; device coloured hashed loop: worst %.4f m (bound %.4f), last %.4f m, status %d, iterations %s, n_color %s, %d blocks"
          % (ref["colored_worst_translation_m"], ref["colored_iterations"], max(err), 2 * ref["colored_worst_translation_m"], err[-1], rc, its,
             [r["n_color_last"] for r in recs], ctx.tsdf_blocks()[0]["n_blocks"]))
    assert rc == 0 and all(r["status"] == 0 for r in recs) and len(recs) == CF.N_FRAMES - 1 and ctx.tsdf_has_color()
    assert max(err) <= 2 * ref["colored_worst_translation_m"]
    assert all(i <= 2 * j for i, j in zip(its, ref["colored_iterations"]))
    travel = ref["lateral_travel_m"]
    gctx = gpu_ctx_factory()
    gposes, grecs, grc = tum.track(gctx, seq, with_gt=False, model=HCO.hashed_model(color=False), sdf=dict(HCO.OPTIONS))
    gerr = CF.translation_errors([np.eye(4)] + [r["pose"] for r in grecs], gt)
    print("device geometric hashed loop: worst %.4f m, last %.4f m (golden %.4f / %.4f), iterations %s" % (max(gerr), gerr[-1], ref["geometric_worst_translation_m"],
                                                                                                           ref["geometric_last_translation_m"], [r["iterations"] for r in grecs]))
    assert grc == 0 and gerr[-1] > travel / 2
    # the densify route: a coloured mesh of the finished hashed model
    out = str(tmp_path / "out")
    _, _, rc2, paths = tum.reconstruct_room(ctx, seq, out_dir=out, with_gt=False, model=HCO.hashed_model(), sdf=sdf, model_mesh="m.ply")
    v, nr, t, col = ctx.tsdf_mesh(colors=True)
    assert rc2 == 0 and len(t) > 1000 and (col[:, 3] == 255).sum() > len(col) // 2 and len({tuple(c) for c in col[::50, :3].tolist()}) > 10
    assert len(meshio.load_ply_mesh(str(tmp_path / "out" / "m.ply"))[0]) == len(v)
    with pytest.raises(ValueError):
        tum.track(ctx, seq, model=dict(HCO.hashed_model(), raycast=True))


# ---- 10. refusals
def test_color_refusals_leave_the_blocks_alone(gpu_ctx_factory):
    """On a coloured hashed volume the calls without a block form (the coloured ray-cast, target, model loop and mesh, and the four calls
    on the dense colour array) return ICP_ERR_INVALID_ARG with a message naming the call and leave all four block arrays bit-identical;
    the new calls refuse no volume, a dense volume and an uncoloured hashed volume; the volume still works afterwards, and
    the geometry-only hashed calls stay legal on it."""
    from icp_amd import binding
    cam, _ = HC.camera()
    ctx = gpu_ctx_factory()
    lib, h = ctx.lib, ctx.h
    P, B = binding._ptr, C.byref
    n = HC.W * HC.H
    one = np.zeros((1, 3), np.int32); z = np.zeros((1, 8, 8, 8), f32); z3 = np.zeros((1, 8, 8, 8, 3), f32); i32 = C.c_int32(0); j32 = C.c_int32(0)
    new_calls = {
        "icp_tsdf_hashed_has_color": lambda: lib.icp_tsdf_hashed_has_color(h, B(i32)),
        "icp_get_tsdf_color_hashed": lambda: lib.icp_get_tsdf_color_hashed(h, None, 0, None, None, None, None, None),
        "icp_tsdf_upload_color_hashed": lambda: lib.icp_tsdf_upload_color_hashed(h, 1, P(one), P(z), P(z), P(z3), P(z)),
        "icp_tsdf_evicted_blocks_color": lambda: lib.icp_tsdf_evicted_blocks_color(h, 1, P(one), None, None, None, None),
        "icp_tsdf_insert_blocks_color": lambda: lib.icp_tsdf_insert_blocks_color(h, 1, P(one), P(z), P(z), P(z3), P(z), None),
    }
    for name, call in new_calls.items():
        assert call() == ERR_INVALID_ARG and "no volume" in lib.icp_last_error(h).decode() and name in lib.icp_last_error(h).decode(), name
    ctx.tsdf_create(dims=HC.BOX_DIMS, **HC.BOX)
    for name, call in new_calls.items():
        assert call() == ERR_INVALID_ARG and "dense" in lib.icp_last_error(h).decode() and name in lib.icp_last_error(h).decode(), name
    ctx.tsdf_create_hashed(**HC.BOX)
    assert not ctx.tsdf_has_color()
    for name, call in new_calls.items():
        if name != "icp_tsdf_hashed_has_color":
            assert call() == ERR_INVALID_ARG and "no colours" in lib.icp_last_error(h).decode() and name in lib.icp_last_error(h).decode(), name
    assert ctx.tsdf_blocks()[0]["n_blocks"] == 0
    # the coloured hashed volume
    ctx.tsdf_create_hashed(color=True, **HC.BOX)
    d = HC.crafted_frame(); rgbx1 = crafted_rgbx()
    ctx.tsdf_integrate(d, cam, np.eye(4, dtype=f32), rgbx=rgbx1)
    before = ctx.tsdf_blocks(colors=True)
    p = binding.pose_to_c(np.eye(4, dtype=f32)); buf = np.zeros(n * 4, f32)
    rgbx = np.zeros((2, n, 4), np.uint8); d2 = np.ascontiguousarray(np.stack([d, d]), f32)
    so = binding.depth_options(False, 2, fix_color_index=True); tf = (binding.IcpTrackFrame * 1)()
    R = P(rgbx)
    calls = {
        "icp_tsdf_raycast_color": lambda: lib.icp_tsdf_raycast_color(h, B(cam), P(p), P(buf), None, None, None, B(i32), B(j32)),
        "icp_set_target_tsdf_color": lambda: lib.icp_set_target_tsdf_color(h, B(cam), P(p), B(i32)),
        "icp_track_depth_model_color": lambda: lib.icp_track_depth_model_color(h, P(d2), R, C.c_int32(2), B(cam), B(so), None, P(p), tf),
        "icp_tsdf_mesh_color": lambda: lib.icp_tsdf_mesh_color(h, C.c_float(0), C.c_int32(0), C.c_int32(0), None, None, None, None, B(i32), B(j32)),
        "icp_tsdf_color_create": lambda: lib.icp_tsdf_color_create(h),
        "icp_tsdf_color_release": lambda: lib.icp_tsdf_color_release(h),
        "icp_tsdf_color_download": lambda: lib.icp_tsdf_color_download(h, P(buf), P(buf)),
        "icp_tsdf_color_upload": lambda: lib.icp_tsdf_color_upload(h, P(buf), P(buf)),
        "icp_tsdf_raycast": lambda: lib.icp_tsdf_raycast(h, B(cam), P(p), P(buf), None, None, B(i32)),
        "icp_tsdf_download": lambda: lib.icp_tsdf_download(h, P(buf), P(buf)),
    }
    for name, call in calls.items():
        rc = call()
        msg = lib.icp_last_error(h).decode()
        assert rc == ERR_INVALID_ARG and "hashed volume" in msg and name in msg, (name, rc, msg)
        if name.startswith("icp_tsdf_color_"):
            assert "icp_get_tsdf_color_hashed" in msg and "icp_tsdf_upload_color_hashed" in msg, msg      # points at the new calls
    after = ctx.tsdf_blocks(colors=True)
    assert after[0] == before[0] and same_cblocks(after[1:], before[1:])
    assert same_bits(binding.pose_from_c(p), np.eye(4, dtype=f32))
    # bad arguments of the new calls: nothing modified
    two = np.zeros((2, 3), np.int32); zz = np.zeros((2, 8, 8, 8), f32); zz3 = np.zeros((2, 8, 8, 8, 3), f32)
    assert lib.icp_tsdf_upload_color_hashed(h, 2, P(two), P(zz), P(zz), P(zz3), P(zz)) == ERR_INVALID_ARG and "twice" in lib.icp_last_error(h).decode()
    assert lib.icp_tsdf_upload_color_hashed(h, 1, P(one), P(z), P(z), None, P(z)) == ERR_INVALID_ARG
    assert lib.icp_get_tsdf_color_hashed(h, None, 0, None, None, None, P(buf), None) == ERR_INVALID_ARG and "max_blocks" in lib.icp_last_error(h).decode()
    assert same_cblocks(ctx.tsdf_blocks(colors=True)[1:], before[1:])
    # still legal, geometry-only, and the colours are left alone
    assert len(ctx.tsdf_mesh_hashed()[2]) > 100 and ctx.tsdf_raycast_hashed(cam, np.eye(4, dtype=f32))[3] > 100
    assert ctx.set_target_tsdf_hashed(cam, np.eye(4, dtype=f32)) > 100
    assert same_cblocks(ctx.tsdf_blocks(colors=True)[1:], before[1:])
    # the volume still works
    n_again = ctx.tsdf_integrate(d, cam, np.eye(4, dtype=f32), rgbx=rgbx1)
    assert n_again[0] > 1000 and n_again[1] > 500 and ctx.tsdf_blocks(colors=True)[5].max() == 2
    # an uncoloured hashed volume created afterwards refuses coloured fusion as it always did
    ctx.tsdf_create_hashed(**HC.BOX)
    rc = lib.icp_tsdf_integrate_color(h, P(d), P(rgbx1), B(cam), P(p), B(i32), B(j32))
    msg = lib.icp_last_error(h).decode()
    assert rc == ERR_INVALID_ARG and "hashed volume" in msg and "icp_tsdf_integrate_color" in msg and not ctx.tsdf_has_color()
