"""The hashed TSDF volume on the device (icp_tsdf_create_hashed and the calls that work on either storage) against the numpy restatement
of the contract (tests/htsdf_restatement.py) and against the dense volume: the set of blocks a frame allocates, the integrate voxel for
voxel, growth from a pool of one block, the field sample in every class of cell, the sums of a step, the tracking loop against a
composition of public calls, the outcome on the 41-frame pan that the dense box loses, and the refusals."""
import ctypes as C
import json
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_outcome_fixture as HF
import htsdf_restatement as HR
import sdf_restatement as SR
import tsdf_outcome_fixture as OF
import tsdf_restatement as TS
from icp_amd.synth import camera_sequence, tum_K, wavy_depth
from support import same_bits, pose_of

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_SOURCE = 1, 4
RECORD_KEYS = ("n_depth", "n_valid_first", "n_valid_last", "iterations", "status")


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_record(a, b):
    return all(a[k] == b[k] for k in RECORD_KEYS) and u64(a["cost_first"]) == u64(b["cost_first"]) and u64(a["cost_last"]) == u64(b["cost_last"]) \
        and same_bits(a["pose"], b["pose"])


def same_blocks(a, b):
    """Two (coords, tsdf, weight) triples in icp_get_tsdf_hashed's layout, bit for bit."""
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def assert_equals_restatement(ctx, hv, what):
    info, coords, t, w = ctx.tsdf_blocks()
    rc, rt, rw = hv.sorted_blocks()
    assert info["n_blocks"] == len(rc) and info["n_unplaced"] == 0 and info["n_out_of_range"] == hv.n_out_of_range, (what, info, len(rc))
    assert np.array_equal(coords, rc), what
    assert same_bits(t, rt) and same_bits(w, rw), what
    return info


def test_touch_allocates_the_restated_set(gpu_ctx_factory):
    """The blocks after ONE integrate equal the restatement's exactly, and so do their contents and the count of voxels written: the
    crafted 64 x 48 frame from the tilted pose into the straddling volume (blocks on both sides of 0 on every axis), a 1 x 1 and a 7 x 5
    frame (one partial tile), a frame with no usable depth (no block, nothing written), and a pose that puts every sample beyond 2^20
    blocks (counted, nothing stored)."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    for w, h in ((HC.W, HC.H), (1, 1), (7, 5)):
        cam, rcam = HC.camera(w, h)
        d = HC.crafted_frame() if w == HC.W else wavy_depth(w, h)
        ctx.tsdf_create_hashed(**HC.STRADDLE)
        hv = HR.HVolume(**HC.STRADDLE)
        n = ctx.tsdf_integrate(d, cam, HC.TILTED)
        rn = HR.integrate(hv, d, rcam, HC.TILTED)
        info = assert_equals_restatement(ctx, hv, (w, h))
        b = np.array(sorted(hv.blocks))
        print("touch %d x %d: %d blocks (capacity %d), %d voxels written" % (w, h, info["n_blocks"], info["capacity"], n))
        assert n == rn and n > 0 and info["n_blocks"] > 0
        if w == HC.W:
            assert (b.min(0) < 0).all() and (b.max(0) >= 0).all() and info["n_blocks"] > 20
    cam, rcam = HC.camera()
    ctx.tsdf_create_hashed(**HC.STRADDLE)
    assert ctx.tsdf_integrate(np.full((HC.H, HC.W), MINF, f32), cam, HC.TILTED) == 0
    info, coords, _, _ = ctx.tsdf_blocks()
    assert info["n_blocks"] == 0 and len(coords) == 0 and info["n_out_of_range"] == 0
    far = HC.TILTED.copy(); far[0, 3] = f32(2.0e6)
    d = HC.crafted_frame()
    hv = HR.HVolume(**HC.STRADDLE)
    assert ctx.tsdf_integrate(d, cam, far) == 0 and HR.integrate(hv, d, rcam, far) == 0
    info = ctx.tsdf_blocks()[0]
    assert info["n_blocks"] == 0 and info["n_out_of_range"] == hv.n_out_of_range > 1000
    # one more frame adds to the count; reset clears it
    ctx.tsdf_integrate(d, cam, far)
    assert ctx.tsdf_blocks()[0]["n_out_of_range"] == 2 * hv.n_out_of_range
    ctx.tsdf_reset()
    assert ctx.tsdf_blocks()[0]["n_out_of_range"] == 0


@pytest.mark.parametrize("case", ["box", "negative"])
def test_integrate_equals_the_dense_volume(gpu_ctx_factory, case):
    """After tsdf_allocate_blocks over a box, three frames integrated into the hashed volume and into a dense one (the same origin for
    `box`; for `negative` 1/16 m voxels, a dyadic origin and the dense origin shifted by whole voxels, which is exact) are equal voxel for
    voxel, tsdf_blocks() against tsdf_volume() bit for bit, and n_updated of every frame too."""
    from icp_amd import binding
    opts, lo, nb = (HC.BOX, (0, 0, 0), tuple(d // 8 for d in HC.BOX_DIMS)) if case == "box" else (HC.NEG, HC.NEG_LO, HC.NEG_BLOCKS)
    cam, rcam = HC.camera()
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    h.tsdf_create_hashed(block_capacity=64, **opts)
    box = HC.box_coords(lo, nb)
    h.tsdf_allocate_blocks(box)
    h.tsdf_allocate_blocks(box[::-1][:17])              # allocated already: no effect
    info = h.tsdf_blocks()[0]
    assert info["n_blocks"] == len(box) and info["n_grown"] > 0 and info["n_unplaced"] == 0
    d.tsdf_create(**HC.dense_options(opts, lo, nb))
    for depth, pose in zip(HC.frames(), HC.POSES):
        nh = h.tsdf_integrate(depth, cam, pose); nd = d.tsdf_integrate(depth, cam, pose)
        print("integrate %s: %d voxels written (dense %d)" % (case, nh, nd))
        assert nh == nd > 1000
    info, coords, t, w = h.tsdf_blocks()
    assert info["n_blocks"] == len(box) and np.array_equal(coords, box)      # the frames reach nothing outside the box; sorted by key
    dims = tuple(8 * n for n in nb)
    T, Wt = binding.tsdf_blocks_to_dense(coords, t, w, np.asarray(lo) * 8, dims)
    Td, Wd = d.tsdf_volume()
    assert same_bits(T, Td) and same_bits(Wt, Wd) and Wd.max() == 3


def test_integrate_without_preallocation_matches_restatement(gpu_ctx_factory):
    """Three frames into an empty hashed volume: blocks and contents equal the restatement bit for bit after every frame."""
    cam, rcam = HC.camera()
    for opts in (HC.STRADDLE, HC.NEG):
        ctx = gpu_ctx_factory()
        ctx.tsdf_create_hashed(**opts)
        hv = HR.HVolume(**opts)
        for k, (depth, pose) in enumerate(zip(HC.frames(), HC.POSES)):
            n = ctx.tsdf_integrate(depth, cam, pose)
            assert n == HR.integrate(hv, depth, rcam, pose)
            info = assert_equals_restatement(ctx, hv, k)
        print("three frames: %d blocks, %d growths" % (info["n_blocks"], info["n_grown"]))
        assert info["n_grown"] == 0 and info["n_blocks"] > 40


def test_growth_from_one_block(gpu_ctx_factory):
    """block_capacity=1: the first frame grows the volume several times; afterwards tsdf_blocks() equals that of a volume created with room
    to spare bit for bit, nothing is unplaced, a second integrate of the same frame allocates nothing new, and reserve, upload and reset
    behave: an upload of the blocks reproduces them, in a volume that has to grow for it too."""
    cam, rcam = HC.camera()
    d = HC.crafted_frame()
    small, roomy = gpu_ctx_factory(), gpu_ctx_factory()
    small.tsdf_create_hashed(block_capacity=1, **HC.STRADDLE)
    roomy.tsdf_create_hashed(block_capacity=1 << 10, **HC.STRADDLE)
    assert small.tsdf_blocks()[0]["capacity"] == 1
    ns, nr = small.tsdf_integrate(d, cam, HC.TILTED), roomy.tsdf_integrate(d, cam, HC.TILTED)
    si, *sb = small.tsdf_blocks(); ri, *rb = roomy.tsdf_blocks()
    print("growth: %d blocks after %d growths, capacity %d" % (si["n_blocks"], si["n_grown"], si["capacity"]))
    assert ns == nr and same_blocks(sb, rb)
    assert si["n_grown"] >= 5 and si["n_unplaced"] == 0 and ri["n_grown"] == 0 and si["capacity"] >= si["n_blocks"] == ri["n_blocks"]
    grown = si["n_grown"]
    small.tsdf_integrate(d, cam, HC.TILTED); roomy.tsdf_integrate(d, cam, HC.TILTED)
    si2, *sb2 = small.tsdf_blocks(); _, *rb2 = roomy.tsdf_blocks()
    assert si2["n_blocks"] == si["n_blocks"] and si2["n_grown"] == grown and same_blocks(sb2, rb2) and sb2[2].max() == 2
    # reserve: grows ahead of time, keeps every block
    small.tsdf_reserve_blocks(4 * si["capacity"]); small.tsdf_reserve_blocks(3)
    si3, *sb3 = small.tsdf_blocks()
    assert si3["capacity"] == 4 * si["capacity"] and si3["n_grown"] == grown + 1 and same_blocks(sb3, sb2)
    # upload replaces the state, growing where it must; the blocks come back as they went in, and the field is the same
    up = gpu_ctx_factory()
    up.tsdf_create_hashed(block_capacity=2, **HC.STRADDLE)
    up.tsdf_integrate(wavy_depth(HC.W, HC.H, 1.2), cam, np.eye(4, dtype=f32))
    up.tsdf_upload_blocks(*sb2)
    ui, *ub = up.tsdf_blocks()
    assert same_blocks(ub, sb2) and ui["n_unplaced"] == 0 and ui["capacity"] >= ui["n_blocks"]
    pts = np.random.default_rng(2).uniform((-1.0, -0.8, 1.0), (1.0, 0.8, 2.4), (3000, 3)).astype(f32)      # around the surface
    fa, fb = up.tsdf_sample(pts), roomy.tsdf_sample(pts)
    assert same_bits(fa[0], fb[0]) and same_bits(fa[1], fb[1]) and np.array_equal(fa[2], fb[2]) and fa[2].sum() > 50
    up.tsdf_reset()
    assert up.tsdf_blocks()[0]["n_blocks"] == 0 and up.tsdf_blocks()[0]["capacity"] == ui["capacity"] and not up.tsdf_sample(pts)[2].any()
    # duplicates and coordinates that are not storable are refused, the state untouched
    lib = up.lib
    two = np.zeros((2, 3), np.int32); z = np.zeros((2, 8, 8, 8), f32)
    assert lib.icp_tsdf_upload_hashed(up.h, 2, two.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)) == ERR_INVALID_ARG
    bad = np.array([[1 << 20, 0, 0]], np.int32)
    assert lib.icp_tsdf_allocate_blocks(up.h, 1, bad.ctypes.data_as(C.c_void_p)) == ERR_INVALID_ARG and "storable" in lib.icp_last_error(up.h).decode()
    assert up.tsdf_blocks()[0]["n_blocks"] == 0


def test_growth_is_refused_past_the_maximum_with_nothing_modified(gpu_ctx_factory):
    """The maximum lowered to 2^3 blocks (a test hook; the library's is 2^22): a volume of capacity 8 that holds the one block of the
    1 x 1 frame refuses the 64 x 48 frame, which needs 42 -- ICP_ERR_INVALID_ARG with a message, n_updated 0 -- and is left as it was: the
    same block bit for bit, the same counts apart from the failed claim's mark, the same field; the small frame still integrates, and
    with the maximum back at 2^22 the large one does, to the blocks of a volume that never refused."""
    from icp_amd import binding
    cam, _ = HC.camera()
    cam1, _ = HC.camera(1, 1)
    d, d1 = HC.crafted_frame(), wavy_depth(1, 1)
    ctx, ref = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, ref):
        c.tsdf_create_hashed(block_capacity=8, **HC.STRADDLE)
        assert c.tsdf_integrate(d1, cam1, HC.TILTED) > 0
    assert ctx.lib.icp_debug_htsdf_max_blocks(ctx.h, 3) == 0
    before = ctx.tsdf_blocks()
    assert before[0]["n_blocks"] == 1 and before[0]["capacity"] == 8
    pts = np.random.default_rng(4).uniform((-1.0, -0.8, 1.0), (1.0, 0.8, 2.4), (2000, 3)).astype(f32)
    f_before = ctx.tsdf_sample(pts)
    n = C.c_int32(-1)
    rc = ctx.lib.icp_tsdf_integrate(ctx.h, binding._ptr(d), C.byref(cam), binding._ptr(binding.pose_to_c(HC.TILTED)), C.byref(n))
    msg = ctx.lib.icp_last_error(ctx.h).decode()
    assert rc == ERR_INVALID_ARG and "2^3 blocks" in msg and "icp_tsdf_integrate" in msg and n.value == 0, (rc, msg)
    after = ctx.tsdf_blocks()
    assert same_blocks(after[1:], before[1:]) and after[0]["n_unplaced"] > 0
    assert {k: v for k, v in after[0].items() if k != "n_unplaced"} == {k: v for k, v in before[0].items() if k != "n_unplaced"}
    f_after = ctx.tsdf_sample(pts)
    assert all(same_bits(a, b) for a, b in zip(f_after[:2], f_before[:2])) and np.array_equal(f_after[2], f_before[2])
    bad = HC.box_coords((5, 5, 5), (3, 3, 1))
    assert ctx.lib.icp_tsdf_allocate_blocks(ctx.h, 9, binding._ptr(bad)) == ERR_INVALID_ARG and same_blocks(ctx.tsdf_blocks()[1:], before[1:])
    for c in (ctx, ref):
        c.tsdf_integrate(d1, cam1, HC.TILTED)
    assert same_blocks(ctx.tsdf_blocks()[1:], ref.tsdf_blocks()[1:]) and ctx.tsdf_blocks()[0]["n_unplaced"] == 0
    assert ctx.lib.icp_debug_htsdf_max_blocks(ctx.h, 22) == 0
    assert ctx.tsdf_integrate(d, cam, HC.TILTED) == ref.tsdf_integrate(d, cam, HC.TILTED)
    assert same_blocks(ctx.tsdf_blocks()[1:], ref.tsdf_blocks()[1:]) and ctx.tsdf_blocks()[0]["n_blocks"] > 40


def test_densify_hashed_model(gpu_ctx_factory):
    """tum.densify_hashed_model: the hashed volume replaced by a dense one over the bounding box of its blocks with the same voxels, which
    the mesh extraction and the ray-cast then accept; a volume without a block is a ValueError."""
    from icp_amd import binding, tum
    cam, _ = HC.camera()
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(**HC.NEG)
    with pytest.raises(ValueError):
        tum.densify_hashed_model(ctx)
    for depth, pose in zip(HC.frames(), HC.POSES):
        ctx.tsdf_integrate(depth, cam, pose)
    _, coords, t, w = ctx.tsdf_blocks()
    lo = coords.min(0).astype(np.int64) * 8; dims = (coords.max(0).astype(np.int64) + 1) * 8 - lo
    tum.densify_hashed_model(ctx)
    T, Wt = ctx.tsdf_volume()
    Tr, Wr = binding.tsdf_blocks_to_dense(coords, t, w, lo, dims)
    assert T.shape == tuple(int(x) for x in dims[::-1]) and same_bits(T, Tr) and same_bits(Wt, Wr) and Wt.max() == 3
    v, nrm, tri = ctx.tsdf_mesh()
    hits = ctx.tsdf_raycast(cam, HC.TILTED)[3]
    print("densified %d blocks into %s voxels: %d vertices, %d triangles, %d ray-cast hits" % (len(coords), tuple(dims), len(v), len(tri), hits))
    assert len(tri) > 1000 and hits > 1000
    # the mesh lies where the surface is: NEG's origin is dyadic, so the dense origin is exact and the vertices are in the world's frame
    assert 0.9 < np.median(v[:, 2]) < 2.2


def test_sample_in_every_class_of_cell(gpu_ctx_factory):
    """tsdf_sample on the hashed volume equals tsdf_sample on a dense volume uploaded from tsdf_blocks_to_dense, and the restatement's,
    bit for bit (F, gradient, valid).  The volume: a 4 x 4 x 4 box of blocks around the origin of a dyadic grid (voxel 1/8 m, so shifting the
    origin by whole voxels and q - o at lattice points are exact) with ONE block of the box missing, crafted values, 2 % of the weights 0.
    The points: per class of cell -- inside one block, across a face, an edge, a corner (1, 2, 4, 8 blocks) -- cells chosen by their local
    coordinates, with fractions on a 1/64 lattice; the cells around the missing block (exactly one corner's block missing); NaN, +-inf and
    coordinates beyond the storable range.  Every class must be present, with valid and invalid members where it can have both."""
    from icp_amd import binding
    opts = dict(origin=(0.5, -0.25, 1.0), voxel_size=0.125, truncation=0.375)
    rng = np.random.default_rng(17)
    lo_b = np.array([-2, -2, -2]); missing = (-1, 0, 0)      # 27 junctions of eight blocks inside the box, 8 of them at the hole
    box = HC.box_coords(lo_b, (4, 4, 4))
    coords = box[~(box == np.array(missing)).all(1)]
    assert len(coords) == 63
    t = rng.uniform(-1.5, 1.5, (63, 8, 8, 8)).astype(f32); w = rng.choice(np.array([1, 2.5, 7], f32), (63, 8, 8, 8))
    w[rng.random(w.shape) < 0.02] = 0
    t.view(np.uint32)[rng.random(t.shape) < 0.003] = 0x7FC12345
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    h.tsdf_create_hashed(block_capacity=8, **opts)
    h.tsdf_upload_blocks(coords, t, w)
    _, gc, gt, gw = h.tsdf_blocks()
    order = np.lexsort((coords[:, 0], coords[:, 1], coords[:, 2]))
    assert np.array_equal(gc, coords[order]) and same_bits(gt, t[order]) and same_bits(gw, w[order])
    lo = lo_b * 8
    T, Wt = binding.tsdf_blocks_to_dense(coords, t, w, lo, (32, 32, 32))
    o, s = np.array(opts["origin"], f32), f32(0.125)
    d_origin = tuple(float(o[a] + f32(lo[a]) * s) for a in range(3))
    d.tsdf_create(dims=(32, 32, 32), origin=d_origin, voxel_size=0.125, truncation=0.375)
    d.tsdf_upload(T, Wt)
    hv = HR.HVolume(**opts)
    hv.allocate(coords)
    for c, tt, ww in zip(coords, t, w):
        hv.blocks[tuple(int(x) for x in c)] = [tt, ww]
    # cells: 6000 at random in and around the box, then 400 per class with the local coordinates set, then the neighbourhood of the hole
    cells = [rng.integers(lo - 3, lo + 35, (6000, 3))]
    for n_cross in range(4):
        f = rng.integers(lo, lo + 32, (400, 3))
        f = (f & ~7) + rng.integers(0, 7, (400, 3))                 # local 0 .. 6 on every axis
        for i in range(400):
            f[i, rng.permutation(3)[:n_cross]] |= 7               # local 7 on n_cross axes
        cells.append(f)
    m0 = np.array(missing) * 8
    around = np.array([[x, y, z] for x in (-1, 3, 7) for y in (-1, 3, 7) for z in (-1, 3, 7)]) + m0      # touches the missing block unless it is its centre
    cells.append(np.repeat(around, 4, 0))
    cells = np.concatenate(cells)
    frac = rng.integers(0, 64, cells.shape).astype(f32) / f32(64)
    pts = (o + (cells.astype(f32) + frac) * s).astype(f32)
    assert np.array_equal(np.floor((pts - o) / s), cells.astype(f32))      # exact: the cell is the one intended
    special = np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [3e6, 0, 1], [0, -3e6, 1], [0, 0, 1.1e6], [1.048570e6, 0, 1]], f32)
    pts = np.concatenate([pts, special]).astype(f32)
    F, G, ok = h.tsdf_sample(pts)
    Fd, Gd, okd = d.tsdf_sample(pts)
    Fr, Gr, okr = SR.sample(hv, pts)
    assert np.array_equal(ok, okd) and same_bits(F, Fd) and same_bits(G, Gd)
    assert np.array_equal(ok, okr.astype(bool)) and same_bits(F, Fr) and same_bits(G, Gr)
    n = len(cells)
    okc = ok[:n]
    n_cross = ((cells & 7) == 7).sum(1)
    in_box = ((cells >= lo) & (cells + 1 < lo + 32)).all(1)
    for k in range(4):
        m = (n_cross == k) & in_box
        print("sample: %d cells across %d block boundaries, %d valid" % (m.sum(), k, okc[m].sum()))
        assert okc[m].sum() >= 30 and (~okc[m]).sum() >= 1, k
    # exactly one corner's block missing: the corner cells at the eight corners of the hole, the face and edge cells on its skin
    blocks_of = lambda f: {tuple(((f + np.array([k & 1, (k >> 1) & 1, k >> 2])) >> 3).tolist()) for k in range(8)}
    have = {tuple(c) for c in coords.tolist()}
    one_missing = np.array([len(blocks_of(f) - have) == 1 and len(blocks_of(f)) > 1 for f in cells])
    print("sample: %d cells with exactly one corner's block missing; %d valid cells at negative coordinates" % (one_missing.sum(), (okc & (cells < 0).all(1)).sum()))
    assert one_missing.sum() >= 40 and not okc[one_missing].any() and (F[:n][one_missing] == 0).all()
    assert {len(blocks_of(f)) for f in cells[one_missing]} == {2, 4, 8}
    assert (okc & (cells < 0).all(1)).sum() >= 20 and (okc & (cells >= 0).all(1)).sum() >= 20
    assert not ok[n:].any() and (F[n:] == 0).all() and (G[n:] == 0).all()
    assert (F[~ok] == 0).all() and np.isnan(F[ok]).sum() > 0


def check_system(h, d, vol, cam, rcam, depth, pose, what, **kw):
    """icp_tsdf_sdf_system on the hashed volume against the densified dense one (counts equal, sums reported) and against the restatement
    (tests/test_gpu_sdf.py's bound: n_valid 2^-52 sum |term|); two calls identical."""
    sums, counts = h.tsdf_sdf_system(depth, cam, pose, **kw)
    dsums, dcounts = d.tsdf_sdf_system(depth, cam, pose, **kw)
    rcounts, rsums, rabs = SR.system(vol, depth, rcam, pose, **kw)
    bound = rcounts[1] * 2.0 ** -52 * rabs
    err = np.abs(sums - rsums)
    equal = np.array_equal(u64(sums), u64(dsums))
    print("system %s %s: n_depth %d, n_valid %d, worst |sum - restatement| / bound = %.3g, bit-equal to the dense call: %s"
          % (what, kw, counts[0], counts[1], (err / np.maximum(bound, 1e-300)).max(), equal))
    assert tuple(counts) == tuple(dcounts) == tuple(rcounts), what
    assert (err <= bound).all(), (what, kw, err, bound)
    again, counts2 = h.tsdf_sdf_system(depth, cam, pose, **kw)
    assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts), what
    return counts, equal


def test_system_matches_dense_and_restatement(gpu_ctx_factory):
    """The sums of one step on the hashed volume (two frames fused on the device, all blocks at non-negative coordinates) against the dense
    volume uploaded from its blocks with the same origin, and against the restatement: 40 x 30 at strides 1 and 3, huber 0 and 0.05,
    two poses; 70 x 50 at stride 1 (20 blocks, partial tiles on both axes)."""
    from icp_amd import binding
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    cam64, _ = HC.camera()
    h.tsdf_create_hashed(**HC.BOX)
    for depth, pose in list(zip(HC.frames(), HC.POSES))[:2]:
        h.tsdf_integrate(depth, cam64, pose)
    _, coords, t, w = h.tsdf_blocks()
    assert coords.min() >= 0 and (coords.max(0) < np.array(HC.BOX_DIMS) // 8).all()
    dense = dict(HC.BOX, dims=HC.BOX_DIMS)
    T, Wt = binding.tsdf_blocks_to_dense(coords, t, w, (0, 0, 0), HC.BOX_DIMS)
    d.tsdf_create(**dense); d.tsdf_upload(T, Wt)
    vol = TS.Volume(**dense); vol.tsdf, vol.weight = T, Wt
    cam, rcam = HC.camera(40, 30)
    frame = HC.crafted_frame(40, 30)
    near = pose_of((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))
    equal = []
    for pose in (np.eye(4, dtype=f32), near):
        for stride in (1, 3):
            for huber in (0.0, 0.05):
                counts, eq = check_system(h, d, vol, cam, rcam, frame, pose, "40 x 30", stride=stride, huber=huber)
                equal.append(eq)
                if stride == 1:
                    assert 500 < counts[1] <= counts[0] < 40 * 30
    cam70, rcam70 = HC.camera(70, 50)
    counts, eq = check_system(h, d, vol, cam70, rcam70, wavy_depth(70, 50), near, "70 x 50", stride=1)
    equal.append(eq)
    assert counts[1] > 1000
    print("system: %d of %d calls bit-equal to the dense volume's" % (sum(equal), len(equal)))


def python_loop(ctx, depth, cam, **kw):
    """icp_track_depth_sdf as a composition of public calls (the volume exists)."""
    pose = np.eye(4, dtype=f32)
    ctx.tsdf_integrate(depth[0], cam, pose)
    recs = []
    for k in range(1, len(depth)):
        pose, rec, rc = ctx.tsdf_align_depth(depth[k], cam, pose, **kw)
        if rc == 0:
            ctx.tsdf_integrate(depth[k], cam, pose)
        recs.append(rec)
    return pose, recs


def test_track_depth_sdf_matches_composition_of_public_calls(gpu_ctx_factory):
    """5 frames of 40 x 30 of the synthetic room, frame 2 all MINF, on a hashed volume that starts with 16 blocks: records, poses and the
    blocks bit for bit, and every tracked pose near its ground truth."""
    from icp_amd import binding
    K, depth, _, gt = camera_sequence(5, 40, 30)
    depth[2][:] = MINF
    cam = binding.depth_camera(K, 40, 30)
    opts = dict(origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.tsdf_create_hashed(block_capacity=16, **opts)
    kw = dict(stride=1, n_iterations=12)
    pose, recs, rc = a.track_depth_sdf(depth, cam, **kw)
    ref_pose, ref = python_loop(b, depth, cam, **kw)
    print("track_depth_sdf (hashed): statuses %s, iterations %s, n_valid %s" % ([r["status"] for r in recs], [r["iterations"] for r in recs], [r["n_valid_last"] for r in recs]))
    assert len(recs) == 4 and rc == ERR_NO_SOURCE
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert same_record(r, h), (k, r, h)
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    assert [r["status"] for r in recs] == [0, ERR_NO_SOURCE, 0, 0] and same_bits(recs[1]["pose"], recs[0]["pose"])
    ai, *ab = a.tsdf_blocks(); bi, *bb = b.tsdf_blocks()
    assert same_blocks(ab, bb) and ab[2].max() == 4 and ai["n_grown"] == bi["n_grown"] > 0 and ai["n_unplaced"] == 0
    for r, g in zip(recs, gt):
        if r["status"] == 0:
            e = OF.pose_error(r["pose"], g)
            assert e[0] < 0.05 and e[1] < 0.1, e
    # colour frames on a hashed volume: refused
    rgbx = np.zeros((5, 40 * 30, 4), np.uint8)
    out = (binding.IcpSdfFrame * 4)(); o = binding.sdf_options(); p = binding.pose_to_c(np.eye(4, dtype=f32))
    d = np.ascontiguousarray(depth, f32)
    assert a.lib.icp_track_depth_sdf(a.h, binding._ptr(d), binding._ptr(rgbx), C.c_int32(5), C.byref(cam), C.byref(o), binding._ptr(p), out) == ERR_INVALID_ARG
    assert "hashed" in a.lib.icp_last_error(a.h).decode()


def test_outcome_on_the_pan(gpu_ctx_factory):
    """The 41-frame, 60 degree pan of tests/tsdf_outcome_fixture.py through tum.track on a HASHED model with that fixture's origin, voxel
    size and truncation and sdf=dict(stride=4, n_iterations=20).  Figures (worst frame, rotation [rad] / translation [m]):
      restatement on the CPU (tests/golden/htsdf_outcome.json): 0.0074 rad / 0.0391 m, 759 blocks after frame 0, 1113 after frame 40
      dense restatement in the box cut to dims (100, 69, 177) at the same origin: ends 1.27 rad / 5.56 m off, every status ICP_OK
      device: printed below next to the bounds
    The bound is TWICE the restatement's worst frame, the margin sections 6q and 6s give a device run over its restatement; the block
    count is the restatement's exactly.  The same test tracks the pan on the device with the dense volume cut to (100, 69, 177) and asserts
    that it ends more than ten times farther off than the hashed run: the failure a fixed extent causes, without an error."""
    from icp_amd import tum
    with open(HF.GOLDEN) as f:
        ref = json.load(f)
    K, depth, gt = OF.fixture()
    seq = dict(depth=depth, rgbx=None, gt=gt, K=K, width=OF.W, height=OF.H)
    ctx = gpu_ctx_factory()
    poses, recs, rc = tum.track(ctx, seq, with_gt=False, model=HF.hashed_model(), sdf=dict(HF.OPTIONS))
    rot, tr, last = OF.worst_errors([np.eye(4)] + [r["pose"] for r in recs], gt)
    info = ctx.tsdf_blocks()[0]
    print("restatement: worst %.4f rad / %.4f m, %d blocks; device on the hashed volume: worst %.4f rad / %.4f m (bound %.4f / %.4f), last %.4f rad / %.4f m, "
          "status %d, %d blocks (capacity %d, %d growths), iterations %s"
          % (ref["worst_rotation_rad"], ref["worst_translation_m"], ref["n_blocks"][-1], rot, tr, 2 * ref["worst_rotation_rad"], 2 * ref["worst_translation_m"],
             last[0], last[1], rc, info["n_blocks"], info["capacity"], info["n_grown"], [r["iterations"] for r in recs]))
    cut = gpu_ctx_factory()
    _, crecs, crc = tum.track(cut, seq, with_gt=False, model=HF.cut_model(), sdf=dict(HF.OPTIONS))
    _, _, clast = OF.worst_errors([np.eye(4)] + [r["pose"] for r in crecs], gt)
    print("dense volume cut to %s: ends %.3f rad / %.3f m off (CPU: %.3f / %.3f), status %d, statuses %s"
          % (HF.CUT_DIMS, clast[0], clast[1], ref["cut_last_rotation_rad"], ref["cut_last_translation_m"], crc, sorted(set(r["status"] for r in crecs))))
    assert rc == 0 and all(r["status"] == 0 for r in recs) and len(recs) == OF.N_FRAMES - 1
    assert rot <= 2 * ref["worst_rotation_rad"] and tr <= 2 * ref["worst_translation_m"]
    assert info["n_blocks"] == ref["n_blocks"][-1] and info["n_unplaced"] == 0 and info["n_out_of_range"] == ref["n_out_of_range"]
    assert clast[0] > 10 * last[0] and clast[1] > 10 * last[1]


def test_refusals_leave_the_blocks_alone(gpu_ctx_factory):
    """Every call that needs the dense box returns ICP_ERR_INVALID_ARG on a hashed volume with a message that names it, and leaves the
    blocks bit-identical; the hashed-only calls refuse a dense volume; a dense volume created afterwards behaves as one created first."""
    from icp_amd import binding
    cam, rcam = HC.camera()
    ctx, ref = gpu_ctx_factory(), gpu_ctx_factory()
    ctx.tsdf_create_hashed(**HC.BOX)
    d = HC.crafted_frame()
    ctx.tsdf_integrate(d, cam, np.eye(4, dtype=f32))
    before = ctx.tsdf_blocks()
    lib, h = ctx.lib, ctx.h
    n = HC.W * HC.H
    p = binding.pose_to_c(np.eye(4, dtype=f32)); buf = np.zeros(n * 4, f32); i32 = C.c_int32(0); j32 = C.c_int32(0)
    rgbx = np.zeros((2, n, 4), np.uint8); d2 = np.ascontiguousarray(np.stack([d, d]), f32)
    so = binding.depth_options(False, 2); sdfo = binding.sdf_options(); co = binding.sdf_color_options(weight=0.1)
    tf = (binding.IcpTrackFrame * 1)(); sf = (binding.IcpSdfColorFrame * 1)(); sums = np.zeros(29); cnt = (C.c_int32 * 3)()
    P, B, R = binding._ptr, C.byref, binding._ptr(rgbx)
    calls = {
        "icp_tsdf_download": lambda: lib.icp_tsdf_download(h, P(buf), P(buf)),
        "icp_tsdf_upload": lambda: lib.icp_tsdf_upload(h, P(buf), P(buf)),
        "icp_tsdf_raycast": lambda: lib.icp_tsdf_raycast(h, B(cam), P(p), P(buf), None, None, B(i32)),
        "icp_tsdf_raycast_color": lambda: lib.icp_tsdf_raycast_color(h, B(cam), P(p), P(buf), None, None, None, B(i32), B(j32)),
        "icp_set_target_tsdf": lambda: lib.icp_set_target_tsdf(h, B(cam), P(p), B(i32)),
        "icp_set_target_tsdf_color": lambda: lib.icp_set_target_tsdf_color(h, B(cam), P(p), B(i32)),
        "icp_track_depth_model": lambda: lib.icp_track_depth_model(h, P(d2), C.c_int32(2), B(cam), B(so), None, P(p), tf),
        "icp_track_depth_model_color": lambda: lib.icp_track_depth_model_color(h, P(d2), R, C.c_int32(2), B(cam), B(so), None, P(p), tf),
        "icp_tsdf_mesh": lambda: lib.icp_tsdf_mesh(h, C.c_float(0), C.c_int32(0), C.c_int32(0), None, None, None, B(i32), B(j32)),
        "icp_tsdf_mesh_color": lambda: lib.icp_tsdf_mesh_color(h, C.c_float(0), C.c_int32(0), C.c_int32(0), None, None, None, None, B(i32), B(j32)),
        "icp_tsdf_color_create": lambda: lib.icp_tsdf_color_create(h),
        "icp_tsdf_color_release": lambda: lib.icp_tsdf_color_release(h),
        "icp_tsdf_color_download": lambda: lib.icp_tsdf_color_download(h, P(buf), P(buf)),
        "icp_tsdf_color_upload": lambda: lib.icp_tsdf_color_upload(h, P(buf), P(buf)),
        "icp_tsdf_integrate_color": lambda: lib.icp_tsdf_integrate_color(h, P(d), R, B(cam), P(p), B(i32), B(j32)),
        "icp_tsdf_sample_color": lambda: lib.icp_tsdf_sample_color(h, P(buf), C.c_int32(4), None, None, None),
        "icp_tsdf_sdf_system_color": lambda: lib.icp_tsdf_sdf_system_color(h, P(d), R, B(cam), P(p), B(sdfo), B(co), P(sums), cnt),
        "icp_tsdf_align_depth_color": lambda: lib.icp_tsdf_align_depth_color(h, P(d), R, B(cam), B(sdfo), B(co), P(p), B(sf[0]), None),
        "icp_track_depth_sdf_color": lambda: lib.icp_track_depth_sdf_color(h, P(d2), R, C.c_int32(2), B(cam), B(sdfo), B(co), P(p), sf),
    }
    for name, call in calls.items():
        rc = call()
        msg = lib.icp_last_error(h).decode()
        assert rc == ERR_INVALID_ARG and "hashed volume" in msg and name in msg, (name, rc, msg)
    after = ctx.tsdf_blocks()
    assert after[0] == before[0] and same_blocks(after[1:], before[1:])
    assert same_bits(binding.pose_from_c(p), np.eye(4, dtype=f32))
    # the volume still works
    n_again = ctx.tsdf_integrate(d, cam, np.eye(4, dtype=f32))
    assert n_again > 1000 and ctx.tsdf_blocks()[3].max() == 2
    # the hashed-only calls on a dense volume, and on none
    ctx.tsdf_create(dims=HC.BOX_DIMS, **HC.BOX)
    one = np.zeros((1, 3), np.int32)
    for rc in (lib.icp_tsdf_reserve_blocks(h, 64), lib.icp_tsdf_allocate_blocks(h, 1, P(one)), lib.icp_get_tsdf_hashed(h, None, 0, None, None, None),
               lib.icp_tsdf_upload_hashed(h, 0, None, None, None)):
        assert rc == ERR_INVALID_ARG and "dense" in lib.icp_last_error(h).decode()
    # the dense volume made after a hashed one behaves as one made first
    ref.tsdf_create(dims=HC.BOX_DIMS, **HC.BOX)
    for c in (ctx, ref):
        for depth, pose in zip(HC.frames(), HC.POSES):
            c.tsdf_integrate(depth, cam, pose)
    (ta, wa), (tb, wb) = ctx.tsdf_volume(), ref.tsdf_volume()
    assert same_bits(ta, tb) and same_bits(wa, wb) and wa.max() == 3
    ra, rb = ctx.tsdf_raycast(cam, HC.TILTED), ref.tsdf_raycast(cam, HC.TILTED)
    assert same_bits(ra[0], rb[0]) and ra[3] == rb[3] > 100
    ctx.tsdf_release()
    assert lib.icp_tsdf_reserve_blocks(h, 64) == ERR_INVALID_ARG and "no volume" in lib.icp_last_error(h).decode()
    # back to a hashed one, released, and bad options
    ctx.tsdf_create_hashed(**HC.STRADDLE)
    assert ctx.tsdf_integrate(d, cam, HC.TILTED) > 1000
    ctx.tsdf_release()
    o = binding.tsdf_options(origin=(0, 0, 0))
    for kw, word in ((dict(voxel_size=0.0), "voxel_size"), (dict(truncation=-1.0), "truncation"), (dict(voxel_size=1e-4, truncation=0.25), "1024")):
        bad = binding.tsdf_options(origin=(0, 0, 0), **kw)
        assert lib.icp_tsdf_create_hashed(h, B(bad), 16) == ERR_INVALID_ARG and word in lib.icp_last_error(h).decode(), kw
    for cap in (0, -1, (1 << 22) + 1):
        assert lib.icp_tsdf_create_hashed(h, B(o), cap) == ERR_INVALID_ARG and "block_capacity" in lib.icp_last_error(h).decode()
