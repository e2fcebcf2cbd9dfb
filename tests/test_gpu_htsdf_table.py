"""The hashed TSDF volume's block table on the device (ht_lookup, ht_touch_block, k_htsdf_rehash of dev_tsdf_hash.hpp on dev_hmap.hpp's
key, home and probe helpers) driven through crafted probe chains and at the edges of the storable range, tests/htsdf_table_cases.py's cases.

Part A: volumes of block_capacity=128 (a pool of 128 blocks behind 256 slots) against a volume created with 2^12 blocks, where nothing
collides, and against the restatements: chains that wrap, forty keys on one home slot, a full pool (every lane through ht_touch_block's
own probe loop), a growth that rehashes colliding keys into 512 slots, a refused growth, and lookups behind more than 16 occupied slots
from the sample, the system, the touch, the integrate, the evict, the insert's presence test, the ray-cast, the mesh and the colour calls.

Part B: origin 0 and 1 m voxels, where coordinates up to 2^23 are exact and the cell is floor(q): the blocks 2^20 - 1 and -2^20 on every
axis, with the TRAP block beside them -- the storable block whose key one block past the edge has when hm_key packs it (the fields are
not masked) -- filled with a constant that a read through the alias would show."""
import ctypes as C
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_color_view_cases as VC
import htsdf_evict_restatement as ER
import htsdf_raycast_restatement as RR
import htsdf_restatement as HR
import htsdf_table_cases as TC
import sdf_restatement as SR
from support import same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG = 1
ROOMY = 1 << 12


@pytest.fixture(scope="module")
def pair(gpu_ctx_factory):
    """Two contexts for the whole module: every test creates its volumes anew in them."""
    return gpu_ctx_factory(), gpu_ctx_factory()


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_blocks(a, b):
    return np.array_equal(a[0], b[0]) and all(same_bits(x, y) for x, y in zip(a[1:], b[1:]))


def same_sample(a, b):
    return same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(np.asarray(a[2], bool), np.asarray(b[2], bool))


def ptr(a):
    from icp_amd import binding
    return binding._ptr(a)


def without(info, *keys):
    return {k: v for k, v in info.items() if k not in keys}


# ================================================================================================ part A
@pytest.mark.parametrize("case", ["WRAP", "ONE_HOME", "RUN", "FULL", "FULL shuffled 1", "FULL shuffled 2"])
def test_allocate_down_crafted_chains(pair, case):
    """tsdf_allocate_blocks of a crafted set in ONE call (WRAP's forty keys are one wave's lanes 0 .. 39, all claiming down the chain that
    starts at the table's last slot): exactly the set, sorted by key, all zero, nothing unplaced, no growth; the reversed set again changes
    nothing."""
    ctx = pair[0]
    cc = TC.sets()[case.split()[0]]
    if "shuffled" in case:
        cc = cc[np.random.default_rng(int(case[-1])).permutation(len(cc))]
    ctx.tsdf_create_hashed(block_capacity=TC.CAPACITY, **TC.DYADIC)
    want = TC.sorted_by_key(cc)[0]
    for coords in (cc, cc[::-1]):
        ctx.tsdf_allocate_blocks(coords)
        info, c, t, w = ctx.tsdf_blocks()
        assert np.array_equal(c, want), case
        assert not t.view(np.uint32).any() and not w.view(np.uint32).any()
        assert info == dict(n_blocks=len(cc), capacity=TC.CAPACITY, n_grown=0, n_unplaced=0, n_out_of_range=0), (case, info)


def full_state(ctx):
    """Case 2's state: FULL uploaded with contents into a pool of exactly 128.  Returns (sorted blocks, lattice points, their values)."""
    S = TC.sets()
    t, w = TC.contents(S["FULL"])
    ctx.tsdf_create_hashed(block_capacity=TC.CAPACITY, **TC.DYADIC)
    ctx.tsdf_upload_blocks(S["FULL"], t, w)
    info = ctx.tsdf_blocks()[0]
    assert info["n_blocks"] == info["capacity"] == TC.CAPACITY and info["n_grown"] == 0 and info["n_unplaced"] == 0, info
    pts, _ = TC.block_lattice_points(TC.DYADIC, S["FULL"])
    return TC.sorted_by_key(S["FULL"], t, w), pts, t[:, 4, 2, 3]


def test_the_pool_full_loop_finds_every_key(pair):
    """With the pool exactly full, tsdf_allocate_blocks(FULL reversed) sends every lane through ht_touch_block's own probe loop, behind a
    cluster of 80 that wraps: all 128 keys found, nothing grows, nothing changes.  One more block whose home is 255 then grows the volume
    exactly once; k_htsdf_rehash enters the 128 keys into 512 slots, where WRAP's forty collide at slot 511.  A lattice point inside every
    block samples that block's value."""
    ctx = pair[0]
    S = TC.sets()
    want, pts, values = full_state(ctx)
    assert same_blocks(ctx.tsdf_blocks()[1:], want)
    ctx.tsdf_allocate_blocks(S["FULL"][::-1])
    info, *got = ctx.tsdf_blocks()
    assert info == dict(n_blocks=128, capacity=128, n_grown=0, n_unplaced=0, n_out_of_range=0), info
    assert same_blocks(got, want)
    hv = TC.volume_of(TC.DYADIC, *want)
    ref = SR.sample(hv, pts)
    assert ref[2].all() and same_bits(ref[0], values)
    assert same_sample(ctx.tsdf_sample(pts), ref)
    ctx.tsdf_allocate_blocks(np.concatenate([S["FULL"], S["NEW255"][None]]))
    info, c, t, w = ctx.tsdf_blocks()
    assert info == dict(n_blocks=129, capacity=256, n_grown=1, n_unplaced=0, n_out_of_range=0), info
    new = (c == S["NEW255"]).all(1)
    assert new.sum() == 1 and not t[new].view(np.uint32).any() and not w[new].view(np.uint32).any()
    assert same_blocks((c[~new], t[~new], w[~new]), want)
    assert same_sample(ctx.tsdf_sample(pts), ref)


def test_refused_growth_rebuilds_the_table(pair):
    """The maximum lowered to 2^7 blocks: one new block with home 255 is refused, and the table, rebuilt from the 128 pool keys behind the
    same cluster, answers as before: blocks, sample and every info field apart from n_unplaced."""
    ctx = pair[0]
    S = TC.sets()
    want, pts, _ = full_state(ctx)
    try:
        assert ctx.lib.icp_debug_htsdf_max_blocks(ctx.h, 7) == 0
        before = ctx.tsdf_blocks(); f_before = ctx.tsdf_sample(pts)
        one = np.ascontiguousarray(S["NEW255"][None], np.int32)
        rc = ctx.lib.icp_tsdf_allocate_blocks(ctx.h, 1, ptr(one))
        msg = ctx.lib.icp_last_error(ctx.h).decode()
        assert rc == ERR_INVALID_ARG and "2^7 blocks" in msg, (rc, msg)
        after = ctx.tsdf_blocks(); f_after = ctx.tsdf_sample(pts)
        assert same_blocks(after[1:], before[1:]) and same_blocks(after[1:], want)
        assert same_sample(f_after, f_before) and f_after[2].all()
        assert without(after[0], "n_unplaced") == without(before[0], "n_unplaced") and after[0]["n_unplaced"] == 1
        ctx.tsdf_allocate_blocks(S["FULL"])                  # allocated already: nothing to grow for
        assert same_blocks(ctx.tsdf_blocks()[1:], want) and ctx.tsdf_blocks()[0]["n_unplaced"] == 0
    finally:
        ctx.lib.icp_debug_htsdf_max_blocks(ctx.h, 22)


def test_upload_and_place_through_a_crowded_table(pair):
    """CROWD uploaded (fillers and junction with their contents, 2 % of the weights 0) into the crowded and into the roomy volume: both give
    back what went in, bit for bit."""
    crowded, roomy = pair
    cr = TC.crowd()
    cc = np.concatenate([cr["fillers"], cr["junction"]])
    t, w = TC.contents(cc, holes=0.02)
    want = TC.sorted_by_key(cc, t, w)
    for ctx, cap in ((crowded, TC.CAPACITY), (roomy, ROOMY)):
        ctx.tsdf_create_hashed(block_capacity=cap, **TC.DYADIC)
        ctx.tsdf_upload_blocks(cc, t, w)
        info, *got = ctx.tsdf_blocks()
        assert same_blocks(got, want) and info["n_blocks"] == 120 and info["capacity"] == cap and info["n_grown"] == 0 and info["n_unplaced"] == 0, info
    assert same_blocks(crowded.tsdf_blocks()[1:], roomy.tsdf_blocks()[1:])


def crowded_junction(pair, color=False):
    """Case 5's state in both volumes: the fillers allocated first in a call of their own, then the junction inserted -- the order that
    puts the junction's blocks behind the fillers.  Returns the restatement's volume (the junction alone: a filler is unobserved)."""
    cr = TC.crowd()
    t, w = TC.contents(cr["junction"], holes=0.02)
    for ctx, cap in zip(pair, (TC.CAPACITY, ROOMY)):
        ctx.tsdf_create_hashed(block_capacity=cap, color=color, **TC.DYADIC)
        ctx.tsdf_allocate_blocks(cr["fillers"])
        if color:
            info = ctx.tsdf_insert_blocks_color(cr["junction"], t, w, *TC.colours(cr["junction"]))
        else:
            info = ctx.tsdf_insert_blocks(cr["junction"], t, w)
        assert info["n_inserted"] == 8 and info["n_blocks"] == 120 and info["capacity"] == cap and info["n_grown"] == 0, info
    return TC.volume_of(TC.DYADIC, cr["junction"], t, w)


def test_sample_and_system_through_a_crowded_table(pair):
    """The junction's cells by class (inside one block, across a face, an edge, the corner) and the 27 cells about its centre, every one
    looked up behind the fillers: F, gradient and valid bit-equal to the roomy volume and to the restatement.  The sums of one step for a
    64 x 48 frame looking at the junction: counts and sums equal to the roomy volume's, within the project's bound of the restatement."""
    from test_gpu_htsdf import check_system
    crowded, roomy = pair
    hv = crowded_junction(pair)
    pts, cells, cls = TC.junction_cells()
    got, ref, res = crowded.tsdf_sample(pts), roomy.tsdf_sample(pts), SR.sample(hv, pts)
    assert same_sample(got, ref) and same_sample(got, res)
    for k in range(4):
        print("crowded sample: %d cells across %d block boundaries, %d valid" % ((cls == k).sum(), k, got[2][cls == k].sum()))
        assert got[2][cls == k].sum() >= 30 and (~got[2][cls == k]).sum() >= 1
    assert got[2][-27:].sum() >= 8
    cam, rcam = HC.camera()
    depth, pose = TC.junction_view()
    counts, equal = check_system(crowded, roomy, hv, cam, rcam, depth, pose, "crowded junction")
    assert equal and counts[1] > 100


def crowded_scene(pair, frames=1, color=False):
    """Case 6's crowded state in both volumes: SCENE_CROWD's fillers allocated first, then the first `frames` frames of HC.frames() fused
    from HC.POSES (the first frame's 38 blocks beside the 80 fillers: 118 blocks in 256 slots)."""
    sc = TC.scene_crowd()
    cam, _ = HC.camera()
    for ctx, cap in zip(pair, (TC.CAPACITY, ROOMY)):
        ctx.tsdf_create_hashed(block_capacity=cap, color=color, **HC.STRADDLE)
        ctx.tsdf_allocate_blocks(sc["fillers"])
        for depth, rgbx, pose in list(zip(HC.frames(), VC.color_frames(), HC.POSES))[:frames]:
            ctx.tsdf_integrate(depth, cam, pose, rgbx=rgbx if color else None)
    return sc


def test_touch_and_integrate_in_a_crowded_table(pair):
    """The three frames fused behind SCENE_CROWD's fillers: after every frame the count of voxels written and the blocks equal the roomy
    volume's bit for bit, and, the fillers taken out, the restatement's.  The first frame's 38 blocks fit beside the 80 fillers (118 in
    256 slots): no growth.  The second frame brings the scene to 51 blocks, 131 with the fillers, which a pool of 128 cannot hold
    (tests/test_htsdf_table_host.py): the touch fills the pool behind the crowd, the volume grows exactly once, and the crowded table is
    rehashed into 512 slots in the middle of the sequence.  No filler is ever written."""
    crowded, roomy = pair
    sc = TC.scene_crowd()
    cam, rcam = HC.camera()
    for ctx, cap in zip(pair, (TC.CAPACITY, ROOMY)):
        ctx.tsdf_create_hashed(block_capacity=cap, **HC.STRADDLE)
        ctx.tsdf_allocate_blocks(sc["fillers"])
    hv = HR.HVolume(**HC.STRADDLE)
    fillers = {tuple(c) for c in sc["fillers"].tolist()}
    for k, (depth, pose) in enumerate(zip(HC.frames(), HC.POSES)):
        n, nr = crowded.tsdf_integrate(depth, cam, pose), roomy.tsdf_integrate(depth, cam, pose)
        assert n == nr == HR.integrate(hv, depth, rcam, pose) and n > 1000
        info, c, t, w = crowded.tsdf_blocks()
        rinfo, *rb = roomy.tsdf_blocks()
        assert same_blocks((c, t, w), rb), k
        is_filler = np.array([tuple(x) in fillers for x in c.tolist()])
        assert is_filler.sum() == 80 and not w[is_filler].view(np.uint32).any() and not t[is_filler].view(np.uint32).any()
        assert same_blocks((c[~is_filler], t[~is_filler], w[~is_filler]), hv.sorted_blocks()), k
        print("crowded integrate, frame %d: %d voxels written, %d blocks, capacity %d, %d growths" % (k, n, info["n_blocks"], info["capacity"], info["n_grown"]))
        assert info["n_unplaced"] == 0 and info["n_out_of_range"] == 0 and rinfo["n_grown"] == 0
        assert (info["n_grown"], info["capacity"]) == ((0, 128) if info["n_blocks"] <= 128 else (1, 256)), info
        assert info["n_blocks"] == (118, 131, 131)[k]


def scene_points():
    return np.random.default_rng(2).uniform((-1.0, -0.8, 1.0), (1.0, 0.8, 2.4), (3000, 3)).astype(f32)      # around the surface


def test_evict_present_insert_in_a_crowded_table(pair):
    """From the crowded scene (118 blocks in 256 slots): an evict that keeps about half the scene and no filler rebuilds the table; the kept
    blocks equal the roomy volume's after the same evict and are found by the sample as before, no evicted block is found (both as the
    restatement has it); an insert of the held blocks with one kept block among them is refused with n_present 1; the held blocks alone
    restore the state bit for bit."""
    from icp_amd import binding
    crowded, roomy = pair
    sc = crowded_scene(pair)
    cam, rcam = HC.camera()
    hv = HR.HVolume(**HC.STRADDLE)
    hv.allocate(sc["fillers"])
    HR.integrate(hv, HC.frames()[0], rcam, HC.POSES[0])
    binfo, *before = crowded.tsdf_blocks()
    assert same_blocks(before, hv.sorted_blocks()) and binfo["n_blocks"] == 118 and binfo["capacity"] == 128
    pts = scene_points()
    f_before = crowded.tsdf_sample(pts)
    scene = np.array([b for b in hv.blocks if np.abs(b).max() < 8])
    o = np.asarray(HC.STRADDLE["origin"], np.float64); s = HC.STRADDLE["voxel_size"]
    centre = tuple(float(x) for x in np.median(o + (scene * 8 + 3.5) * s, axis=0).astype(f32))
    radius = float(np.median(np.linalg.norm(o + (scene * 8 + 3.5) * s - np.array(centre), axis=1)))
    info, ec, et, ew = crowded.tsdf_evict_blocks(centre, radius)
    rinfo, rc_, rt, rw = roomy.tsdf_evict_blocks(centre, radius)
    n_ev, out = ER.evict(hv, centre, radius)
    print("crowded evict: %d of 118 evicted, %d kept, %d moved" % (info["n_evicted"], info["n_blocks"], info["n_moved"]))
    assert info["n_evicted"] == rinfo["n_evicted"] == n_ev and 80 + 12 <= n_ev <= 80 + 26 and all(np.abs(b).max() < 8 for b in hv.blocks)
    assert same_blocks((ec, et, ew), (rc_, rt, rw))
    kept = crowded.tsdf_blocks()[1:]
    assert same_blocks(kept, roomy.tsdf_blocks()[1:]) and same_blocks(kept, hv.sorted_blocks())
    f_after = crowded.tsdf_sample(pts)
    assert same_sample(f_after, SR.sample(hv, pts)) and same_sample(f_after, roomy.tsdf_sample(pts))
    still = f_after[2]
    assert still.sum() > 20 and (f_before[2] & ~still).sum() > 20 and not (still & ~f_before[2]).any()
    assert same_bits(f_after[0][still], f_before[0][still]) and same_bits(f_after[1][still], f_before[1][still])
    gone, _ = TC.block_lattice_points(HC.STRADDLE, ec)
    assert not crowded.tsdf_sample(gone)[2].any()
    mixed = np.concatenate([ec, kept[0][:1]]); mt = np.concatenate([et, kept[1][:1]]); mw = np.concatenate([ew, kept[2][:1]])
    st = binding.IcpTsdfStreamInfo()
    rc = crowded.lib.icp_tsdf_insert_blocks(crowded.h, len(mixed), ptr(mixed), ptr(mt), ptr(mw), C.byref(st))
    assert rc == ERR_INVALID_ARG and st.n_present == 1, (rc, st.n_present, crowded.lib.icp_last_error(crowded.h).decode())
    assert same_blocks(crowded.tsdf_blocks()[1:], kept)
    iinfo = crowded.tsdf_insert_blocks(ec, et, ew)
    assert iinfo["n_inserted"] == len(ec) and iinfo["n_present"] == 0 and iinfo["n_grown"] == 0 and iinfo["capacity"] == 128
    assert same_blocks(crowded.tsdf_blocks()[1:], before) and same_sample(crowded.tsdf_sample(pts), f_before)


def test_evict_all_but_the_wrapping_chain(pair):
    """From the full pool of case 2, a sphere about the corner of the search cube where WRAP lies keeps WRAP's forty blocks and evicts
    ONE_HOME and RUN: the table rebuilt from forty keys with one home is a chain that wraps, and every one of them is found; the presence
    test and the insert then bring the 88 back."""
    from icp_amd import binding
    ctx = pair[0]
    S = TC.sets()
    want, pts, values = full_state(ctx)
    o = np.asarray(TC.DYADIC["origin"], np.float64); s = TC.DYADIC["voxel_size"]
    centre = tuple(float(x) for x in (o + (np.array(TC.LOW) * 8 + 3.5) * s).astype(f32))
    d = np.linalg.norm(o + (S["FULL"] * 8 + 3.5) * s - np.array(centre), axis=1)
    radius = float(f32(0.5 * (d[:40].max() + d[40:].min())))
    keep = ER.kept(S["FULL"], TC.DYADIC["origin"], s, centre, radius)
    assert keep[:40].all() and not keep[40:].any()
    info, ec, et, ew = ctx.tsdf_evict_blocks(centre, radius)
    assert info["n_evicted"] == 88 and info["n_blocks"] == 40 and info["n_held"] == 88, info
    wt, ww = TC.contents(S["WRAP"])
    assert same_blocks(ctx.tsdf_blocks()[1:], TC.sorted_by_key(S["WRAP"], wt, ww))
    in_wrap = np.arange(128) < 40
    F, G, ok = ctx.tsdf_sample(pts)
    assert np.array_equal(ok, in_wrap) and same_bits(F[in_wrap], values[in_wrap]) and not F[~in_wrap].any()
    ctx.tsdf_allocate_blocks(S["WRAP"][::-1])                # found down the rebuilt chain: nothing new
    assert ctx.tsdf_blocks()[0]["n_blocks"] == 40
    mixed = np.concatenate([ec, S["WRAP"][7:8]]); z = np.zeros((len(mixed), 8, 8, 8), f32)
    st = binding.IcpTsdfStreamInfo()
    assert ctx.lib.icp_tsdf_insert_blocks(ctx.h, len(mixed), ptr(mixed), ptr(z), ptr(z), C.byref(st)) == ERR_INVALID_ARG and st.n_present == 1
    iinfo = ctx.tsdf_insert_blocks(ec, et, ew)
    assert iinfo["n_inserted"] == 88 and iinfo["n_blocks"] == 128 and iinfo["n_grown"] == 0 and iinfo["capacity"] == 128, iinfo
    assert same_blocks(ctx.tsdf_blocks()[1:], want)
    F, G, ok = ctx.tsdf_sample(pts)
    assert ok.all() and same_bits(F, values)


def test_raycast_and_mesh_through_a_crowded_table(pair):
    """The ray-cast from HC.TILTED at 64 x 48 and at 7 x 5 and the mesh with normals of the crowded scene equal the roomy volume's bit for
    bit (the mesh is ordered by key, not by pool place), and leave the blocks as they were."""
    crowded, roomy = pair
    crowded_scene(pair)
    before = crowded.tsdf_blocks()
    for w, h in ((HC.W, HC.H), (7, 5)):
        cam, _ = HC.camera(w, h)
        a, b = crowded.tsdf_raycast_hashed(cam, HC.TILTED), roomy.tsdf_raycast_hashed(cam, HC.TILTED)
        print("crowded ray-cast %d x %d: %d hits" % (w, h, a[3]))
        assert a[3] == b[3] > 0 and all(same_bits(x, y) for x, y in zip(a[:3], b[:3]))
    (v, n, tri), (rv, rn, rtri) = crowded.tsdf_mesh_hashed(normals=True), roomy.tsdf_mesh_hashed(normals=True)
    print("crowded mesh: %d vertices, %d triangles" % (len(v), len(tri)))
    assert len(v) > 0 and len(tri) > 0 and same_bits(v, rv) and same_bits(n, rn) and np.array_equal(tri, rtri)
    after = crowded.tsdf_blocks()
    assert after[0] == before[0] and same_blocks(after[1:], before[1:])


def test_colour_through_a_crowded_table(pair):
    """A coloured volume: CROWD uploaded with colours that are a function of the block round-trips; the intensity field over case 5's
    cells, looked up behind the fillers, equals the roomy coloured volume's bit for bit; and so does the coloured ray-cast of the crowded
    scene fused from one coloured frame."""
    crowded, roomy = pair
    cr = TC.crowd()
    cc = np.concatenate([cr["fillers"], cr["junction"]])
    t, w = TC.contents(cc, holes=0.02)
    rgb, cw = TC.colours(cc)
    want = TC.sorted_by_key(cc, t, w, rgb, cw)
    for ctx, cap in zip(pair, (TC.CAPACITY, ROOMY)):
        ctx.tsdf_create_hashed(block_capacity=cap, color=True, **TC.DYADIC)
        ctx.tsdf_upload_blocks(cc, t, w, rgb, cw)
        info, *got = ctx.tsdf_blocks(colors=True)
        assert same_blocks(got, want) and info["n_blocks"] == 120 and info["capacity"] == cap and info["n_grown"] == 0, info
    crowded_junction(pair, color=True)
    pts, cells, cls = TC.junction_cells()
    a, b = crowded.tsdf_sample_color(pts), roomy.tsdf_sample_color(pts)
    print("crowded colour sample: %d of %d valid" % (a[2].sum(), len(pts)))
    assert same_sample(a, b) and a[2].sum() >= 100 and (~a[2]).sum() >= 100 and np.abs(a[0][a[2]]).max() > 0
    assert same_sample(crowded.tsdf_sample(pts), roomy.tsdf_sample(pts))
    crowded_scene(pair, color=True)
    cam, _ = HC.camera()
    a, b = crowded.tsdf_raycast_color_hashed(cam, HC.TILTED), roomy.tsdf_raycast_color_hashed(cam, HC.TILTED)
    print("crowded coloured ray-cast: %d hits, %d coloured" % (a[4], a[5]))
    assert a[4] == b[4] > 0 and a[5] == b[5] > 0 and all(same_bits(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[3], b[3])
    assert same_blocks(crowded.tsdf_blocks(colors=True)[1:], roomy.tsdf_blocks(colors=True)[1:])


# ================================================================================================ part B
def edge_volume(ctx, axis, ends=(+1, -1), trap=True, color=False):
    cc, t, w = TC.edge_blocks(axis, ends, trap)
    ctx.tsdf_create_hashed(block_capacity=TC.CAPACITY, color=color, **TC.EDGE)
    if color:
        rgb, cw = TC.colours(cc)
        ctx.tsdf_upload_blocks(cc, t, w, rgb, np.maximum(cw, f32(1)))
    else:
        ctx.tsdf_upload_blocks(cc, t, w)
    assert same_blocks(ctx.tsdf_blocks()[1:], TC.sorted_by_key(cc, t, w))
    return cc, t, w


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sample_at_the_exact_boundary(pair, axis):
    """Cell 2^23 - 2 is valid and cell 2^23 - 1 is not (F and G read 0), with the trap block in the volume; cell -2^23 is valid and
    -2^23 - 1 is not.  Bit-equal to the restatement (its block-by-block cell: E+, E- and the trap have no common box) and to the same
    volume without the trap; the intensity field of a coloured volume at the same points likewise (with and without the trap)."""
    ctx = pair[0]
    pts, valid, _ = TC.edge_points(axis)
    with_trap = edge_volume(ctx, axis)
    got = ctx.tsdf_sample(pts)
    print("edge sample, axis %d: %d of %d valid" % (axis, got[2].sum(), len(pts)))
    assert np.array_equal(got[2], valid) and not got[0][~valid].view(np.uint32).any() and not got[1][~valid].view(np.uint32).any()
    assert same_sample(got, SR.sample(TC.volume_of(TC.EDGE, *with_trap), pts))
    edge_volume(ctx, axis, trap=False)
    assert same_sample(ctx.tsdf_sample(pts), got)
    colour = []
    for trap in (True, False):
        edge_volume(ctx, axis, trap=trap, color=True)
        colour.append(ctx.tsdf_sample_color(pts))
        assert same_sample(ctx.tsdf_sample(pts), got)
    S, H, ok = colour[0]
    assert np.array_equal(ok, valid) and not S[~valid].view(np.uint32).any() and not H[~valid].view(np.uint32).any() and (S[valid] > 0).all()
    assert same_sample(colour[0], colour[1])


@pytest.mark.parametrize("end", [+1, -1])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_touch_integrate_and_system_across_the_edge(pair, axis, end):
    """A 16 x 12 frame from a pure translation that puts its samples across the edge: the voxels written, the blocks, and the samples out
    of range equal the restatement's; no block lies outside -2^20 .. 2^20 - 1; the sums of one step of the same frame have the
    restatement's counts, lie within the project's bound of its sums, and are the same in a second call."""
    ctx = pair[0]
    cam, rcam = TC.edge_camera()
    depth, pose = TC.edge_frame(axis, end)
    ctx.tsdf_create_hashed(block_capacity=TC.CAPACITY, **TC.EDGE)
    hv = HR.HVolume(**TC.EDGE)
    n = ctx.tsdf_integrate(depth, cam, pose)
    assert n == HR.integrate(hv, depth, rcam, pose) and n > 0
    info, c, t, w = ctx.tsdf_blocks()
    print("edge frame, axis %d end %+d: %d blocks, %d voxels written, n_out_of_range %d" % (axis, end, info["n_blocks"], n, info["n_out_of_range"]))
    assert same_blocks((c, t, w), hv.sorted_blocks())
    assert info["n_out_of_range"] == hv.n_out_of_range > 0 and info["n_unplaced"] == 0 and info["n_grown"] == 0
    assert (c >= TC.B_LO).all() and (c <= TC.B_HI).all() and (c[:, axis] == (TC.B_HI if end > 0 else TC.B_LO)).any()
    sums, counts = ctx.tsdf_sdf_system(depth, cam, pose)
    rcounts, rsums, rabs = SR.system(hv, depth, rcam, pose)
    bound = rcounts[1] * 2.0 ** -52 * rabs
    print("edge system, axis %d end %+d: n_depth %d, n_valid %d, worst |sum - restatement| / bound %.3g"
          % (axis, end, counts[0], counts[1], (np.abs(sums - rsums) / np.maximum(bound, 1e-300)).max()))
    assert tuple(counts) == tuple(rcounts) and (np.abs(sums - rsums) <= bound).all()
    again, counts2 = ctx.tsdf_sdf_system(depth, cam, pose)
    assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts)


@pytest.mark.parametrize("axis", [0, 1])
def test_raycast_through_the_last_cells(pair, axis):
    """A 16 x 12 view from inside E+ along +axis: rays on one half of the image end at the surface inside the block, the others run
    through positive values to the last cell and on out of the storable range.  The image with the trap block in the volume equals the
    image without it and the ray-cast restatement's on E+ alone, bit for bit."""
    ctx = pair[0]
    cam, rcam = TC.edge_camera()
    view = TC.edge_view(axis)
    trace = {}
    ref = RR.raycast(RR.Blocks(*TC.edge_blocks(axis, ends=(+1,), trap=False), **TC.EDGE), rcam, view, trace)
    assert 0 < ref[3] < TC.EDGE_W * TC.EDGE_H and trace["out_of_range"] > 0
    for trap in (True, False):
        edge_volume(ctx, axis, ends=(+1,), trap=trap)
        got = ctx.tsdf_raycast_hashed(cam, view)
        print("edge ray-cast, axis %d, trap %s: %d hits (restatement %d)" % (axis, trap, got[3], ref[3]))
        assert got[3] == ref[3] and all(same_bits(x, y) for x, y in zip(got[:3], ref[:3])), (axis, trap)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_system_at_the_last_cells(pair, axis):
    """The frame of the edge frames stores too few voxels this close to 2^23 for a valid cell, so the sums of a step are also taken on the
    crafted E+: a frame seen from inside the block whose points fall into cells 2^23 - 3 and 2^23 - 2 (valid) and 2^23 - 1 (not
    storable).  Counts equal the restatement's, sums within the project's bound, the same with and without the trap block."""
    ctx = pair[0]
    cam, rcam = TC.edge_camera()
    depth, view = TC.edge_view_frame(), TC.edge_view(axis)
    rcounts, rsums, rabs = SR.system(TC.volume_of(TC.EDGE, *TC.edge_blocks(axis, ends=(+1,), trap=False)), depth, rcam, view)
    assert 30 < rcounts[1] < rcounts[0] - 30
    bound = rcounts[1] * 2.0 ** -52 * rabs
    seen = []
    for trap in (True, False):
        edge_volume(ctx, axis, ends=(+1,), trap=trap)
        sums, counts = ctx.tsdf_sdf_system(depth, cam, view)
        print("edge system on E+, axis %d, trap %s: n_depth %d, n_valid %d, worst |sum - restatement| / bound %.3g"
              % (axis, trap, counts[0], counts[1], (np.abs(sums - rsums) / np.maximum(bound, 1e-300)).max()))
        assert tuple(counts) == tuple(rcounts) and (np.abs(sums - rsums) <= bound).all()
        seen.append(sums)
    assert np.array_equal(u64(seen[0]), u64(seen[1]))


def triangle_rows(v, tri):
    """The triangles as sorted rows of nine coordinates (bit patterns): independent of the vertex numbering."""
    rows = np.ascontiguousarray(v[tri.astype(np.int64)].reshape(-1, 9)).view(np.uint32)
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mesh_does_not_bridge_the_alias(pair, axis):
    """The mesh of {E+, trap} has exactly the vertices and triangles of E+ alone (the trap block is constant and has none of its own; a
    bridge across the alias would add some); the mesh of E- alone, whose lower neighbours do not exist, and of E+ alone are together the
    mesh of E+ and E- in one volume."""
    ctx = pair[0]
    edge_volume(ctx, axis, ends=(+1,), trap=False)
    v, n, tri = ctx.tsdf_mesh_hashed(normals=True)
    print("edge mesh, axis %d: E+ alone %d vertices, %d triangles" % (axis, len(v), len(tri)))
    assert len(v) > 0 and len(tri) > 0
    lo = np.array(TC.edge_block(axis, +1)) * 8
    assert ((v >= lo) & (v <= lo + 7)).all()
    if TC.trap_block(axis) is not None:
        edge_volume(ctx, axis, ends=(+1,), trap=True)
        v2, n2, tri2 = ctx.tsdf_mesh_hashed(normals=True)
        assert same_bits(v, v2) and same_bits(n, n2) and np.array_equal(tri, tri2)
    edge_volume(ctx, axis, ends=(-1,), trap=False)
    vm, nm, trim = ctx.tsdf_mesh_hashed(normals=True)
    lo = np.array(TC.edge_block(axis, -1)) * 8
    assert len(vm) > 0 and ((vm >= lo) & (vm <= lo + 7)).all()
    edge_volume(ctx, axis, trap=False)                       # (x's trap block is E-'s neighbour on y: a true surface lies between them)
    va, na, tria = ctx.tsdf_mesh_hashed(normals=True)
    assert len(va) == len(v) + len(vm) and len(tria) == len(tri) + len(trim)
    both = np.concatenate([triangle_rows(v, tri), triangle_rows(vm, trim)])
    assert np.array_equal(triangle_rows(va, tria), both[np.lexsort(both.T[::-1])])
