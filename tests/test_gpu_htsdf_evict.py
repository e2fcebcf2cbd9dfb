"""Streaming the hashed TSDF volume on the device (icp_tsdf_evict_blocks, icp_tsdf_evicted_blocks, icp_tsdf_insert_blocks,
tsdf_local.track_depth_sdf_local): the evict on the exact lattice against the numpy restatement
(tests/htsdf_evict_restatement.py); the identity the feature rests on with EXISTING code as the reference -- after an evict every public
call returns the bits it returns on a fresh volume that tsdf_upload_blocks filled with the kept blocks -- over the pool sizes and patterns
at which the compaction takes another path; the clean tail; insert; the local loop against the unbounded one bit for bit; the refusals."""
import ctypes as C
import json
import os
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_restatement as HR
import htsdf_evict_restatement as ER
import htsdf_evict_fixture as EF
import test_htsdf_evict_host as EH
from icp_amd.synth import camera_sequence, wavy_depth
from support import same_bits

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
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def sort_blocks(coords, t, w):
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    order = np.lexsort((coords[:, 0], coords[:, 1], coords[:, 2]))
    return coords[order], np.asarray(t, f32).reshape(-1, 8, 8, 8)[order], np.asarray(w, f32).reshape(-1, 8, 8, 8)[order]


def hv_blocks(d):
    """{coords: [t, w]} in icp_get_tsdf_hashed's layout."""
    keys = sorted(d, key=lambda b: (b[2], b[1], b[0]))
    if not keys:
        return np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), f32), np.zeros((0, 8, 8, 8), f32)
    return np.array(keys, np.int32), np.stack([d[b][0] for b in keys]), np.stack([d[b][1] for b in keys])


@pytest.mark.parametrize("radius,n_keep", [(1.5, 123), (0.0, 1), (2e19, 729)])
def test_lattice_against_restatement(gpu_ctx_factory, radius, n_keep):
    """The 9 x 9 x 9 lattice of tests/test_htsdf_evict_host.py, uploaded into a pool of 1024 blocks: resident and evicted are disjoint,
    their union is what was there bit for bit, each is the restatement's set, the info matches; with r2 infinite nothing is modified."""
    hv, cc = EH.lattice_volume()
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(block_capacity=1024, **EH.LATTICE)
    before = hv.sorted_blocks()
    ctx.tsdf_upload_blocks(*before)
    info0 = ctx.tsdf_blocks()[0]
    n_ev, out = ER.evict(hv, EH.LATTICE_CENTRE, radius)
    info, ec, et, ew = ctx.tsdf_evict_blocks(EH.LATTICE_CENTRE, radius)
    binfo, *res = ctx.tsdf_blocks()
    print("lattice radius %g: %s" % (radius, info))
    assert info["n_evicted"] == n_ev == 729 - n_keep and info["n_blocks"] == n_keep == binfo["n_blocks"] and info["n_held"] == n_ev and len(ec) == n_ev
    assert info["capacity"] == 1024 == binfo["capacity"] and binfo["n_grown"] == info0["n_grown"] == info["n_grown"] and binfo["n_unplaced"] == 0
    assert 0 <= info["n_moved"] <= min(n_keep, n_ev) and info["n_inserted"] == 0 and info["n_present"] == 0
    assert same_blocks(res, hv.sorted_blocks()) and same_blocks((ec, et, ew), hv_blocks(out))
    assert not ({tuple(b) for b in ec.tolist()} & {tuple(b) for b in res[0].tolist()})
    assert same_blocks(sort_blocks(np.concatenate([res[0], ec]), np.concatenate([res[1], et]), np.concatenate([res[2], ew])), before)
    if n_ev == 0:
        assert info["n_moved"] == 0 and binfo == info0
    # a second evict with the same sphere removes nothing and empties the outbox
    again, ac, _, _ = ctx.tsdf_evict_blocks(EH.LATTICE_CENTRE, radius)
    assert again["n_evicted"] == 0 and again["n_moved"] == 0 and again["n_held"] == 0 and len(ac) == 0 and again["n_blocks"] == n_keep
    assert same_blocks(ctx.tsdf_blocks()[1:], res)


# ---- the identity, with existing code as the reference ----
CENTRE = (0.25, 0.15, 1.3)                          # HC.STRADDLE's origin: the scene's blocks lie within a few blocks of it
RADIUS = 9.0                                        # 11 blocks of 0.8 m: the scene and the near filler are inside, the far filler (x + 100 blocks) outside
PATTERNS = ("all kept", "all evicted", "last evicted", "first evicted", "alternating")


@pytest.fixture(scope="module")
def scene(gpu_ctx_factory):
    """Three fused frames in HC.STRADDLE (real surface content), then filler blocks with crafted content: near ones (kept) and far ones
    (evicted).  Computed once and left unchanged: (scene blocks, near filler, far filler), each a list of (coords, t, w)."""
    ctx = gpu_ctx_factory()
    cam, _ = HC.camera()
    ctx.tsdf_create_hashed(**HC.STRADDLE)
    for depth, pose in zip(HC.frames(), HC.POSES):
        ctx.tsdf_integrate(depth, cam, pose)
    _, sc, st, sw = ctx.tsdf_blocks()
    ctx.tsdf_release()
    have = {tuple(b) for b in sc.tolist()}
    rng = np.random.default_rng(23)
    near = [b for b in HC.box_coords((-5, -5, -5), (10, 10, 10)).tolist() if tuple(b) not in have][:600]
    far = (HC.box_coords((-5, -5, -5), (10, 10, 10))[:600] + np.array([100, 0, 0])).tolist()
    k = ER.kept(np.array(near + far), HC.STRADDLE["origin"], HC.STRADDLE["voxel_size"], CENTRE, RADIUS)
    assert k[:len(near)].all() and not k[len(near):].any()
    assert ER.kept(sc, HC.STRADDLE["origin"], HC.STRADDLE["voxel_size"], CENTRE, RADIUS).all()

    def crafted(n):
        t = rng.uniform(-1, 1, (n, 8, 8, 8)).astype(f32); w = rng.integers(0, 4, (n, 8, 8, 8)).astype(f32)
        return t, w
    nt, nw = crafted(len(near)); ft, fw = crafted(len(far))
    blocks = lambda cc, t, w: [(tuple(c), t[i], w[i]) for i, c in enumerate(cc)]
    return blocks(sc.tolist(), st, sw), blocks(near, nt, nw), blocks(far, ft, fw)


def pool_layout(scene, n, pattern):
    """n blocks in pool order, and which of them the evict keeps: kept places take the scene's blocks first, then near filler; evicted
    places take far filler."""
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
    """Points in cells of every class around the kept blocks: inside one block, across a face, an edge, a corner (local coordinate 7 on 0 .. 3 axes)."""
    o, s = np.array(HC.STRADDLE["origin"], f32), f32(HC.STRADDLE["voxel_size"])
    if len(kept_coords) == 0:
        kept_coords = np.zeros((1, 3), np.int32)
    base = kept_coords[rng.integers(0, len(kept_coords), 400)].astype(np.int64) * 8
    cells = base + rng.integers(0, 7, (400, 3))
    for i in range(400):
        cells[i, rng.permutation(3)[:i % 4]] |= 7
    frac = rng.integers(0, 64, cells.shape).astype(f32) / f32(64)
    return (o + (cells.astype(f32) + frac) * s).astype(f32)


def assert_same_state(a, b, what):
    """Every public call that reads the volume returns identical bits on both contexts; then one more integrate, and the blocks again."""
    cam, _ = HC.camera()
    ai, *ab = a.tsdf_blocks(); bi, *bb = b.tsdf_blocks()
    assert same_blocks(ab, bb), what
    assert ai["n_blocks"] == bi["n_blocks"] and ai["n_unplaced"] == bi["n_unplaced"] == 0, what
    pts = sample_points(ab[0], np.random.default_rng(3))
    fa, fb = a.tsdf_sample(pts), b.tsdf_sample(pts)
    assert same_bits(fa[0], fb[0]) and same_bits(fa[1], fb[1]) and np.array_equal(fa[2], fb[2]), what
    frame = HC.crafted_frame()
    for stride in (1, 3):
        sa, ca = a.tsdf_sdf_system(frame, cam, HC.TILTED, stride=stride); sb, cb = b.tsdf_sdf_system(frame, cam, HC.TILTED, stride=stride)
        assert np.array_equal(u64(sa), u64(sb)) and tuple(ca) == tuple(cb), what
    ma, mb = a.tsdf_mesh_hashed(), b.tsdf_mesh_hashed()
    assert same_bits(ma[0], mb[0]) and same_bits(ma[1], mb[1]) and np.array_equal(ma[2], mb[2]), what
    ra, rb = a.tsdf_raycast_hashed(cam, HC.TILTED), b.tsdf_raycast_hashed(cam, HC.TILTED)
    assert all(same_bits(x, y) for x, y in zip(ra[:3], rb[:3])) and ra[3] == rb[3], what
    na, nb = a.tsdf_integrate(wavy_depth(HC.W, HC.H, 1.4), cam, HC.POSES[2]), b.tsdf_integrate(wavy_depth(HC.W, HC.H, 1.4), cam, HC.POSES[2])
    assert na == nb and same_blocks(a.tsdf_blocks()[1:], b.tsdf_blocks()[1:]), what
    return fa[2].sum(), len(ma[2]), ra[3]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_evict_equals_a_fresh_upload_of_the_kept_blocks(gpu_ctx_factory, scene, n):
    """A pool of n blocks whose ORDER is known (one block per insert call), evicted by the five patterns: afterwards the context equals a fresh
    one that tsdf_upload_blocks filled with the kept blocks -- through tsdf_blocks, tsdf_sample, tsdf_sdf_system, tsdf_mesh_hashed,
    tsdf_raycast_hashed and one more tsdf_integrate, bit for bit -- the evicted blocks come back as they were, and n_moved is the number of
    kept blocks at or above n_keep."""
    ctx, ref = gpu_ctx_factory(), gpu_ctx_factory()
    for pattern in PATTERNS:
        layout, keep = pool_layout(scene, n, pattern)
        ctx.tsdf_create_hashed(block_capacity=16, **HC.STRADDLE)
        for c, t, w in layout:
            ctx.tsdf_insert_blocks([c], t[None], w[None])
        info0 = ctx.tsdf_blocks()[0]
        assert info0["n_blocks"] == n
        info, ec, et, ew = ctx.tsdf_evict_blocks(CENTRE, RADIUS)
        n_keep = int(keep.sum())
        kept = sort_blocks(*[np.array([b[j] for b, k in zip(layout, keep) if k]).reshape((-1,) + s) for j, s in ((0, (3,)), (1, (8, 8, 8)), (2, (8, 8, 8)))])
        gone = sort_blocks(*[np.array([b[j] for b, k in zip(layout, keep) if not k]).reshape((-1,) + s) for j, s in ((0, (3,)), (1, (8, 8, 8)), (2, (8, 8, 8)))])
        assert info["n_evicted"] == n - n_keep == info["n_held"] and info["n_blocks"] == n_keep and info["capacity"] == info0["capacity"] and info["n_grown"] == info0["n_grown"], (pattern, info)
        assert info["n_moved"] == (int(keep[n_keep:].sum()) if n_keep < n else 0), (pattern, info)
        assert same_blocks((ec, et, ew), gone), pattern
        ref.tsdf_create_hashed(block_capacity=16, **HC.STRADDLE)
        ref.tsdf_upload_blocks(*kept)
        valid, tris, hits = assert_same_state(ctx, ref, (n, pattern))
        print("n %d, %s: %d evicted, %d moved; %d valid samples, %d triangles, %d ray-cast hits" % (n, pattern, info["n_evicted"], info["n_moved"], valid, tris, hits))
        if n >= 63 and pattern != "all evicted":
            assert valid > 20 and tris > 100
        if n >= 255 and pattern == "all kept":
            assert hits > 100                           # (the whole scene is among the kept blocks)


def test_clean_tail(gpu_ctx_factory):
    """Evict, then integrate a frame that allocates blocks again, evicted keys among them: blocks and contents equal the restatement's bit
    for bit (an evicted key reads what ONE frame writes, not its old content), also from a pool that starts at one block and grows after
    the evict; and an evicted key that is allocated by hand reads zero."""
    cam, rcam = HC.camera()
    cam7, rcam7 = HC.camera(7, 5)
    first_big = [(d, cam, rcam, p) for d, p in list(zip(HC.frames(), HC.POSES))[:2]]
    first_small = [(wavy_depth(7, 5), cam7, rcam7, HC.TILTED)]
    for cap, first, (depth, pose) in ((1 << 10, first_big, (HC.frames()[2], HC.POSES[2])), (1, first_small, (HC.crafted_frame(), HC.TILTED))):
        ctx = gpu_ctx_factory()
        ctx.tsdf_create_hashed(block_capacity=cap, **HC.STRADDLE)
        hv = HR.HVolume(**HC.STRADDLE)
        for d, c, rc_, p in first:
            ctx.tsdf_integrate(d, c, p); HR.integrate(hv, d, rc_, p)
        n_before = len(hv.blocks)
        n_ev, out = ER.evict(hv, CENTRE, 1.0)
        info, ec, et, ew = ctx.tsdf_evict_blocks(CENTRE, 1.0, hold=(cap == 1))
        assert 0 < n_ev == info["n_evicted"] < n_before and info["n_held"] == (n_ev if cap == 1 else 0) and len(ec) == info["n_held"]
        grown = info["n_grown"]
        assert ctx.tsdf_integrate(depth, cam, pose) == HR.integrate(hv, depth, rcam, pose)
        binfo, bc, bt, bw = ctx.tsdf_blocks()
        assert same_blocks((bc, bt, bw), hv.sorted_blocks()) and binfo["n_unplaced"] == 0
        back = set(out) & set(hv.blocks)
        print("clean tail (capacity %d): %d of %d evicted, %d of them allocated again by the next frame, max weight there %g, %d growths after the evict" %
              (cap, n_ev, n_before, len(back), max(hv.blocks[b][1].max() for b in back), binfo["n_grown"] - grown))
        assert len(back) >= 1 and all(hv.blocks[b][1].max() <= 1 for b in back) and bw.max() >= 2
        assert binfo["n_grown"] > grown if cap == 1 else binfo["n_grown"] == grown == 0
    small = gpu_ctx_factory()
    small.tsdf_create_hashed(block_capacity=1, **HC.STRADDLE)
    small.tsdf_integrate(HC.crafted_frame(), cam, HC.TILTED)
    before = small.tsdf_blocks()
    info, ec, et, ew = small.tsdf_evict_blocks(CENTRE, 0.0, hold=True)
    assert info["n_evicted"] == before[0]["n_blocks"] and info["n_blocks"] == 0 and et.any()
    small.tsdf_reserve_blocks(4 * info["capacity"])      # growth after the evict carries nothing stale
    small.tsdf_allocate_blocks(ec)
    ai, ac, at, aw = small.tsdf_blocks()
    assert np.array_equal(ac, ec) and not at.any() and not aw.any() and ai["n_grown"] == before[0]["n_grown"] + 1
    assert not small.tsdf_sample(sample_points(ec, np.random.default_rng(1)))[2].any()


def test_insert(gpu_ctx_factory):
    cam, _ = HC.camera()
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(block_capacity=64, **HC.STRADDLE)
    for depth, pose in zip(HC.frames(), HC.POSES):
        ctx.tsdf_integrate(depth, cam, pose)
    binfo, *before = ctx.tsdf_blocks()
    info, ec, et, ew = ctx.tsdf_evict_blocks(CENTRE, 1.0)
    assert 5 < info["n_evicted"] < binfo["n_blocks"] - 5
    kept = ctx.tsdf_blocks()[1:]
    # a resident key refuses the call: counted, reported, nothing modified
    mixed = np.concatenate([ec[:4], kept[0][:3]])
    st = binding_info()
    rc = ctx.lib.icp_tsdf_insert_blocks(ctx.h, 7, ptr(mixed), ptr(np.zeros((7, 8, 8, 8), f32)), ptr(np.zeros((7, 8, 8, 8), f32)), C.byref(st))
    msg = ctx.lib.icp_last_error(ctx.h).decode()
    assert rc == ERR_INVALID_ARG and st.n_present == 3 and "3 of the 7" in msg and "icp_tsdf_insert_blocks" in msg, (rc, msg)
    assert same_blocks(ctx.tsdf_blocks()[1:], kept)
    # a repeated key and a coordinate that is not storable
    twice = np.concatenate([ec[:2], ec[:1]])
    assert ctx.lib.icp_tsdf_insert_blocks(ctx.h, 3, ptr(twice), ptr(et[:3]), ptr(ew[:3]), None) == ERR_INVALID_ARG and "twice" in ctx.lib.icp_last_error(ctx.h).decode()
    bad = np.array([[0, -(1 << 20) - 1, 0]], np.int32)
    assert ctx.lib.icp_tsdf_insert_blocks(ctx.h, 1, ptr(bad), ptr(et[:1]), ptr(ew[:1]), None) == ERR_INVALID_ARG and "storable" in ctx.lib.icp_last_error(ctx.h).decode()
    assert same_blocks(ctx.tsdf_blocks()[1:], kept)
    # too small a max_blocks names both numbers; the outbox is still there
    assert ctx.lib.icp_tsdf_evicted_blocks(ctx.h, len(ec) - 1, ptr(np.zeros_like(ec)), None, None) == ERR_INVALID_ARG
    msg = ctx.lib.icp_last_error(ctx.h).decode()
    assert str(len(ec) - 1) in msg and str(len(ec)) in msg and "icp_tsdf_evicted_blocks" in msg
    c2 = np.zeros_like(ec); t2 = np.zeros_like(et); w2 = np.zeros_like(ew)
    assert ctx.lib.icp_tsdf_evicted_blocks(ctx.h, len(ec) + 5, ptr(c2), ptr(t2), ptr(w2)) == 0 and same_blocks((c2, t2, w2), (ec, et, ew))
    # the evicted blocks inserted back: the original volume bit for bit
    iinfo = ctx.tsdf_insert_blocks(ec[::-1], et[::-1], ew[::-1])
    assert iinfo["n_inserted"] == len(ec) and iinfo["n_blocks"] == binfo["n_blocks"] and iinfo["n_present"] == 0
    assert same_blocks(ctx.tsdf_blocks()[1:], before)
    # hold=False leaves an empty outbox
    info2, e2, _, _ = ctx.tsdf_evict_blocks(CENTRE, 1.0, hold=False)
    assert info2["n_evicted"] == info["n_evicted"] and info2["n_held"] == 0 and len(e2) == 0
    assert ctx.lib.icp_tsdf_evicted_blocks(ctx.h, 0, ptr(c2), ptr(t2), ptr(w2)) == 0
    # an insert that forces a growth, into a small pool, beside resident blocks
    small = gpu_ctx_factory()
    small.tsdf_create_hashed(block_capacity=2, **HC.STRADDLE)
    small.tsdf_insert_blocks(kept[0][:2], kept[1][:2], kept[2][:2])
    assert small.tsdf_blocks()[0]["n_grown"] == 0
    ginfo = small.tsdf_insert_blocks(np.concatenate([kept[0][2:], ec]), np.concatenate([kept[1][2:], et]), np.concatenate([kept[2][2:], ew]))
    assert ginfo["n_grown"] >= 4 and ginfo["capacity"] >= ginfo["n_blocks"] == binfo["n_blocks"]
    assert same_blocks(small.tsdf_blocks()[1:], before)
    pts = sample_points(before[0], np.random.default_rng(9))
    ctx.tsdf_insert_blocks(ec, et, ew)                  # (forgotten by hold=False: put back)
    fa, fb = small.tsdf_sample(pts), ctx.tsdf_sample(pts)
    assert same_bits(fa[0], fb[0]) and same_bits(fa[1], fb[1]) and np.array_equal(fa[2], fb[2]) and fa[2].sum() > 20


def ptr(a):
    from icp_amd import binding
    return binding._ptr(a)


def binding_info():
    from icp_amd import binding
    return binding.IcpTsdfStreamInfo()


def test_local_loop_with_everything_in_reach(gpu_ctx_factory):
    """keep_radius 1e6 on the 5-frame 40 x 30 case of the composition test (frame 2 all MINF): poses, records, status and blocks equal
    track_depth_sdf's bit for bit; nothing is ever evicted, and the failed frame's evict record is all zero."""
    from icp_amd import binding, tsdf_local
    K, depth, _, gt = camera_sequence(5, 40, 30)
    depth[2][:] = MINF
    cam = binding.depth_camera(K, 40, 30)
    opts = dict(origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.tsdf_create_hashed(block_capacity=16, **opts)
    kw = dict(stride=1, n_iterations=12)
    pose, recs, rc = a.track_depth_sdf(depth, cam, **kw)
    lpose, lrecs, lrc, evs, store = tsdf_local.track_depth_sdf_local(b, depth, cam, 1e6, **kw)
    assert len(lrecs) == 4 and lrc == rc == ERR_NO_SOURCE and same_bits(pose, lpose)
    for k, (r, h) in enumerate(zip(recs, lrecs)):
        assert same_record(r, h), (k, r, h)
    assert same_blocks(a.tsdf_blocks()[1:], b.tsdf_blocks()[1:]) and len(store) == 0
    assert len(evs) == 5 and evs[2] == dict.fromkeys(tsdf_local.EVICT_RECORD, 0) and all(e["n_evicted"] == 0 and e["n_inserted"] == 0 for e in evs)
    assert [e["n_resident"] > 0 for e in evs] == [True, True, False, True, True]


@pytest.fixture(scope="module")
def unbounded(gpu_ctx_factory):
    """track_depth_sdf on the fixture's frames on an unbounded hashed volume: (pose, records, blocks, mesh), computed once."""
    from icp_amd import binding
    K, depth, _ = EF.frames()
    cam = binding.depth_camera(K, EF.W, EF.H)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(block_capacity=16, **EF.VOLUME)
    pose, recs, rc = ctx.track_depth_sdf(depth, cam, **EF.OPTIONS)
    out = dict(pose=pose, recs=recs, rc=rc, blocks=ctx.tsdf_blocks(), mesh=ctx.tsdf_mesh_hashed(), depth=depth, cam=cam, K=K)
    ctx.tsdf_release()
    return out


def test_local_loop_on_the_fixture(gpu_ctx_factory, unbounded):
    """The out-and-back slide of tests/htsdf_evict_fixture.py with keep_radius = reach + twice the step: poses and records equal the
    unbounded run's bit for bit, `restore` gives its blocks bit for bit, store and device never share a key, and the per-frame evicted,
    inserted and resident counts and the peak equal the restatement's (tests/golden/htsdf_evict_outcome.json)."""
    from icp_amd import tsdf_local
    with open(EF.GOLDEN) as f:
        gold = json.load(f)
    u = unbounded
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(block_capacity=16, **EF.VOLUME)
    pose, recs, rc, evs, store = tsdf_local.track_depth_sdf_local(ctx, u["depth"], u["cam"], gold["keep_radius"], **EF.OPTIONS)
    peak = max(e["n_resident"] + e["n_evicted"] for e in evs)
    print("local loop: evicted %s, inserted %s, moved %s, peak %d of %d blocks, capacity %d" %
          ([e["n_evicted"] for e in evs], [e["n_inserted"] for e in evs], [e["n_moved"] for e in evs], peak, u["blocks"][0]["n_blocks"], evs[-1]["capacity"]))
    assert rc == u["rc"] == 0 and same_bits(pose, u["pose"]) and len(recs) == len(u["recs"]) == gold["frames"] - 1
    for k, (r, h) in enumerate(zip(recs, u["recs"])):
        assert same_record(r, h), (k, r, h)
    for key in ("n_evicted", "n_inserted", "n_resident", "n_stored"):
        assert [e[key] for e in evs] == gold[key], key
    assert peak == gold["peak_resident"] and u["blocks"][0]["n_blocks"] == gold["total_blocks"] and evs[-1]["capacity"] == 128
    resident = {tuple(b) for b in ctx.tsdf_blocks()[1].tolist()}
    assert not (resident & {tuple(b) for b in store.blocks()[0].tolist()}) and len(resident) + len(store) == gold["total_blocks"]
    assert tsdf_local.restore(ctx, store) == gold["total_blocks"]
    assert same_blocks(ctx.tsdf_blocks()[1:], u["blocks"][1:])
    mesh = ctx.tsdf_mesh_hashed()
    assert same_bits(mesh[0], u["mesh"][0]) and same_bits(mesh[1], u["mesh"][1]) and np.array_equal(mesh[2], u["mesh"][2]) and len(mesh[2]) > 1000


def test_local_loop_fits_where_the_unbounded_one_is_refused(gpu_ctx_factory, unbounded):
    """The maximum lowered to 2^7 blocks (the hook of tests/test_gpu_htsdf.py): track_depth_sdf is refused mid-track, the local loop
    finishes with the unbounded run's poses."""
    from icp_amd import binding, tsdf_local
    u = unbounded
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.tsdf_create_hashed(block_capacity=16, **EF.VOLUME)
        assert c.lib.icp_debug_htsdf_max_blocks(c.h, 7) == 0
    with pytest.raises(binding.IcpError) as e:
        a.track_depth_sdf(u["depth"], u["cam"], **EF.OPTIONS)
    assert "2^7 blocks" in str(e.value)
    assert a.tsdf_blocks()[0]["n_blocks"] <= 128 < u["blocks"][0]["n_blocks"]
    keep = EF.model()["keep_radius"]
    pose, recs, rc, evs, store = tsdf_local.track_depth_sdf_local(b, u["depth"], u["cam"], keep, **EF.OPTIONS)
    assert rc == 0 and same_bits(pose, u["pose"]) and all(same_record(r, h) for r, h in zip(recs, u["recs"]))
    assert b.tsdf_blocks()[0]["capacity"] <= 128 and len(store) + b.tsdf_blocks()[0]["n_blocks"] == u["blocks"][0]["n_blocks"]
    for c in (a, b):
        assert c.lib.icp_debug_htsdf_max_blocks(c.h, 22) == 0


def test_through_tum(tmp_path, gpu_ctx_factory, unbounded):
    """tum.track and tum.reconstruct_room(densify=False) with keep_radius in the model: the unbounded run's poses, and the mesh of the
    whole model (restored from the store) as the file."""
    from icp_amd import meshio, tum
    u = unbounded
    n = len(u["depth"])
    seq = dict(depth=u["depth"], rgbx=np.zeros((n, EF.W * EF.H, 4), np.uint8), gt=None, K=u["K"], width=EF.W, height=EF.H, frames=list(range(n)))
    ctx = gpu_ctx_factory()
    poses, recs, rc = tum.track(ctx, seq, with_gt=False, model=EF.model(), sdf=dict(EF.OPTIONS))
    assert rc == 0 and len(poses) == n and all(same_record(r, h) for r, h in zip(recs, u["recs"]))
    assert len(ctx.tsdf_store) > 0 and ctx.tsdf_blocks()[0]["n_blocks"] + len(ctx.tsdf_store) == u["blocks"][0]["n_blocks"]
    out = str(tmp_path / "out")
    _, recs2, rc2, paths = tum.reconstruct_room(ctx, seq, out_dir=out, with_gt=False, model=EF.model(), sdf=dict(EF.OPTIONS), model_mesh="m.ply", densify=False)
    assert rc2 == 0 and len(paths) == n and os.path.exists(os.path.join(out, "m.ply"))
    v, nr, t = meshio.load_ply_mesh(os.path.join(out, "m.ply"))
    assert same_bits(v, u["mesh"][0]) and np.array_equal(t, u["mesh"][2])
    assert ctx.tsdf_blocks()[0]["n_blocks"] == u["blocks"][0]["n_blocks"]
    # keep_radius=None, the default, changes nothing: the unbounded path
    plain = gpu_ctx_factory()
    m = {k: v for k, v in EF.model().items() if k != "keep_radius"}
    _, recs3, rc3 = tum.track(plain, seq, with_gt=False, model=m, sdf=dict(EF.OPTIONS))
    assert rc3 == 0 and plain.tsdf_store is None and all(same_record(r, h) for r, h in zip(recs3, u["recs"])) and same_blocks(plain.tsdf_blocks()[1:], u["blocks"][1:])


def test_refusals_leave_the_state_alone(gpu_ctx_factory):
    """No volume, a dense volume, a NaN centre, a negative radius, a null centre: ICP_ERR_INVALID_ARG with a message that names the call,
    nothing modified (the outbox included); and a context that made every new call and then created its volume again returns the same
    bytes as a fresh one."""
    from icp_amd import binding
    cam, _ = HC.camera()
    ctx, fresh = gpu_ctx_factory(), gpu_ctx_factory()
    lib, h = ctx.lib, ctx.h
    ce = np.array(CENTRE, f32); one = np.zeros((1, 3), np.int32); z = np.zeros((1, 8, 8, 8), f32)
    calls = {"icp_tsdf_evict_blocks": lambda: lib.icp_tsdf_evict_blocks(h, ptr(ce), C.c_float(1.0), 1, None),
             "icp_tsdf_evicted_blocks": lambda: lib.icp_tsdf_evicted_blocks(h, 1, ptr(one), None, None),
             "icp_tsdf_insert_blocks": lambda: lib.icp_tsdf_insert_blocks(h, 1, ptr(one), ptr(z), ptr(z), None)}
    for name, call in calls.items():
        assert call() == ERR_INVALID_ARG and "no volume" in lib.icp_last_error(h).decode() and name in lib.icp_last_error(h).decode(), name
    ctx.tsdf_create(dims=HC.BOX_DIMS, **HC.BOX)
    ctx.tsdf_integrate(HC.crafted_frame(), cam, np.eye(4, dtype=f32))
    dense = ctx.tsdf_volume()
    for name, call in calls.items():
        assert call() == ERR_INVALID_ARG and "dense" in lib.icp_last_error(h).decode() and name in lib.icp_last_error(h).decode(), name
    after = ctx.tsdf_volume()
    assert same_bits(dense[0], after[0]) and same_bits(dense[1], after[1])
    ctx.tsdf_create_hashed(**HC.STRADDLE)
    for depth, pose in zip(HC.frames(), HC.POSES):
        ctx.tsdf_integrate(depth, cam, pose)
    info, ec, et, ew = ctx.tsdf_evict_blocks(CENTRE, 1.0)
    before = ctx.tsdf_blocks()
    assert info["n_held"] > 5
    st = binding.IcpTsdfStreamInfo()
    for centre, radius, word in (((np.nan, 0, 0), 1.0, "centre"), ((0, np.inf, 0), 1.0, "centre"), (CENTRE, -1.0, "radius"), (CENTRE, np.nan, "radius"), (CENTRE, np.inf, "radius")):
        bad = np.array(centre, f32)
        assert lib.icp_tsdf_evict_blocks(h, ptr(bad), C.c_float(radius), 1, C.byref(st)) == ERR_INVALID_ARG and word in lib.icp_last_error(h).decode()
    assert lib.icp_tsdf_evict_blocks(h, None, C.c_float(1.0), 1, None) == ERR_INVALID_ARG
    assert lib.icp_tsdf_insert_blocks(h, -1, None, None, None, None) == ERR_INVALID_ARG and lib.icp_tsdf_insert_blocks(h, 1, ptr(one), None, ptr(z), None) == ERR_INVALID_ARG
    after = ctx.tsdf_blocks()
    assert after[0] == before[0] and same_blocks(after[1:], before[1:])
    c2 = np.zeros_like(ec); t2 = np.zeros_like(et); w2 = np.zeros_like(ew)
    assert lib.icp_tsdf_evicted_blocks(h, len(ec), ptr(c2), ptr(t2), ptr(w2)) == 0 and same_blocks((c2, t2, w2), (ec, et, ew))      # the outbox too
    # reset, release, create and upload end the outbox
    ctx.tsdf_reset()
    assert lib.icp_tsdf_evicted_blocks(h, 0, ptr(c2), ptr(t2), ptr(w2)) == 0
    # a context that made every new call, with its volume created again, against a fresh one
    ctx.tsdf_insert_blocks(ec, et, ew)
    ctx.tsdf_evict_blocks(CENTRE, 0.5)
    for c in (ctx, fresh):
        c.tsdf_create_hashed(**HC.STRADDLE)
        for depth, pose in zip(HC.frames(), HC.POSES):
            c.tsdf_integrate(depth, cam, pose)
    assert lib.icp_tsdf_evicted_blocks(h, 0, ptr(c2), ptr(t2), ptr(w2)) == 0
    assert ctx.tsdf_blocks()[0] == fresh.tsdf_blocks()[0] and same_blocks(ctx.tsdf_blocks()[1:], fresh.tsdf_blocks()[1:])
    pa, pb = ctx.track_depth_sdf(np.stack(HC.frames()), cam, stride=2, n_iterations=5), fresh.track_depth_sdf(np.stack(HC.frames()), cam, stride=2, n_iterations=5)
    assert same_bits(pa[0], pb[0]) and all(same_record(r, q) for r, q in zip(pa[1], pb[1]))
