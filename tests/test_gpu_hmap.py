"""The hashed voxel map on the device.  Two references: EXISTING CODE -- the dense voxel map over a covering extent, given the same inserts on
the same device, whose occupied cells the hashed map's sorted entries must equal bit for bit -- and the numpy restatement of the contract
(tests/hmap_restatement.py).  Inserts at poses, in both orders and at block-edge sizes, crafted probe chains (wrapping, one home slot, a
run of consecutive homes), the ends of the storable range, growth with content in the table, the upload round trip, the refusals, the
sums of a step and every step of an alignment, tracking from a 256-slot table against the dense loop, the case the feature exists for (a
trajectory that leaves a dense extent), the recorded outcome, and the paths that must stay untouched."""
import ctypes as C
import functools
import json
import numpy as np
import pytest

import support as S
import vgicp_restatement as VR
import vmap_restatement as MR
import hmap_restatement as HR
import vmap_outcome_fixture as MF
from support import pose_of, same_bits

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = 1, 3, 4, 8
N = 4101
EPS = 1e-3
POSE_A = ((0.05, -0.04, 0.3), (0.4, -0.3, 0.2))
POSE_B = ((-0.1, 0.08, -0.25), (-0.35, 0.2, 0.1))
EYE = np.eye(4, dtype=f32)
COVER = ((-40, -12, -8), (50, 50, 30))             # a dense extent around everything the crafted cloud reaches at these poses (cells -36 .. 7, -9 .. 35, -6 .. 19 at 0.25 m)


def u64(a):
    return np.ascontiguousarray(a, dtype=f64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def crafted():
    """4101 points with normals in scan order (rows of 59 points over a tilted, wavy sheet), and in it:
      [40, 340)     300 consecutive points of ONE cell at voxel sizes 0.25 and 0.3: the run crosses the wave boundaries 64 .. 320 and the block boundary 256
      [500, 540)    40 points of one cell across the block boundary 512
      [600, 680)    dyadic coordinates (multiples of 1/8: on cell faces at 0.25), negative ones among them
      [700, 712)    single-point cells, far from everything else
      [720, 728)    positions with NaN / +inf / -inf; [728, 732) NaN normals; 732, 733 an infinite normal component: all stay out
      4100          the last point, alone in the last (partial) block
    Returned read-only: (points, normals)."""
    r = np.random.default_rng(2024)
    k = np.arange(N)
    row, col = k // 59, k % 59
    x = -1.3 + col * (2.5 / 59) + r.normal(0, 0.002, N); y = -1.1 + row * (2.3 / 70) + r.normal(0, 0.002, N)
    z = 0.2 * np.sin(2.2 * x) + 0.25 * np.cos(1.8 * y) + 0.15 * x
    n = np.stack([-0.44 * np.cos(2.2 * x) - 0.15, 0.45 * np.sin(1.8 * y), np.ones(N)], 1) + r.normal(0, 0.02, (N, 3))
    pts = np.stack([x, y, z], 1)
    pts[40:340] = (0.67, -0.66, 0.67) + r.uniform(-0.02, 0.02, (300, 3))
    pts[500:540] = (-0.41, 0.40, -0.40) + r.uniform(-0.02, 0.02, (40, 3))
    pts[600:680] = r.integers(-11, 12, (80, 3)) / 8.0
    pts[700:712] = np.array([-3.1, 2.4, 1.3]) + np.arange(12)[:, None] * np.array([-0.41, 0.37, 0.33])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    pts = pts.astype(f32); n = n.astype(f32)
    pts[720:728] = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (np.nan, np.nan, np.nan), (np.inf, -np.inf, 0), (-np.inf, 1, 1), (1, np.nan, 1), (1, 1, np.inf)], f32)
    n[728:732] = np.array([(np.nan, 0, 1), (0, np.nan, 0), (0, 0, np.nan), (np.nan, np.nan, np.nan)], f32)
    n[732] = (0, np.inf, 1); n[733] = (-np.inf, 0, 0)
    pts.setflags(write=False); n.setflags(write=False)
    return pts, n


def fresh_ctx(factory):
    ctx = factory()
    ctx.set_gicp_options(EPS, 0)
    return ctx


def same_entries(a, b, what=""):
    """Two (coords, counts, sums, cells) tuples: equal bit for bit."""
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what
    assert np.array_equal(S.u32(a[3]), S.u32(b[3])), what


def hashed_entries(ctx, what=""):
    info, coords, counts, sums, cells = ctx.voxel_map_hashed()
    assert info["n_unplaced"] == 0 and info["n_occupied"] == len(counts) and (counts > 0).all(), (what, info)
    assert info["capacity"] & (info["capacity"] - 1) == 0 and 256 <= info["capacity"] and 2 * info["n_occupied"] <= info["capacity"], (what, info)
    return info, (coords, counts, sums, cells)


def dense_entries(ctx):
    info, counts, sums, cells = ctx.voxel_map()
    e = HR.dense_entries(dict(lo=info["lo"], dims=info["dims"], counts=counts, sums=sums, cells=cells))
    assert len(e[0]) == info["n_occupied"]
    return e


def assert_is(ctx, m, what=""):
    """The hashed map of the context against the restatement's: entries, capacity, growth."""
    info, e = hashed_entries(ctx, what)
    same_entries(e, HR.entries(m), what)
    assert (info["capacity"], info["n_grown"], info["voxel_size"]) == (m["capacity"], m["n_grown"], m["voxel_size"]), (what, info, m["capacity"], m["n_grown"])
    return info, e


def insert_both(ctx, m, pts, nrm, pose, what=""):
    ctx.set_source(pts, nrm, None)
    info = ctx.voxel_map_insert(1, pose)
    want = HR.insert(m, pts, nrm, pose)
    print("insert %s: %s" % (what, info))
    assert info == want, (what, info, want)
    return info, assert_is(ctx, m, what)


def test_crafted_cloud_has_what_it_claims():
    pts, n = crafted()
    ok = VR.entering(pts, n)
    assert len(pts) == N and ok.sum() == N - 14 and (pts[ok] < 0).any()
    for vs in (0.25, 0.3):
        assert len(np.unique(VR.cell_coords(pts[40:340], vs), axis=0)) == 1 and len(np.unique(VR.cell_coords(pts[500:540], vs), axis=0)) == 1
        g = VR.grid(pts, n, vs)
        assert g["counts"].max() >= 300 and (g["counts"] == 1).sum() >= 12
    dy = pts[600:680]
    assert (dy * 8 == np.rint(dy * 8)).all() and ((dy / f32(0.25)) == np.rint(dy / f32(0.25))).any(1).sum() > 30 and (dy < 0).any()


@pytest.mark.parametrize("vs", [0.25, 0.3])
def test_inserts_equal_the_dense_map_and_the_restatement(gpu_ctx_factory, vs):
    """Existing code as the reference: the same inserts (identity, POSE_A, POSE_B; both orders) into a dense map covering everything and
    into a hashed map of 2^14 slots: all six info fields equal, the hashed entries equal the dense map's occupied cells bit for bit, and
    both equal the restatement.  Then a translation of 3e38: nothing lands, the map keeps its bytes."""
    pts, n = crafted()
    jobs = [(pts, n, EYE), (pts[:3000], n[:3000], pose_of(*POSE_A)), (pts[1000:], n[1000:], pose_of(*POSE_B))]
    finals = []
    for order in (jobs, jobs[::-1]):
        dn, hs = fresh_ctx(gpu_ctx_factory), fresh_ctx(gpu_ctx_factory)
        dn.voxel_map_create(vs, *COVER); hs.voxel_map_create_hashed(vs, 1 << 14)
        m = HR.create(vs, 1 << 14)
        for k, (p, q, pose) in enumerate(order):
            dn.set_source(p, q, None)
            di = dn.voxel_map_insert(1, pose)
            hi, (_, e) = insert_both(hs, m, p, q, pose, "%.2f job %d" % (vs, k))
            assert hi == di and di["n_outside"] == 0 and di["n_cells_touched"] > 50, (hi, di)
            same_entries(e, dense_entries(dn), "dense, job %d" % k)
        big = np.concatenate([pts[:300], np.array([[2e38, 0, 0], [0, 2e38, 0], [0, 0, 2e38], [-2e38, -2e38, -2e38]], f32)]); bn = np.concatenate([n[:300], n[:4]])
        for t in ((3e38, 3e38, 3e38), (-3e38, 1.0, 3e38)):
            far = np.eye(4, dtype=f32); far[:3, 3] = t
            i3, (_, e3) = insert_both(hs, m, big, bn, far, "3e38")
            assert i3["n_cells_touched"] == 0 and i3["n_cells_new"] == 0 and i3["n_outside"] == i3["n_entered"] < i3["n_considered"] == 304
            same_entries(e3, e, "after 3e38")
        finals.append(e)
    same_entries(*finals, "A, B against B, A")


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 256, 257, 4099])
def test_insert_sizes(gpu_ctx_factory, n_src):
    """The first n_src points (one lane .. 17 blocks with 3 points in the last), twice at two poses into the same 256-slot map."""
    pts, n = crafted()
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create_hashed(0.3, 256); m = HR.create(0.3, 256)
    insert_both(ctx, m, pts[:n_src], n[:n_src], pose_of(*POSE_A), "n = %d" % n_src)
    insert_both(ctx, m, pts[:n_src], n[:n_src], pose_of(*POSE_B), "n = %d again" % n_src)


def test_insert_cell_patterns(gpu_ctx_factory):
    """Every point in ONE cell (every head claims the same key); every point in a cell of its own, in shuffled order (no run longer than a
    lane, 4099 claims)."""
    r = np.random.default_rng(78)
    ctx = fresh_ctx(gpu_ctx_factory)
    nrm = r.normal(size=(4099, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    one = (np.array([0.375, -0.375, 0.125]) + r.uniform(-0.12, 0.12, (4099, 3))).astype(f32)
    ctx.voxel_map_create_hashed(0.25, 256); m = HR.create(0.25, 256)
    info, (_, e) = insert_both(ctx, m, one, nrm, EYE, "one cell")
    assert info["n_cells_touched"] == 1 and e[1].max() == 4099 and tuple(e[0][0]) == (1, -2, 0)
    info, _ = insert_both(ctx, m, one[:1000], nrm[:1000], EYE, "one cell again")
    assert info["n_cells_touched"] == 1 and info["n_cells_new"] == 0
    ids = r.permutation(17 * 17 * 15)[:4099]
    cc = np.stack([ids % 17, (ids // 17) % 17, ids // 289], 1) + np.array([-8, -8, -7])
    own = ((cc + 0.5) * 0.25 + r.uniform(-0.1, 0.1, (4099, 3))).astype(f32)
    ctx.voxel_map_create_hashed(0.25, 256); m = HR.create(0.25, 256)
    info, (_, e) = insert_both(ctx, m, own, nrm, EYE, "a cell each")
    assert info["n_cells_touched"] == info["n_cells_new"] == 4099 and e[1].max() == 1


@functools.lru_cache(maxsize=None)
def homes_in_256():
    """Every cell of -40 .. 39 cubed with its home slot in a 256-slot table (numpy uint64 arithmetic wraps as the contract's does)."""
    g = np.arange(-40, 40, dtype=np.int64)
    cz, cy, cx = [a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij")]
    key = ((cz + HR.RANGE).astype(np.uint64) << np.uint64(42)) | ((cy + HR.RANGE).astype(np.uint64) << np.uint64(21)) | (cx + HR.RANGE).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = (key * np.uint64(HR.MUL)) >> np.uint64(56)
    return np.stack([cx, cy, cz], 1), h.astype(np.int64)


@pytest.mark.parametrize("case", ["wrap", "one_home", "consecutive"])
def test_probe_chains(gpu_ctx_factory, case):
    """Crafted collisions in a 256-slot table, found by search with the restatement's hash: 40 single-point cells whose home slot is 255
    (the chain wraps round the end), 40 cells sharing home slot 0, 100 cells whose homes are consecutive slots (one long cluster).
    Afterwards every cell is present and exact, nothing was unplaced, the table did not grow, and a system whose source points are those
    points has every one of them valid."""
    cells, h = homes_in_256()
    r = np.random.default_rng(5)
    if case == "wrap":
        cc = cells[h == 255][:40]
    elif case == "one_home":
        cc = cells[h == 0][:40]
    else:
        cc = np.concatenate([cells[h == 100 + k][:1] for k in range(100)])
    assert len(cc) == (100 if case == "consecutive" else 40)
    homes = [HR.home(HR.pack(c), 256) for c in cc]               # (the restatement's hash, one cell at a time, agrees with the search)
    assert homes == ([255] * 40 if case == "wrap" else [0] * 40 if case == "one_home" else list(range(100, 200)))
    cc = cc[r.permutation(len(cc))]
    pts = ((cc + 0.5) * 0.25).astype(f32)                        # cell centres: exact in fp32
    nrm = r.normal(size=(len(cc), 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create_hashed(0.25, 256); m = HR.create(0.25, 256)
    info, (hinfo, e) = insert_both(ctx, m, pts, nrm, EYE, case)
    assert info["n_cells_new"] == len(cc) == info["n_occupied"] and hinfo["capacity"] == 256 and hinfo["n_grown"] == 0 and hinfo["n_unplaced"] == 0
    assert {tuple(c) for c in e[0]} == {tuple(int(v) for v in c) for c in cc} and (e[1] == 1).all()
    again, _ = insert_both(ctx, m, pts[::-1], nrm[::-1], EYE, case + " again")      # every key is found where it was claimed
    assert again["n_cells_new"] == 0 and again["n_cells_touched"] == len(cc)
    sums, counts = ctx.voxel_map_system(EYE, voxel_size=0.25, min_points=1)
    rc, rs, rabs = HR.system(m, pts[::-1], nrm[::-1], EYE, EPS, 1)
    assert tuple(counts) == (len(cc), len(cc)) == tuple(rc)
    assert (np.abs(sums - rs) <= rc[1] * 2.0 ** -52 * rabs).all()


def test_storable_range(gpu_ctx_factory):
    """At 0.25 m the centres of the cells 2^20 - 1, 2^20, -2^20 and -2^20 - 1 are exact in fp32 (22 significant bits): on every axis the
    first and the third enter, the second and the fourth are OUTSIDE.  A source point in a cell that is not storable is not valid."""
    R = HR.RANGE
    rows = []
    for a in range(3):
        for c in (R - 1, R, -R, -R - 1):
            p = np.full(3, 0.125); p[a] = (c + 0.5) * 0.25
            rows.append(p)
    pts = np.array(rows, f64).astype(f32)
    assert np.array_equal(pts.astype(f64), np.array(rows, f64))
    nrm = np.tile(np.array([[0.6, 0.0, 0.8]], f32), (12, 1))
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create_hashed(0.25, 256); m = HR.create(0.25, 256)
    info, (_, e) = insert_both(ctx, m, pts, nrm, EYE, "range")
    assert info["n_entered"] == 12 and info["n_outside"] == 6 and info["n_cells_new"] == 6
    got = {tuple(int(v) for v in c) for c in e[0]}
    assert got == {tuple((c if b == a else 0) for b in range(3)) for a in range(3) for c in (R - 1, -R)}
    sums, counts = ctx.voxel_map_system(EYE, voxel_size=0.25)
    assert tuple(counts) == (12, 6)


def test_growth_and_reserve(gpu_ctx_factory):
    """From 256 slots: the crafted cloud grows the table before it goes in (capacity >= 2 x 4101); two clouds of 4099 cells of their own
    grow it again with content in it; an explicit reserve between two inserts, and a reserve to a smaller size, leave the entries
    bit-identical.  The refusals: a capacity beyond 2^26, below 1; a capacity that is no power of two is rounded UP."""
    pts, n = crafted()
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create_hashed(0.25, 256); m = HR.create(0.25, 256)
    _, (info, _) = insert_both(ctx, m, pts, n, EYE, "from 256")
    assert info["n_grown"] > 0 and info["capacity"] >= 2 * N and info["capacity"] == 1 << 14
    r = np.random.default_rng(79)
    nrm = r.normal(size=(4099, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    ids = r.permutation(26 * 26 * 26)[:8198]
    cc = np.stack([ids % 26, (ids // 26) % 26, ids // 676], 1) - 13
    own = ((cc + 0.5) * 0.25 + r.uniform(-0.1, 0.1, (8198, 3))).astype(f32)
    ctx.voxel_map_create_hashed(0.25, 300); m = HR.create(0.25, 300)
    assert ctx.voxel_map_hashed()[0]["capacity"] == 512
    i1, (h1, _) = insert_both(ctx, m, own[:4099], nrm, EYE, "own cells 1")
    i2, (h2, e2) = insert_both(ctx, m, own[4099:], nrm, pose_of((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), "own cells 2")
    assert i1["n_cells_new"] == 4099 and i2["n_cells_new"] == 4099 and h1["capacity"] == 1 << 14 and h2["capacity"] == 1 << 15 and h2["n_grown"] == 2
    ctx.voxel_map_reserve(1 << 17); HR.reserve(m, 1 << 17)
    h3, e3 = assert_is(ctx, m, "reserved")
    assert h3["capacity"] == 1 << 17 and h3["n_grown"] == 3
    same_entries(e3, e2, "reserve keeps the entries")
    ctx.voxel_map_reserve(1 << 10); ctx.voxel_map_reserve(1 << 17); ctx.voxel_map_reserve(100000)
    h4, e4 = assert_is(ctx, m, "reserve to a smaller size")
    assert h4 == h3
    same_entries(e4, e2)
    insert_both(ctx, m, pts, n, pose_of(*POSE_A), "on a reserved map")
    lib, h = ctx.lib, ctx.h
    for bad in ((1 << 26) + 1, 0, -5):
        assert lib.icp_voxel_map_reserve(h, bad) == ERR_INVALID_ARG and "capacity" in lib.icp_last_error(h).decode()
        assert lib.icp_voxel_map_create_hashed(h, C.c_float(0.25), bad) == ERR_INVALID_ARG and "capacity" in lib.icp_last_error(h).decode()
    assert lib.icp_voxel_map_create_hashed(h, C.c_float(0.0), 256) == ERR_INVALID_ARG
    assert lib.icp_voxel_map_upload_hashed(h, -1, None, None, None) == ERR_INVALID_ARG
    assert_is(ctx, m, "after the refusals")


def test_upload_round_trip_and_refusals(gpu_ctx_factory):
    """Download, create, upload, download is a round trip; counts near 2^20 and a zero trace give the restatement's records; an insert on
    top goes on from there; a duplicate coordinate, a negative count and a coordinate that is not storable are refused and change nothing;
    the dense get and upload calls refuse a hashed map with a reason, and the other way round."""
    pts, n = crafted()
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create_hashed(0.25, 256); m = HR.create(0.25, 256)
    insert_both(ctx, m, pts, n, pose_of(*POSE_A), "to save")
    _, saved = hashed_entries(ctx)
    ctx.voxel_map_create_hashed(0.25, 256)
    assert ctx.voxel_map_hashed()[0]["n_occupied"] == 0
    ctx.voxel_map_upload_hashed(*saved[:3])
    info, back = hashed_entries(ctx)
    same_entries(back, saved, "round trip")
    assert info["capacity"] >= 2 * len(saved[0])
    r = np.random.default_rng(4)
    nc = 60
    coords = np.stack([r.permutation(200)[:nc] - 100, r.integers(-50, 50, nc), r.integers(-(1 << 20), 1 << 20, nc)], 1).astype(np.int32)
    counts = r.integers(0, 5, nc).astype(np.int32)
    counts[[3, 17, 41]] = (1 << 20) - np.array([0, 1, 7]); counts[5] = 1
    cn = counts.astype(np.int64)
    sums = np.zeros((nc, 9), np.int64)
    sums[:, :3] = r.integers(-32768, 32769, (nc, 3)) * cn[:, None]
    d = r.integers(0, 1 << 28, (nc, 3)) * cn[:, None]
    sums[:, [3, 6, 8]] = d
    sums[:, [4, 5, 7]] = (r.uniform(-0.5, 0.5, (nc, 3)) * np.sqrt(d[:, [0, 0, 1]].astype(f64) * d[:, [1, 2, 2]].astype(f64))).astype(np.int64)
    sums[counts == 0] = 0
    sums[5, 3:] = 0                                              # an occupied cell with a zero trace: S = 0
    ctx.voxel_map_upload_hashed(coords, counts, sums)
    m = HR.create(0.25, info["capacity"]); m["n_grown"] = info["n_grown"]
    HR.upload(m, coords, counts, sums)
    _, e = assert_is(ctx, m, "upload")
    k5 = int(np.nonzero((e[0] == coords[5]).all(1))[0][0])
    assert len(e[0]) == (counts > 0).sum() and not e[3][k5, 3:].any() and e[3][k5, :3].any() and np.isfinite(e[3]).all()
    shift = np.eye(4, dtype=f32); shift[:3, 3] = (-20.1, 1.6, 1.1)
    insert_both(ctx, m, pts[:700], n[:700], shift, "on an uploaded map")
    lib, h = ctx.lib, ctx.h
    up = lambda c, k, s: lib.icp_voxel_map_upload_hashed(h, len(k), np.ascontiguousarray(c, np.int32).ctypes.data_as(C.c_void_p),
                                                         np.ascontiguousarray(k, np.int32).ctypes.data_as(C.c_void_p), np.ascontiguousarray(s, np.int64).ctypes.data_as(C.c_void_p))
    dup = coords.copy(); dup[9] = dup[2]
    neg = counts.copy(); neg[0] = -1
    out = coords.copy(); out[7, 1] = 1 << 20
    for args, word in (((dup, counts, sums), "twice"), ((coords, neg, sums), "negative"), ((out, counts, sums), "storable")):
        assert up(*args) == ERR_INVALID_ARG and word in lib.icp_last_error(h).decode(), word
    assert_is(ctx, m, "after the refused uploads")
    # the dense calls on a hashed map, the hashed calls on a dense map
    assert lib.icp_get_voxel_map(h, None, None, None, None) == ERR_INVALID_ARG and "hashed" in lib.icp_last_error(h).decode()
    assert lib.icp_voxel_map_upload(h, counts.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)) == ERR_INVALID_ARG and "hashed" in lib.icp_last_error(h).decode()
    ctx.voxel_map_create(0.25, (-2, -2, -2), (4, 4, 4))
    assert lib.icp_get_voxel_map_hashed(h, None, 0, None, None, None, None) == ERR_INVALID_ARG and "dense" in lib.icp_last_error(h).decode()
    assert up(coords, counts, sums) == ERR_INVALID_ARG and "dense" in lib.icp_last_error(h).decode()
    assert lib.icp_voxel_map_reserve(h, 1024) == ERR_INVALID_ARG and "dense" in lib.icp_last_error(h).decode()
    assert ctx.voxel_map()[0]["n_occupied"] == 0
    ctx.voxel_map_destroy()
    assert lib.icp_get_voxel_map_hashed(h, None, 0, None, None, None, None) == ERR_INVALID_ARG and "no voxel map" in lib.icp_last_error(h).decode()
    # max_entries below the occupied count while an array is asked for
    ctx.voxel_map_create_hashed(0.25, 256)
    ctx.voxel_map_upload_hashed(coords, counts, sums)
    buf = np.empty(3 * nc, np.int32)
    assert lib.icp_get_voxel_map_hashed(h, None, 3, buf.ctypes.data_as(C.c_void_p), None, None, None) == ERR_INVALID_ARG and "max_entries" in lib.icp_last_error(h).decode()
    assert lib.icp_get_voxel_map_hashed(h, None, 0, None, None, None, None) == 0


@functools.lru_cache(maxsize=None)
def moved_source():
    """The crafted cloud moved by the inverse of a small pose (fp64, rounded once), with a zero normal and a NaN normal of its own."""
    pts, n = crafted()
    T = np.linalg.inv(pose_of((0.02, -0.015, 0.01), (0.03, 0.02, -0.025)).astype(f64))
    with np.errstate(all="ignore"):
        sp = (pts.astype(f64) @ T[:3, :3].T + T[:3, 3]).astype(f32); sn = (n.astype(f64) @ T[:3, :3].T).astype(f32)
    sn[5] = (0, 0, 0); sn[6] = (np.nan, 0, 0)
    sp.setflags(write=False); sn.setflags(write=False)
    return sp, sn


def two_insert_maps(factory):
    """Two contexts with NO target and the same two inserts: a dense map over a covering extent and a hashed map grown from 256 slots; the
    moved source resident in both.  Returns (dense ctx, hashed ctx, the restatement's hashed map)."""
    pts, n = crafted()
    dn, hs = fresh_ctx(factory), fresh_ctx(factory)
    dn.voxel_map_create(0.25, *COVER); hs.voxel_map_create_hashed(0.25, 256); m = HR.create(0.25, 256)
    second = pose_of((0.01, -0.008, 0.006), (0.02, -0.015, 0.01))
    for p, q, pose in ((pts, n, EYE), (pts[:2500], n[:2500], second)):
        dn.set_source(p, q, None); dn.voxel_map_insert(1, pose)
        insert_both(hs, m, p, q, pose, "map")
    dn.set_source(*moved_source(), None); hs.set_source(*moved_source(), None)
    return dn, hs, m


def test_system_against_the_dense_map(gpu_ctx_factory):
    """The sums of one step, with no target set, at three poses and min_points 1 and 3: counts exactly the dense map's and the
    restatement's; every sum within the contract's bound n_valid 2^-52 sum |term| of both; the largest difference to the dense map is
    printed (the per-point arithmetic and the fold are the same and the build does not contract: 0 is expected, the bound is asserted); a
    second call gives identical bits."""
    dn, hs, m = two_insert_maps(gpu_ctx_factory)
    sp, sn = moved_source()
    worst = 0.0
    for pose in (EYE, pose_of((0.012, -0.009, 0.015), (0.02, -0.015, 0.01)), pose_of((0.3, -0.2, 0.25), (0.8, -0.5, 0.3))):
        for mp in (1, 3):
            sums, counts = hs.voxel_map_system(pose, voxel_size=0.25, min_points=mp)
            dsums, dcounts = dn.voxel_map_system(pose, voxel_size=0.25, min_points=mp)
            rcounts, rsums, rabs = HR.system(m, sp, sn, pose, EPS, mp)
            bound = rcounts[1] * 2.0 ** -52 * rabs
            diff = float(np.abs(sums - dsums).max())
            worst = max(worst, diff)
            print("system min_points %d: considered %d, valid %d, max |hashed - dense| = %.3g, worst |hashed - restatement| / bound = %.3g" % (
                mp, counts[0], counts[1], diff, float((np.abs(sums - rsums) / np.maximum(bound, 1e-300)).max())))
            assert tuple(counts) == tuple(dcounts) == tuple(rcounts) and counts[0] == N - 8 and counts[1] > 0
            assert (np.abs(sums - dsums) <= bound).all() and (np.abs(sums - rsums) <= bound).all()
            again, counts2 = hs.voxel_map_system(pose, voxel_size=0.25, min_points=mp)
            assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts)
    print("largest |hashed - dense| over all sums: %.3g" % worst)


def test_align_steps(gpu_ctx_factory):
    """8 iterations with the stops off, traced, from two starts: iteration i's pose within 1e-5 per element of step(system(the DEVICE's
    pose i - 1)) on the restatement's map, n_valid exactly; against the dense map's run the difference is printed; a second run gives
    identical bits.  Then the stop (the trace is the head of the full run's, zeros behind it), max_trace, and a start 50 m away: carried."""
    from icp_amd import binding
    dn, hs, m = two_insert_maps(gpu_ctx_factory)
    sp, sn = moved_source()
    g = HR.dense(m)[0]
    kw = dict(voxel_size=0.25, n_iterations=8, stop_rotation=0.0, stop_translation=0.0)
    for start in (EYE, pose_of((-0.03, 0.025, -0.02), (-0.04, 0.03, 0.035))):
        pose, rec, rc, trace = hs.voxel_map_align(start, trace=True, **kw)
        dpose, drec, drc, dtrace = dn.voxel_map_align(start, trace=True, **kw)
        assert rc == 0 and rec["status"] == 0 and rec["iterations"] == 8 and len(trace) == 8 and drc == 0
        prev = start
        for i, t in enumerate(trace):
            counts, sums, sabs = VR.system(g, sp, sn, prev, EPS)
            want, _ = VR.step(sums, counts, prev)
            diff = float(np.abs(t["pose"] - want).max())
            print("align step %d: n_valid %d, |pose - restatement| = %.3g, |pose - dense map's| = %.3g" % (i, t["n_valid"], diff, float(np.abs(t["pose"] - dtrace[i]["pose"]).max())))
            assert t["status"] == 0 and t["n_valid"] == counts[1] == dtrace[i]["n_valid"], i
            assert diff <= 1e-5, i
            assert abs(t["cost"] - sums[27]) <= counts[1] * 2.0 ** -52 * sabs[27], i
            prev = t["pose"]
        assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose) and rec["cost_last"] < rec["cost_first"]
        pose2, rec2, rc2, trace2 = hs.voxel_map_align(start, trace=True, **kw)
        assert rc2 == 0 and same_bits(pose2, pose)
        for a, b in zip(trace, trace2):
            assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    full_pose, full_rec, rc, full = hs.voxel_map_align(EYE, trace=True, stop_rotation=0.0, stop_translation=0.0)
    assert rc == 0 and len(full) == 30
    pose, rec, rc, trace = hs.voxel_map_align(EYE, trace=True, stop_rotation=1e-3, stop_translation=1e-3)
    ns = rec["iterations"]
    print("stop: %d of 30 iterations" % ns)
    assert rc == 0 and 1 <= ns < 30 and len(trace) == ns and same_bits(pose, trace[-1]["pose"])
    for a, b in zip(trace, full):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    o = binding.vgicp_options(stop_rotation=1e-3, stop_translation=1e-3)
    p = binding.pose_to_c(EYE); r = binding.IcpSdfFrame(); tr = (binding.IcpSdfIter * 30)()
    assert hs.lib.icp_voxel_map_align(hs.h, C.byref(o), binding._ptr(p), C.byref(r), tr, 30) == 0
    assert r.iterations == ns and not any(bytes(tr[i]) != bytes(80) for i in range(ns, 30)) and bytes(tr[ns - 1]) != bytes(80)
    tr2 = (binding.IcpSdfIter * 30)(); p = binding.pose_to_c(EYE)
    assert hs.lib.icp_voxel_map_align(hs.h, C.byref(o), binding._ptr(p), C.byref(r), tr2, 1) == 0
    assert bytes(tr2[0]) == bytes(tr[0]) and not any(bytes(tr2[i]) != bytes(80) for i in range(1, 30))
    away = pose_of((0.0, 0.0, 0.0), (50.0, 0.0, 0.0))
    pose, rec, rc, trace = hs.voxel_map_align(away, trace=True)
    assert rc == ERR_NO_CORRESPONDENCES and rec["status"] == rc and same_bits(pose, away) and rec["iterations"] == 1 and rec["n_valid_first"] == 0
    assert "icp_voxel_map_align" in hs.lib.icp_last_error(hs.h).decode()
    o3 = binding.vgicp_options(voxel_size=0.3); p = binding.pose_to_c(EYE)
    assert hs.lib.icp_voxel_map_align(hs.h, C.byref(o3), binding._ptr(p), None, None, 0) == ERR_INVALID_ARG and "voxel_size" in hs.lib.icp_last_error(hs.h).decode()


TRACK = dict(voxel_size=MF.VOXEL, n_iterations=6, stop_rotation=0.0, stop_translation=0.0)


@functools.lru_cache(maxsize=None)
def small_scans():
    """6 scans of 43 x 135 points along the fixture's path, each in its sensor frame."""
    return MF.scans(6, (43, 135))


def wide_extent(cells=16):
    lo, dims = MF.extent()
    return tuple(int(v) - cells for v in lo), tuple(int(v) + 2 * cells for v in dims)


def test_tracking_against_the_dense_loop(gpu_ctx_factory):
    """The six scans tracked into a hashed map that starts at 256 slots, against the dense loop over an extent that covers everything, on
    the same device: statuses and valid counts exactly, poses within 1e-5 per step taken (the measured difference is printed), the final
    maps equal cell for cell."""
    from icp_amd import eth
    scans = small_scans()
    start = MF.truth(0).astype(f32)
    dn, hs = fresh_ctx(gpu_ctx_factory), fresh_ctx(gpu_ctx_factory)
    dn.voxel_map_create(MF.VOXEL, *wide_extent())
    dpose, drecs, drc = dn.track_scans_vmap(scans, start, **TRACK)
    poses, recs, rc = eth.track_map(hs, scans, start, voxel_size=MF.VOXEL, hashed=True, capacity=256, **{k: v for k, v in TRACK.items() if k != "voxel_size"})
    assert rc == drc == 0 and len(recs) == 5 and len(poses) == 6
    for k, (a, b) in enumerate(zip(recs, drecs), 1):
        diff = float(np.abs(a["pose"] - b["pose"]).max())
        print("scan %d: %d iterations, n_valid %d -> %d, |pose - dense loop's| = %.3g" % (k, a["iterations"], a["n_valid_first"], a["n_valid_last"], diff))
        assert (a["status"], a["n_depth"], a["n_valid_first"], a["n_valid_last"], a["iterations"]) == (b["status"], b["n_depth"], b["n_valid_first"], b["n_valid_last"], b["iterations"]), k
        assert diff <= 1e-5 * a["iterations"], k
        rot, tr = MF.pose_error(a["pose"], MF.truth(k))
        assert rot < 0.02 and tr < 0.05, (k, rot, tr)
    info, e = hashed_entries(hs, "tracked")
    full = dense_entries(dn)
    same_entries(e, full, "hashed against the covering dense map")
    assert info["n_grown"] > 0 and info["capacity"] >= 2 * 43 * 135
    with pytest.raises(ValueError):
        eth.track_map(hs, scans, start, voxel_size=MF.VOXEL, hashed=True, extent=wide_extent())


@functools.lru_cache(maxsize=None)
def near_scans():
    """The six scans as a laser of 3 m range sees them (the fixture's room is closed and every full scan reaches all of it: nothing of
    a later scan lies beyond scan 0's bounds).  Some 3 200 to 3 700 points each; by the true poses 14, 51, 101, 338 and 639 points of
    scans 1 .. 5 lie beyond the tight bounds of scan 0."""
    out = []
    for xyz, nrm in small_scans():
        keep = np.linalg.norm(xyz.astype(f64), axis=1) < 3.0
        out.append((np.ascontiguousarray(xyz[keep]), np.ascontiguousarray(nrm[keep])))
    return out


def test_a_trajectory_that_leaves_the_dense_extent(gpu_ctx_factory):
    """What the feature exists for.  A sensor of 3 m range walks along the fixture's path: the hashed map, from 256 slots, equals the
    dense map over a covering extent cell for cell (poses and valid counts as in the test above), while a dense map whose extent is scan
    0's tight bounds, given the same scans at the same poses, reports n_outside > 0 on every later scan and ends with fewer occupied
    cells than the hashed map."""
    from icp_amd import binding, eth
    scans = near_scans()
    start = MF.truth(0).astype(f32)
    dn, hs = fresh_ctx(gpu_ctx_factory), fresh_ctx(gpu_ctx_factory)
    dn.voxel_map_create(MF.VOXEL, *wide_extent())
    dpose, drecs, drc = dn.track_scans_vmap(scans, start, **TRACK)
    poses, recs, rc = eth.track_map(hs, scans, start, voxel_size=MF.VOXEL, hashed=True, capacity=256, **{k: v for k, v in TRACK.items() if k != "voxel_size"})
    assert rc == drc == 0
    for k, (a, b) in enumerate(zip(recs, drecs), 1):
        diff = float(np.abs(a["pose"] - b["pose"]).max())
        print("scan %d: n_valid %d -> %d, |pose - dense loop's| = %.3g" % (k, a["n_valid_first"], a["n_valid_last"], diff))
        assert (a["status"], a["n_depth"], a["n_valid_first"], a["n_valid_last"], a["iterations"]) == (b["status"], b["n_depth"], b["n_valid_first"], b["n_valid_last"], b["iterations"]), k
        assert diff <= 1e-5 * a["iterations"], k
    info, e = hashed_entries(hs, "tracked")
    same_entries(e, dense_entries(dn), "hashed against the covering dense map")
    world = scans[0][0].astype(f64) @ start[:3, :3].astype(f64).T + start[:3, 3].astype(f64)
    tight = fresh_ctx(gpu_ctx_factory)
    tight.voxel_map_create(MF.VOXEL, *binding.voxel_map_extent(world.min(0), world.max(0), MF.VOXEL))
    outside = []
    for (xyz, nrm), P in zip(scans, poses):
        tight.set_source(xyz, nrm, None)
        outside.append(tight.voxel_map_insert(1, P)["n_outside"])
    n_tight = tight.voxel_map()[0]["n_occupied"]
    print("tight dense extent: n_outside per scan %s, %d cells against %d hashed" % (outside, n_tight, info["n_occupied"]))
    assert outside[0] == 0 and all(v > 0 for v in outside[1:]) and n_tight < info["n_occupied"]


def test_tracking_skips_failed_scans(gpu_ctx_factory):
    """A scan that is all NaN (ICP_ERR_NO_SOURCE) and a scan 50 m away (ICP_ERR_NO_CORRESPONDENCES) among four good ones: each is carried and
    skipped with its status, the first error is returned, and the map is what the good scans alone leave (the restatement, given the
    device's poses)."""
    good = small_scans()
    nan = (np.full_like(good[2][0], np.nan), good[2][1])
    far = (good[3][0] + f32(50.0) * np.array([1, 0, 0], f32), good[3][1])
    scans = [good[0], good[1], nan, good[2], far, good[3]]
    start = MF.truth(0).astype(f32)
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create_hashed(MF.VOXEL, 256)
    pose, recs, rc = ctx.track_scans_vmap(scans, start, **TRACK)
    assert rc == ERR_NO_SOURCE and [r["status"] for r in recs] == [0, ERR_NO_SOURCE, 0, ERR_NO_CORRESPONDENCES, 0]
    assert "icp_track_scans_vmap" in ctx.lib.icp_last_error(ctx.h).decode()
    assert same_bits(recs[1]["pose"], recs[0]["pose"]) and same_bits(recs[3]["pose"], recs[2]["pose"]) and recs[1]["n_depth"] == 0 and recs[3]["n_valid_first"] == 0
    only_good = HR.create(MF.VOXEL, 256)
    for (xyz, nrm), P in zip(good[:4], [start, recs[0]["pose"], recs[2]["pose"], recs[4]["pose"]]):
        HR.insert(only_good, xyz, nrm, P)
    _, e = hashed_entries(ctx)
    same_entries(e, HR.entries(only_good), "the good scans alone")


def test_outcome_on_the_recorded_fixture(gpu_ctx_factory):
    """The fixture's 12 scans of 86 x 270 points through eth.track_map(hashed=True): the bounds tests/golden/vmap_outcome.json holds for the
    map loop -- the final and the worst pose error at most twice the restatement's figures, and below the pair chain's."""
    from icp_amd import eth
    with open(MF.GOLDEN) as f:
        gold = json.load(f)
    ctx = gpu_ctx_factory()
    ctx.set_gicp_options(MF.EPSILON, 0)
    opt = {k: v for k, v in MF.OPTIONS.items() if k != "voxel_size"}
    poses, recs, rc = eth.track_map(ctx, MF.scans(), MF.truth(0).astype(f32), voxel_size=MF.VOXEL, hashed=True, **opt)
    e = MF.errors(poses)
    info = ctx.voxel_map_hashed()[0]
    print("outcome: device %s; restatement map %s; chain %s; iterations %s; %s" % (e, gold["map"], gold["chain"], [r["iterations"] for r in recs], info))
    assert rc == 0 and len(recs) == MF.N_SCANS - 1 and all(r["status"] == 0 for r in recs)
    assert info["n_occupied"] > 0.9 * gold["n_occupied"] and info["n_unplaced"] == 0
    for k, v in e.items():
        assert v <= 2 * gold["map"][k], k
        assert v < gold["chain"][k], k


def use_the_hashed_map(ctx):
    """Every new call once, on a context whose clouds are resident."""
    ctx.voxel_map_create_hashed(0.5, 256)
    assert ctx.voxel_map_insert(0, EYE)["n_cells_new"] > 10 and ctx.voxel_map_insert(1, EYE)["n_cells_touched"] > 10
    ctx.voxel_map_reserve(1 << 18)
    ctx.voxel_map_system(EYE, voxel_size=0.5)
    _, rec, rc = ctx.voxel_map_align(EYE, voxel_size=0.5, n_iterations=5)
    assert rc == 0 and rec["n_valid_first"] > 64
    info, coords, counts, sums, cells = ctx.voxel_map_hashed()
    ctx.voxel_map_upload_hashed(coords, counts, sums)
    assert info["n_grown"] > 0


def dense_calls(ctx):
    ctx.voxel_map_create(0.5, (-10, -12, -2), (20, 24, 9))
    a = ctx.voxel_map_insert(0, EYE); b = ctx.voxel_map_insert(1, EYE)
    sums, counts = ctx.voxel_map_system(EYE, voxel_size=0.5)
    pose, rec, rc = ctx.voxel_map_align(EYE, voxel_size=0.5, n_iterations=5)
    return a, b, sums, counts, pose, rec, rc, ctx.voxel_map()


@pytest.mark.parametrize("metric", [1, 3])
def test_untouched_paths(gpu_ctx_factory, metric):
    """The dense map calls, icp_vgicp_align on a target and icp_run (point-to-plane; GICP), on a context that has made every new call
    against a context that never made one: the same bytes."""
    from icp_amd import synth
    d = synth.eth_like_pair(0, 20, 64)
    runs = []
    for touched in (True, False):
        ctx = gpu_ctx_factory()
        S.configure(ctx, metric=metric, n_iterations=6, max_distance=0.5)
        S.load(ctx, d, colors=False)
        if touched:
            use_the_hashed_map(ctx)
        dm = dense_calls(ctx)
        if touched:
            use_the_hashed_map(ctx)
        vg = ctx.vgicp_align(EYE, trace=True, voxel_size=0.5, n_iterations=5)
        if touched:
            use_the_hashed_map(ctx)
        runs.append((dm, vg, ctx.run(EYE), ctx.voxel_grid(voxel_size=0.5)))
    (da, va, (pa, ra, rca), ga), (db, vb, (pb, rb, rcb), gb) = runs
    assert da[0] == db[0] and da[1] == db[1] and np.array_equal(u64(da[2]), u64(db[2])) and tuple(da[3]) == tuple(db[3]) and same_bits(da[4], db[4]) and da[6] == db[6] == 0
    assert {k: v for k, v in da[5].items() if k != "pose"} == {k: v for k, v in db[5].items() if k != "pose"}
    assert da[7][0] == db[7][0] and all(np.array_equal(S.raw_bits(a), S.raw_bits(b)) for a, b in zip(da[7][1:], db[7][1:]))
    assert va[2] == vb[2] == 0 and same_bits(va[0], vb[0]) and len(va[3]) == len(vb[3]) == 5
    for a, b in zip(va[3], vb[3]):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    assert {k: v for k, v in va[1].items() if k != "pose"} == {k: v for k, v in vb[1].items() if k != "pose"}
    assert rca == rcb == 0 and same_bits(pa, pb)
    S.assert_same_run(ra, rb)
    assert ga[0] == gb[0] and all(np.array_equal(S.raw_bits(a), S.raw_bits(b)) for a, b in zip(ga[1:], gb[1:]))
