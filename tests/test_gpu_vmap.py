"""Scan-to-map laser tracking on the device against the numpy restatement of its contract (tests/vmap_restatement.py): an insert at the
identity against icp_voxelize_target's grid, inserts at poses, beyond the extent, in both orders and at block-edge sizes against the
restatement -- counts, sums, records and the info record exactly -- the upload round trip, the refusals, the sums of a step and every step
of an alignment against the map with no target set, tracking against the restatement run from the device's own poses, the paths that
must stay untouched, and the outcome on the recorded fixture."""
import ctypes as C
import functools
import json
import numpy as np
import pytest

import support as S
import vgicp_restatement as VR
import vmap_restatement as MR
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


def u64(a):
    return np.ascontiguousarray(a, dtype=f64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def crafted():
    """4101 points with normals in the order a tilting scan has (rows of 61 points over a wavy surface), and in it:
      [30, 350)     320 consecutive points of ONE cell at voxel sizes 0.25 and 0.3: the run crosses the wave boundaries 64 .. 320 and the block boundary 256
      [480, 530)    50 points of one cell across the block boundary 512
      [600, 672)    dyadic coordinates (multiples of 1/8: exactly on cell faces at 0.25), negative ones among them
      [700, 710)    single-point cells, far from everything else
      [720, 728)    positions with NaN / +inf / -inf; [728, 732) NaN normals; 732, 733 an infinite normal component: all stay out
      4100          the last point, alone in the last (partial) block
    Returned read-only: (points, normals)."""
    r = np.random.default_rng(1912)
    k = np.arange(N)
    row, col = k // 61, k % 61
    x = -1.1 + col * (2.3 / 61) + r.normal(0, 0.002, N); y = -1.2 + row * (2.4 / 68) + r.normal(0, 0.002, N)
    z = 0.25 * np.sin(2.5 * x) + 0.2 * np.cos(2.0 * y) + 0.3 * (y > 0.5)
    n = np.stack([-0.625 * np.cos(2.5 * x), 0.4 * np.sin(2.0 * y), np.ones(N)], 1) + r.normal(0, 0.02, (N, 3))
    pts = np.stack([x, y, z], 1)
    pts[30:350] = (0.67, -0.66, 0.67) + r.uniform(-0.02, 0.02, (320, 3))
    pts[480:530] = (-0.41, 0.40, -0.40) + r.uniform(-0.02, 0.02, (50, 3))
    pts[600:672] = r.integers(-10, 11, (72, 3)) / 8.0
    pts[700:710] = np.array([-3.2, 2.3, 1.4]) + np.arange(10)[:, None] * np.array([-0.37, 0.43, 0.31])
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


def assert_same_map(ctx, m, what=""):
    info, counts, sums, cells = ctx.voxel_map()
    assert info["lo"] == tuple(int(v) for v in m["lo"]) and info["dims"] == tuple(int(v) for v in m["dims"]) and info["voxel_size"] == m["voxel_size"], what
    assert np.array_equal(counts, m["counts"]), what
    assert np.array_equal(sums, m["sums"]), what
    assert np.array_equal(S.u32(cells), S.u32(m["cells"])), what
    assert info["n_occupied"] == m["n_occupied"] == int((counts > 0).sum()), what
    return counts, sums, cells


def insert_both(ctx, m, pts, nrm, pose, what=""):
    """The cloud becomes the source and goes into the device's map and into the restatement's at `pose`: the six info fields and the whole
    map must agree exactly."""
    ctx.set_source(pts, nrm, None)
    info = ctx.voxel_map_insert(1, pose)
    want = MR.insert(m, pts, nrm, pose)
    print("insert %s: %s" % (what, info))
    assert info == want, (what, info, want)
    return info, assert_same_map(ctx, m, what)


def test_crafted_cloud_has_what_it_claims():
    pts, n = crafted()
    ok = VR.entering(pts, n)
    assert len(pts) == N and ok.sum() == N - 14 and (pts[ok] < 0).any()
    for vs in (0.25, 0.3):
        assert len(np.unique(VR.cell_coords(pts[30:350], vs), axis=0)) == 1 and len(np.unique(VR.cell_coords(pts[480:530], vs), axis=0)) == 1
        g = VR.grid(pts, n, vs)
        assert g["counts"].max() >= 320 and (g["counts"] == 1).sum() >= 10 and (g["counts"] == 0).sum() > 100
    dy = pts[600:672]
    assert (dy * 8 == np.rint(dy * 8)).all() and ((dy / f32(0.25)) == np.rint(dy / f32(0.25))).any(1).sum() > 30 and (dy < 0).any()


@pytest.mark.parametrize("vs", [0.25, 0.3])
def test_identity_insert_is_the_targets_grid(gpu_ctx_factory, vs):
    """The crafted cloud as the target with its own normals: inserted with which = 0 at the identity into a map whose extent is
    icp_voxelize_target's, it gives that grid's counts, sums and records bit for bit -- existing code as the reference."""
    ctx = fresh_ctx(gpu_ctx_factory)
    pts, n = crafted()
    ctx.set_target(pts, n, None)
    ginfo, gcounts, gsums, gcells = ctx.voxel_grid(voxel_size=vs)
    ctx.voxel_map_create(vs, ginfo["lo"], ginfo["dims"])
    info = ctx.voxel_map_insert(0, EYE)
    minfo, counts, sums, cells = ctx.voxel_map()
    print("identity %.2f: %s" % (vs, info))
    assert info == dict(n_considered=N - 8, n_entered=ginfo["n_points"], n_outside=0, n_cells_touched=ginfo["n_occupied"], n_cells_new=ginfo["n_occupied"], n_occupied=ginfo["n_occupied"])
    assert ginfo["n_points"] == N - 14 and minfo["n_occupied"] == ginfo["n_occupied"] and minfo["lo"] == ginfo["lo"] and minfo["dims"] == ginfo["dims"]
    assert np.array_equal(counts, gcounts) and np.array_equal(sums, gsums) and np.array_equal(S.u32(cells), S.u32(gcells))
    # the target's grid is separate state: still there, still the same bytes
    _, c2, s2, r2 = ctx.voxel_grid(voxel_size=vs)
    assert np.array_equal(c2, gcounts) and np.array_equal(s2, gsums) and np.array_equal(S.u32(r2), S.u32(gcells))


def test_inserts_match_restatement(gpu_ctx_factory):
    """A non-trivial pose into an extent smaller than the cloud (n_outside > 0), a second insert at another pose, the same two in the other
    order (the same bytes), and poses with a translation of 3e38: the moved coordinates are 3e38 or overflow, no point lands inside the
    extent, the map keeps its bytes."""
    pts, n = crafted()
    A, B = pose_of(*POSE_A), pose_of(*POSE_B)
    vs, lo, dims = 0.25, (-4, -5, -3), (9, 9, 7)
    jobs = [(pts, n, A), (pts[:2000], n[:2000], B)]
    maps = []
    for order in (jobs, jobs[::-1]):
        ctx = fresh_ctx(gpu_ctx_factory)
        ctx.voxel_map_create(vs, lo, dims)
        m = MR.create(vs, lo, dims)
        i1, _ = insert_both(ctx, m, *order[0], "first")
        assert i1["n_considered"] in (N - 8, 2000 - 8) and 0 < i1["n_outside"] < i1["n_entered"] <= i1["n_considered"] - 6 and i1["n_cells_new"] == i1["n_cells_touched"] == i1["n_occupied"]
        i2, state = insert_both(ctx, m, *order[1], "second")
        assert 0 < i2["n_cells_new"] < i2["n_cells_touched"] and i2["n_occupied"] == i1["n_occupied"] + i2["n_cells_new"]
        maps.append(state)
        # huge points next to the cloud's: +2e38 + 3e38 overflows (considered, does not enter), the others enter and are all outside
        big = np.concatenate([pts[:300], np.array([[2e38, 0, 0], [0, 2e38, 0], [0, 0, 2e38], [-2e38, -2e38, -2e38]], f32)]); bn = np.concatenate([n[:300], n[:4]])
        for t in ((3e38, 3e38, 3e38), (-3e38, 1.0, 3e38)):
            far = np.eye(4, dtype=f32); far[:3, 3] = t
            i3, state3 = insert_both(ctx, m, big, bn, far, "3e38")
            assert i3["n_cells_touched"] == 0 and i3["n_cells_new"] == 0 and i3["n_outside"] == i3["n_entered"] < i3["n_considered"] == 304 and i3["n_occupied"] == i2["n_occupied"]
            assert all(np.array_equal(S.raw_bits(a), S.raw_bits(b)) for a, b in zip(state, state3))
    for a, b in zip(*maps):
        assert np.array_equal(S.raw_bits(a), S.raw_bits(b))


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 256, 257, 4099])
def test_insert_sizes(gpu_ctx_factory, n_src):
    """The first n_src points (one lane, a wave less one, a wave, a wave and one, a block, a block and one, 17 blocks with 3 points in the
    last), twice at two poses into the same map."""
    pts, n = crafted()
    ctx = fresh_ctx(gpu_ctx_factory)
    vs, lo, dims = 0.3, (-6, -6, -4), (13, 12, 9)
    ctx.voxel_map_create(vs, lo, dims)
    m = MR.create(vs, lo, dims)
    insert_both(ctx, m, pts[:n_src], n[:n_src], pose_of(*POSE_A), "n = %d" % n_src)
    insert_both(ctx, m, pts[:n_src], n[:n_src], pose_of(*POSE_B), "n = %d again" % n_src)


def test_insert_cell_patterns(gpu_ctx_factory):
    """Every point in ONE cell (all atomics on one address, one list entry); every point in a cell of its own, in shuffled order (no run
    longer than one lane, the list as long as the cloud); a 2 x 2 x 2 map under 4099 points (the list shorter than its launch)."""
    r = np.random.default_rng(77)
    ctx = fresh_ctx(gpu_ctx_factory)
    nrm = r.normal(size=(4099, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    # one cell: cell (1, -2, 0) at 0.25
    one = (np.array([0.375, -0.375, 0.125]) + r.uniform(-0.12, 0.12, (4099, 3))).astype(f32)
    ctx.voxel_map_create(0.25, (-1, -3, -1), (4, 3, 3)); m = MR.create(0.25, (-1, -3, -1), (4, 3, 3))
    info, (counts, _, _) = insert_both(ctx, m, one, nrm, EYE, "one cell")
    assert info["n_cells_touched"] == 1 and counts.max() == 4099
    info, _ = insert_both(ctx, m, one[:1000], nrm[:1000], EYE, "one cell again")
    assert info["n_cells_touched"] == 1 and info["n_cells_new"] == 0
    # a cell each: 17 x 17 x 15 = 4335 cells, 4099 of them in shuffled order
    dims = (17, 17, 15)
    ids = r.permutation(17 * 17 * 15)[:4099]
    cc = np.stack([ids % 17, (ids // 17) % 17, ids // 289], 1) + np.array([-8, -8, -7])
    own = ((cc + 0.5) * 0.25 + r.uniform(-0.1, 0.1, (4099, 3))).astype(f32)
    ctx.voxel_map_create(0.25, (-8, -8, -7), dims); m = MR.create(0.25, (-8, -8, -7), dims)
    info, (counts, _, _) = insert_both(ctx, m, own, nrm, EYE, "a cell each")
    assert info["n_cells_touched"] == info["n_cells_new"] == 4099 and counts.max() == 1
    # 2 x 2 x 2 under the crafted cloud
    pts, n = crafted()
    ctx.voxel_map_create(0.6, (-1, -1, -1), (2, 2, 2)); m = MR.create(0.6, (-1, -1, -1), (2, 2, 2))
    info, _ = insert_both(ctx, m, pts[:4099], n[:4099], pose_of(*POSE_B), "2 x 2 x 2")
    assert 4 <= info["n_cells_touched"] <= 8 and info["n_outside"] > 1000
    again, _ = insert_both(ctx, m, pts[:4099], n[:4099], pose_of(*POSE_A), "2 x 2 x 2 again")
    assert 4 <= again["n_cells_touched"] <= 8 and again["n_cells_new"] < again["n_cells_touched"] and again["n_occupied"] == info["n_occupied"] + again["n_cells_new"]


def test_upload_round_trip_and_large_counts(gpu_ctx_factory):
    """Upload then download is a round trip of the integers; the records are the restatement's, for counts near 2^20 too (sums of 2^20
    offsets of up to 2^15, of 2^20 products of up to 2^28: far beyond fp32's integers); an insert on top goes on from there."""
    r = np.random.default_rng(3)
    lo, dims = (-2, 0, 3), (5, 4, 3)
    nc = 60
    counts = r.integers(0, 5, nc).astype(np.int32)
    counts[[3, 17, 41]] = (1 << 20) - np.array([0, 1, 7]); counts[5] = 1
    sums = np.zeros((nc, 9), np.int64)
    cn = counts.astype(np.int64)
    sums[:, :3] = r.integers(-32768, 32769, (nc, 3)) * cn[:, None]
    d = r.integers(0, 1 << 28, (nc, 3)) * cn[:, None]
    sums[:, [3, 6, 8]] = d
    sums[:, [4, 5, 7]] = (r.uniform(-0.5, 0.5, (nc, 3)) * np.sqrt(d[:, [0, 0, 1]].astype(f64) * d[:, [1, 2, 2]].astype(f64))).astype(np.int64)
    sums[counts == 0] = 0
    sums[5, 3:] = 0                                              # an occupied cell with a zero trace: S = 0
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create(0.25, lo, dims)
    ctx.voxel_map_upload(counts, sums)
    m = MR.create(0.25, lo, dims)
    MR.upload(m, counts, sums)
    _, _, cells = assert_same_map(ctx, m, "upload")
    assert (counts > 0).sum() == m["n_occupied"] and not cells[5, 3:].any() and cells[5, :3].any() and np.isfinite(cells).all()
    pts, n = crafted()
    shift = np.eye(4, dtype=f32); shift[:3, 3] = (-0.1, 1.6, 1.1)
    info, _ = insert_both(ctx, m, pts[:700], n[:700], shift, "on an uploaded map")
    assert info["n_cells_touched"] > info["n_cells_new"] >= 0 and info["n_cells_touched"] > 3
    bad = counts.copy(); bad[0] = -1
    assert ctx.lib.icp_voxel_map_upload(ctx.h, bad.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)) == ERR_INVALID_ARG
    assert_same_map(ctx, m, "after a refused upload")


def test_refusals(gpu_ctx_factory):
    """No map; more than 2^24 cells; no source; a voxel_size that is not the map's; covariance_k = 0 and a cloud without normals."""
    from icp_amd import binding
    ctx = fresh_ctx(gpu_ctx_factory)
    lib, h = ctx.lib, ctx.h
    pts, n = crafted()
    p = binding.pose_to_c(EYE); o = binding.vgicp_options()
    sums = np.empty(28, f64); cnt = (C.c_int32 * 2)()
    ctx.set_source(pts, n, None)
    for rc in (lib.icp_voxel_map_insert(h, 1, binding._ptr(p), None), lib.icp_get_voxel_map(h, None, None, None, None),
               lib.icp_voxel_map_system(h, binding._ptr(p), C.byref(o), binding._ptr(sums), cnt), lib.icp_voxel_map_align(h, C.byref(o), binding._ptr(p), None, None, 0)):
        assert rc == ERR_INVALID_ARG and "no voxel map" in lib.icp_last_error(h).decode()
    with pytest.raises(binding.IcpError):
        ctx.track_scans_vmap([(pts, n), (pts, n)])
    assert lib.icp_voxel_map_destroy(h) == 0                     # nothing to free: fine
    big = binding.voxel_map_options(0.25, (0, 0, 0), (256, 256, 257))
    assert lib.icp_voxel_map_create(h, C.byref(big)) == ERR_INVALID_ARG and "2^24" in lib.icp_last_error(h).decode()
    assert lib.icp_voxel_map_create(h, C.byref(binding.voxel_map_options(0.0, (0, 0, 0), (2, 2, 2)))) == ERR_INVALID_ARG
    assert lib.icp_get_voxel_map(h, None, None, None, None) == ERR_INVALID_ARG
    # a map, and no source / no target
    ctx2 = fresh_ctx(gpu_ctx_factory)
    ctx2.voxel_map_create(0.25, (-4, -4, -4), (8, 8, 8))
    lib, h = ctx2.lib, ctx2.h
    assert lib.icp_voxel_map_insert(h, 1, binding._ptr(p), None) == ERR_NO_SOURCE and lib.icp_voxel_map_insert(h, 0, binding._ptr(p), None) == ERR_NO_TARGET
    assert lib.icp_voxel_map_insert(h, 2, binding._ptr(p), None) == ERR_INVALID_ARG
    assert lib.icp_voxel_map_align(h, C.byref(o), binding._ptr(p), None, None, 0) == ERR_NO_SOURCE
    assert lib.icp_voxel_map_system(h, binding._ptr(p), C.byref(o), binding._ptr(sums), cnt) == ERR_NO_SOURCE
    ctx2.set_source(pts, n, None)
    o3 = binding.vgicp_options(voxel_size=0.3)
    assert lib.icp_voxel_map_align(h, C.byref(o3), binding._ptr(p), None, None, 0) == ERR_INVALID_ARG and "voxel_size" in lib.icp_last_error(h).decode()
    assert lib.icp_voxel_map_system(h, binding._ptr(p), C.byref(o3), binding._ptr(sums), cnt) == ERR_INVALID_ARG
    assert lib.icp_voxel_map_align(h, C.byref(binding.vgicp_options(min_valid=5)), binding._ptr(p), None, None, 0) == ERR_INVALID_ARG
    assert lib.icp_voxel_map_align(h, C.byref(o), binding._ptr(p), None, None, -1) == ERR_INVALID_ARG
    with pytest.raises(binding.IcpError):
        ctx2.track_scans_vmap([(pts, n), (pts, n)], voxel_size=0.3)
    # k = 0 without normals
    ctx2.set_source(pts, None, None)
    assert lib.icp_voxel_map_insert(h, 1, binding._ptr(p), None) == ERR_INVALID_ARG and "normals" in lib.icp_last_error(h).decode()
    assert lib.icp_voxel_map_align(h, C.byref(o), binding._ptr(p), None, None, 0) == ERR_INVALID_ARG and "normals" in lib.icp_last_error(h).decode()
    with pytest.raises(binding.IcpError):
        ctx2.track_scans_vmap([(pts, n), (pts, None)])
    info, counts, _, _ = ctx2.voxel_map()
    assert info["n_occupied"] == 0 and not counts.any()         # nothing of all this reached the map
    ctx2.voxel_map_destroy()
    assert lib.icp_get_voxel_map(h, None, None, None, None) == ERR_INVALID_ARG


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


def two_insert_map(factory):
    """A context with NO target: the crafted cloud fused at the identity and again, its first 2500 points, at a pose 2 cm and 0.01 rad off;
    the moved source resident.  Returns (ctx, the restatement's map)."""
    pts, n = crafted()
    ctx = fresh_ctx(factory)
    vs, lo, dims = 0.25, (-8, -8, -4), (16, 18, 10)
    ctx.voxel_map_create(vs, lo, dims); m = MR.create(vs, lo, dims)
    insert_both(ctx, m, pts, n, EYE, "map 1")
    insert_both(ctx, m, pts[:2500], n[:2500], pose_of((0.01, -0.008, 0.006), (0.02, -0.015, 0.01)), "map 2")
    ctx.set_source(*moved_source(), None)
    return ctx, m


def test_system_against_the_map(gpu_ctx_factory):
    """The sums of one step against a map of two inserts, with no target set: counts exactly; every sum within n_valid 2^-52 sum |term| of
    the restatement's; two calls give identical bits.  Poses that leave points outside the map, in empty cells and in cells below
    min_points; min_points 1 and 3."""
    ctx, m = two_insert_map(gpu_ctx_factory)
    sp, sn = moved_source()
    seen = []
    for pose in (EYE, pose_of((0.012, -0.009, 0.015), (0.02, -0.015, 0.01)), pose_of((0.3, -0.2, 0.25), (0.8, -0.5, 0.3))):
        for mp in (1, 3):
            sums, counts = ctx.voxel_map_system(pose, voxel_size=0.25, min_points=mp)
            rcounts, rsums, rabs = MR.system(m, sp, sn, pose, EPS, mp)
            bound = rcounts[1] * 2.0 ** -52 * rabs
            err = np.abs(sums - rsums)
            print("system min_points %d: considered %d, valid %d, worst |sum - restatement| / bound = %.3g" % (mp, counts[0], counts[1], float((err / np.maximum(bound, 1e-300)).max())))
            assert tuple(counts) == tuple(rcounts), (counts, rcounts)
            assert (err <= bound).all(), (err, bound)
            again, counts2 = ctx.voxel_map_system(pose, voxel_size=0.25, min_points=mp)
            assert np.array_equal(u64(sums), u64(again)) and tuple(counts2) == tuple(counts)
            seen.append(counts)
    assert all(c[0] == N - 8 for c in seen) and seen[0][1] > seen[1][1] > 1000 and seen[4][1] < 0.8 * seen[0][1]


def test_align_steps_against_the_map(gpu_ctx_factory):
    """8 iterations with the stops off, traced, from two starts, with no target set: iteration i's pose within 1e-5 per element of
    step(system(the DEVICE's pose i - 1)); n_valid exactly; the cost within the summation bound; a second run gives identical bits.  Then
    the stop: with the stops at 1e-3 the trace is bit for bit the head of the full run's and the records past it stay zero; max_trace
    below n_iterations writes that many records; a start 50 m away fails, carries the pose and reports ICP_ERR_NO_CORRESPONDENCES."""
    from icp_amd import binding
    ctx, m = two_insert_map(gpu_ctx_factory)
    sp, sn = moved_source()
    kw = dict(voxel_size=0.25, n_iterations=8, stop_rotation=0.0, stop_translation=0.0)
    for start in (EYE, pose_of((-0.03, 0.025, -0.02), (-0.04, 0.03, 0.035))):
        pose, rec, rc, trace = ctx.voxel_map_align(start, trace=True, **kw)
        assert rc == 0 and rec["status"] == 0 and rec["iterations"] == 8 and len(trace) == 8
        prev = start
        for i, t in enumerate(trace):
            counts, sums, sabs = MR.system(m, sp, sn, prev, EPS)
            want, _ = VR.step(sums, counts, prev)
            diff = float(np.abs(t["pose"] - want).max())
            print("align step %d: n_valid %d, cost %.6g, |pose - restatement| = %.3g" % (i, t["n_valid"], t["cost"], diff))
            assert t["status"] == 0 and t["n_valid"] == counts[1], i
            assert diff <= 1e-5, i
            assert abs(t["cost"] - sums[27]) <= counts[1] * 2.0 ** -52 * sabs[27], i
            prev = t["pose"]
        assert same_bits(pose, trace[-1]["pose"]) and same_bits(rec["pose"], pose)
        assert (rec["n_depth"], rec["n_valid_first"], rec["n_valid_last"]) == (N - 8, trace[0]["n_valid"], trace[-1]["n_valid"]) and rec["cost_last"] < rec["cost_first"]
        pose2, rec2, rc2, trace2 = ctx.voxel_map_align(start, trace=True, **kw)
        assert rc2 == 0 and same_bits(pose2, pose)
        for a, b in zip(trace, trace2):
            assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    full_pose, full_rec, rc, full = ctx.voxel_map_align(EYE, trace=True, stop_rotation=0.0, stop_translation=0.0)
    assert rc == 0 and len(full) == 30
    pose, rec, rc, trace = ctx.voxel_map_align(EYE, trace=True, stop_rotation=1e-3, stop_translation=1e-3)
    ns = rec["iterations"]
    print("stop: %d of 30 iterations" % ns)
    assert rc == 0 and 1 <= ns < 30 and len(trace) == ns and same_bits(pose, trace[-1]["pose"])
    for a, b in zip(trace, full):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    o = binding.vgicp_options(stop_rotation=1e-3, stop_translation=1e-3)
    p = binding.pose_to_c(EYE); r = binding.IcpSdfFrame(); tr = (binding.IcpSdfIter * 30)()
    assert ctx.lib.icp_voxel_map_align(ctx.h, C.byref(o), binding._ptr(p), C.byref(r), tr, 30) == 0
    assert r.iterations == ns and not any(bytes(tr[i]) != bytes(80) for i in range(ns, 30)) and bytes(tr[ns - 1]) != bytes(80)
    tr2 = (binding.IcpSdfIter * 30)(); p = binding.pose_to_c(EYE)
    assert ctx.lib.icp_voxel_map_align(ctx.h, C.byref(o), binding._ptr(p), C.byref(r), tr2, 1) == 0
    assert bytes(tr2[0]) == bytes(tr[0]) and not any(bytes(tr2[i]) != bytes(80) for i in range(1, 30))
    away = pose_of((0.0, 0.0, 0.0), (50.0, 0.0, 0.0))
    pose, rec, rc, trace = ctx.voxel_map_align(away, trace=True)
    assert rc == ERR_NO_CORRESPONDENCES and rec["status"] == rc and same_bits(pose, away) and rec["iterations"] == 1 and rec["n_valid_first"] == 0
    assert "icp_voxel_map_align" in ctx.lib.icp_last_error(ctx.h).decode()


TRACK = dict(voxel_size=MF.VOXEL, n_iterations=6, stop_rotation=0.0, stop_translation=0.0)


@functools.lru_cache(maxsize=None)
def small_scans():
    """6 scans of 43 x 135 points along the fixture's path, each in its sensor frame."""
    return MF.scans(6, (43, 135))


def check_tracked(ctx, scans, start, poses, recs, want_status):
    """Every record against the restatement run from the device's previous pose on the restatement's map, which takes each scan at the
    pose the DEVICE reported: n_depth and n_valid_first exactly, the first cost within the summation bound, the final pose within 1e-5
    per step taken (the bound of one step, test_align_steps_against_the_map, times the steps); the map in the end bit for bit."""
    lo, dims = MF.extent()
    m = MR.create(MF.VOXEL, lo, dims)
    MR.insert(m, scans[0][0], scans[0][1], start)
    prev = start
    for k in range(1, len(scans)):
        rec = recs[k - 1]
        before = (m["counts"].copy(), m["sums"].copy())
        pose, want, _ = MR.align(m, scans[k][0], scans[k][1], prev, EPS, **TRACK)
        counts, sums, sabs = MR.system(m, scans[k][0], scans[k][1], prev, EPS)
        diff = float(np.abs(rec["pose"] - pose).max())
        print("scan %d: status %d, %d iterations, n_valid %d -> %d (restatement %d -> %d), |pose - restatement| = %.3g" % (
            k, rec["status"], rec["iterations"], rec["n_valid_first"], rec["n_valid_last"], want["n_valid_first"], want["n_valid_last"], diff))
        assert rec["status"] == want["status"] == want_status[k - 1], k
        assert (rec["n_depth"], rec["n_valid_first"], rec["iterations"]) == (want["n_depth"], want["n_valid_first"], want["iterations"]), k
        assert same_bits(rec["pose"], poses[k]), k
        if rec["status"] == 0:
            assert abs(rec["cost_first"] - sums[27]) <= counts[1] * 2.0 ** -52 * sabs[27], k
            assert diff <= 1e-5 * rec["iterations"], k
            MR.insert(m, scans[k][0], scans[k][1], rec["pose"])
        else:
            assert same_bits(rec["pose"], prev), k                  # carried
            assert np.array_equal(before[0], m["counts"]) and np.array_equal(before[1], m["sums"])
        prev = rec["pose"]
    assert_same_map(ctx, m, "tracked")
    return m


def test_tracking_matches_restatement(gpu_ctx_factory):
    from icp_amd import binding
    scans = small_scans()
    start = MF.truth(0).astype(f32)
    lo, dims = MF.extent()
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create(MF.VOXEL, lo, dims)
    pose, recs, rc = ctx.track_scans_vmap(scans, start, **TRACK)
    assert rc == 0 and len(recs) == 5 and same_bits(pose, recs[-1]["pose"])
    check_tracked(ctx, scans, start, [start] + [r["pose"] for r in recs], recs, [0] * 5)
    for k, r in enumerate(recs, 1):
        rot, tr = MF.pose_error(r["pose"], MF.truth(k))
        assert rot < 0.02 and tr < 0.05, (k, rot, tr)            # it tracks: a scan's own step is 0.05 rad / 0.175 m
    # the same call again on a fresh map: the same bytes
    ctx.voxel_map_create(MF.VOXEL, lo, dims)
    pose2, recs2, rc2 = ctx.track_scans_vmap(scans, start, **TRACK)
    assert rc2 == 0 and same_bits(pose2, pose) and all(same_bits(a["pose"], b["pose"]) and u64(a["cost_last"]) == u64(b["cost_last"]) for a, b in zip(recs, recs2))
    # eth.track_map is the same call behind an extent of its own
    from icp_amd import eth
    poses3, recs3, rc3 = eth.track_map(ctx, scans, start, voxel_size=MF.VOXEL, extent=(tuple(int(v) for v in lo), tuple(int(v) for v in dims)),
                                       **{k: v for k, v in TRACK.items() if k != "voxel_size"})
    assert rc3 == 0 and len(poses3) == 6 and all(same_bits(a, b["pose"]) for a, b in zip(poses3[1:], recs))
    poses4, _, rc4 = eth.track_map(ctx, scans[:3], start, voxel_size=MF.VOXEL, **{k: v for k, v in TRACK.items() if k != "voxel_size"})
    info = ctx.voxel_map()[0]
    world = scans[0][0].astype(f64) @ start[:3, :3].astype(f64).T + start[:3, 3].astype(f64)
    want = binding.voxel_map_extent(world.min(0) - 2.0, world.max(0) + 2.0, MF.VOXEL)      # extent None: scan 0's bounds at the start pose, grown by the margin
    assert rc4 == 0 and (info["lo"], info["dims"]) == want and len(poses4) == 3


def test_tracking_skips_failed_scans(gpu_ctx_factory):
    """A scan that is all NaN (ICP_ERR_NO_SOURCE) and a scan 50 m away (ICP_ERR_NO_CORRESPONDENCES) among four good ones: each is carried and
    skipped with its status, the first error is returned, the map is what the good scans alone leave."""
    good = small_scans()
    nan = (np.full_like(good[2][0], np.nan), good[2][1])
    far = (good[3][0] + f32(50.0) * np.array([1, 0, 0], f32), good[3][1])
    scans = [good[0], good[1], nan, good[2], far, good[3]]
    start = MF.truth(0).astype(f32)
    ctx = fresh_ctx(gpu_ctx_factory)
    ctx.voxel_map_create(MF.VOXEL, *MF.extent())
    pose, recs, rc = ctx.track_scans_vmap(scans, start, **TRACK)
    assert rc == ERR_NO_SOURCE and [r["status"] for r in recs] == [0, ERR_NO_SOURCE, 0, ERR_NO_CORRESPONDENCES, 0]
    assert "icp_track_scans_vmap" in ctx.lib.icp_last_error(ctx.h).decode()
    assert same_bits(recs[1]["pose"], recs[0]["pose"]) and same_bits(recs[3]["pose"], recs[2]["pose"]) and recs[1]["n_depth"] == 0 and recs[3]["n_valid_first"] == 0
    m = check_tracked(ctx, scans, start, [start] + [r["pose"] for r in recs], recs, [r["status"] for r in recs])
    only_good = MR.create(MF.VOXEL, *MF.extent())
    for (xyz, nrm), P in zip(good[:4], [start, recs[0]["pose"], recs[2]["pose"], recs[4]["pose"]]):
        MR.insert(only_good, xyz, nrm, P)
    assert np.array_equal(only_good["counts"], m["counts"]) and np.array_equal(only_good["sums"], m["sums"])


def use_the_map(ctx):
    """Every new call once, on a context whose clouds are resident."""
    ctx.voxel_map_create(0.5, (-10, -12, -2), (20, 24, 9))
    assert ctx.voxel_map_insert(0, EYE)["n_cells_new"] > 10 and ctx.voxel_map_insert(1, EYE)["n_cells_touched"] > 10
    ctx.voxel_map_system(EYE, voxel_size=0.5)
    _, rec, rc = ctx.voxel_map_align(EYE, voxel_size=0.5, n_iterations=5)
    assert rc == 0 and rec["n_valid_first"] > 64
    ctx.voxel_map()


@pytest.mark.parametrize("metric", [1, 3])
def test_untouched_paths(gpu_ctx_factory, metric):
    """icp_vgicp_align on a target, then icp_run (point-to-plane; GICP with its 20-neighbour normals), on a context that has made every new
    call against a context that never made one: records and poses bit for bit."""
    from icp_amd import synth
    d = synth.eth_like_pair(0, 20, 64)
    runs = []
    for touched in (True, False):
        ctx = gpu_ctx_factory()
        S.configure(ctx, metric=metric, n_iterations=6, max_distance=0.5)
        S.load(ctx, d, colors=False)
        if touched:
            use_the_map(ctx)
        vg = ctx.vgicp_align(EYE, trace=True, voxel_size=0.5, n_iterations=5)
        if touched:
            use_the_map(ctx)
        runs.append((vg, ctx.run(EYE), ctx.voxel_grid(voxel_size=0.5)))
    (va, (pa, ra, rca), ga), (vb, (pb, rb, rcb), gb) = runs
    assert va[2] == vb[2] == 0 and same_bits(va[0], vb[0]) and len(va[3]) == len(vb[3]) == 5
    for a, b in zip(va[3], vb[3]):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    assert {k: v for k, v in va[1].items() if k != "pose"} == {k: v for k, v in vb[1].items() if k != "pose"}
    assert rca == rcb == 0 and same_bits(pa, pb)
    S.assert_same_run(ra, rb)
    assert ga[0] == gb[0] and all(np.array_equal(S.raw_bits(a), S.raw_bits(b)) for a, b in zip(ga[1:], gb[1:]))


def test_outcome_on_the_recorded_fixture(gpu_ctx_factory):
    """The fixture's 12 scans of 86 x 270 points through eth.track_map with its extent and options: the final and the worst pose error at
    most twice the restatement's map figures (tests/golden/vmap_outcome.json: final 1.01e-3 rad / 3.20e-3 m, worst 1.01e-3 rad / 3.85e-3 m)
    and below the pair chain's (final 3.62e-3 rad / 8.91e-3 m, worst 3.64e-3 rad / 8.91e-3 m)."""
    from icp_amd import eth
    with open(MF.GOLDEN) as f:
        gold = json.load(f)
    scans = MF.scans()
    lo, dims = MF.extent()
    ctx = gpu_ctx_factory()
    ctx.set_gicp_options(MF.EPSILON, 0)
    opt = {k: v for k, v in MF.OPTIONS.items() if k != "voxel_size"}
    poses, recs, rc = eth.track_map(ctx, scans, MF.truth(0).astype(f32), voxel_size=MF.VOXEL, extent=(tuple(int(v) for v in lo), tuple(int(v) for v in dims)), **opt)
    e = MF.errors(poses)
    print("outcome: device %s; restatement map %s; chain %s; iterations %s (restatement %s)" % (e, gold["map"], gold["chain"], [r["iterations"] for r in recs], gold["iterations"]))
    assert rc == 0 and len(recs) == MF.N_SCANS - 1 and all(r["status"] == 0 for r in recs)
    assert ctx.voxel_map()[0]["n_occupied"] > 0.9 * gold["n_occupied"]
    for k, v in e.items():
        assert v <= 2 * gold["map"][k], k
        assert v < gold["chain"][k], k
