"""The local voxel map on the device: icp_voxel_map_prune, icp_voxel_map_compact and icp_track_scans_vmap_local on both storages.  The
references: EXISTING CODE -- a map that the existing insert builds from the host-filtered cloud, which a pruned map must equal bit for
bit, and the dense map over a covering extent, which the hashed map must equal entry for entry -- and the numpy restatement of the
contract (tests/vmap_prune_restatement.py).  Sweep sizes at the wave and block edges, probe chains through vacated slots, the compaction
rule round by round against the restatement, the tracking loop with and without cells leaving, the refusals, and the paths that must
stay untouched."""
import ctypes as C
import functools
import numpy as np
import pytest

import support as S
import vgicp_restatement as VR
import vmap_restatement as MR
import hmap_restatement as HR
import vmap_prune_restatement as PR
import vmap_outcome_fixture as MF
from support import pose_of, same_bits
from test_gpu_hmap import COVER, EPS, EYE, POSE_A, POSE_B, TRACK, crafted, dense_entries, fresh_ctx, hashed_entries, homes_in_256, same_entries, small_scans, u64, wide_extent

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ERR_INVALID_ARG, ERR_NO_SOURCE = 1, 4
FAR = (1000.0, 0.0, 0.0)                            # prune(FAR, 0) removes everything
ALL = 2e19                                          # a radius whose square is infinite in fp32: removes nothing, returns the counters


def entries_of(ctx, hashed, what=""):
    return hashed_entries(ctx, what)[1] if hashed else dense_entries(ctx)


def make_map(factory, hashed, vs, extent=COVER, capacity=256):
    """(context, restatement) of an empty map."""
    ctx = fresh_ctx(factory)
    if hashed:
        ctx.voxel_map_create_hashed(vs, capacity)
        return ctx, HR.create(vs, capacity)
    ctx.voxel_map_create(vs, *extent)
    return ctx, MR.create(vs, *extent)


def insert_both(ctx, m, pts, nrm, pose, what=""):
    ctx.set_source(pts, nrm, None)
    info = ctx.voxel_map_insert(1, pose)
    want = PR.insert(m, pts, nrm, pose)
    assert info == want, (what, info, want)
    return info


def prune_both(ctx, m, centre, radius, what=""):
    info = ctx.voxel_map_prune(centre, radius)
    want = PR.prune(m, centre, radius)
    print("prune %s: %s" % (what, info))
    assert info == want, (what, info, want)
    return info


def state_is(ctx, m, hashed, what=""):
    """The map of the context against the restatement's: entries bit for bit; for a hashed map capacity, growth, vacated and compacted too."""
    e = entries_of(ctx, hashed, what)
    same_entries(e, PR.entries(m), what)
    if hashed:
        info = ctx.voxel_map_hashed()[0]
        now = ctx.voxel_map_prune((0.0, 0.0, 0.0), ALL)
        assert (info["capacity"], info["n_grown"], info["n_unplaced"]) == (m["capacity"], m["n_grown"], 0), (what, info, m["capacity"], m["n_grown"])
        assert (now["n_removed"], now["n_occupied"], now["n_vacated"], now["n_compacted"], now["capacity"]) == (
            0, len(m["cells"]), m.get("n_vacated", 0), m.get("n_compacted", 0), m["capacity"]), (what, now)
    return e


def surviving(pts, nrm, pose, vs, centre, radius):
    """The points that enter and whose cell the prune keeps (the host's filter for the reference map)."""
    pt = VR.transform_points(pose, pts); nt = VR.transform_normals(pose, nrm)
    ok = np.isfinite(np.asarray(pts, f32)).all(1) & np.isfinite(pt).all(1) & np.isfinite(nt).all(1)
    idx = np.nonzero(ok)[0]
    return idx[PR.kept(VR.cell_coords(pt[idx], vs), vs, centre, radius)]


def block9():
    g = np.arange(9)
    cc = np.stack([a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij")], 1)
    pts = ((cc + 0.5) * 0.25).astype(f32)
    return cc, pts, np.tile(np.array([[0.6, 0.0, 0.8]], f32), (len(pts), 1))


@pytest.mark.parametrize("vs", [0.25, 0.3])
def test_prune_equals_a_map_the_points_never_entered(gpu_ctx_factory, vs):
    """Existing code as the reference.  The crafted cloud at three poses into a dense map over a covering extent and into a hashed map from
    256 slots, then one prune: the info records equal the restatement's; both maps equal, bit for bit (counts, sums, records), the map
    that the EXISTING insert builds in a fresh context from the host-filtered cloud; hashed equals dense equals the restatement."""
    pts, n = crafted()
    for pose in (EYE, pose_of(*POSE_A), pose_of(*POSE_B)):
        world = VR.transform_points(pose, pts[:700])
        centre = np.median(world[np.isfinite(world).all(1)], axis=0).astype(f32)
        radius = 0.9
        idx = surviving(pts, n, pose, vs, centre, radius)
        got = []
        for hashed in (False, True):
            ctx, m = make_map(gpu_ctx_factory, hashed, vs)
            before = insert_both(ctx, m, pts, n, pose, "all")
            info = prune_both(ctx, m, centre, radius, "%s %.2f" % ("hashed" if hashed else "dense", vs))
            assert 0 < info["n_removed"] < before["n_occupied"] and info["n_occupied"] == before["n_occupied"] - info["n_removed"]
            ref, _ = make_map(gpu_ctx_factory, hashed, vs)
            ref.set_source(pts[idx], n[idx], None)
            ri = ref.voxel_map_insert(1, pose)
            assert ri["n_occupied"] == info["n_occupied"] and ri["n_entered"] == len(idx) == before["n_entered"] - before["n_outside"] - info["n_points_removed"]
            e = state_is(ctx, m, hashed, "pruned")
            same_entries(e, entries_of(ref, hashed), "against the existing insert of the filtered cloud")
            got.append(e)
        same_entries(*got, "hashed against dense")


@pytest.mark.parametrize("hashed", [False, True])
def test_exact_boundary_block(gpu_ctx_factory, hashed):
    """Voxel 0.25, the 9 x 9 x 9 block with one point a cell, pruned about the middle cell's centre with 0.75 m: everything is exact in fp32,
    and the kept set is exactly dx^2 + dy^2 + dz^2 <= 9 in cells, the cells ON the sphere included.  Radius 0 then keeps the centre alone."""
    cc, pts, nrm = block9()
    ctx, m = make_map(gpu_ctx_factory, hashed, 0.25)
    insert_both(ctx, m, pts, nrm, EYE)
    info = prune_both(ctx, m, (1.125, 1.125, 1.125), 0.75, "9^3")
    e = state_is(ctx, m, hashed, "9^3")
    want = {tuple(int(v) for v in c) for c in cc if ((c - 4) ** 2).sum() <= 9}
    assert {tuple(int(v) for v in c) for c in e[0]} == want and info["n_occupied"] == 123 and info["n_removed"] == 606 == info["n_points_removed"]
    assert {(7, 4, 4), (1, 4, 4), (6, 6, 5), (2, 3, 2)} <= want
    keep = np.array([tuple(int(v) for v in c) in want for c in cc])
    ref, _ = make_map(gpu_ctx_factory, hashed, 0.25)
    ref.set_source(pts[keep], nrm[keep], None); ref.voxel_map_insert(1, EYE)
    same_entries(e, entries_of(ref, hashed), "against the existing insert")
    zero = prune_both(ctx, m, (1.125, 1.125, 1.125), 0.0, "radius 0")
    assert zero["n_occupied"] == 1 and zero["n_removed"] == 122
    assert [tuple(c) for c in state_is(ctx, m, hashed, "radius 0")[0]] == [(4, 4, 4)]


def line_cells(first, n):
    cc = np.stack([np.arange(first, first + n), np.zeros(n, np.int64), np.zeros(n, np.int64)], 1)
    return ((cc + 0.5) * 0.25).astype(f32), np.tile(np.array([[0.0, 0.6, 0.8]], f32), (n, 1))


@pytest.mark.parametrize("case", ["dense 1", "dense 257", "dense 729", "hashed 1", "hashed 63", "hashed 64", "hashed 65", "hashed 128", "dense empty", "hashed empty"])
def test_sweep_sizes(gpu_ctx_factory, case):
    """One lane, one wave and a lane, a block and a cell, 9^3 cells; 256 slots holding 1 .. 128 cells; an empty map.  A prune that keeps
    about half, a prune that removes everything (a centre 1000 m away, radius 0), and the same insert again: the result equals a fresh
    map with that insert; the hashed map reports the slots it vacated and nothing unplaced."""
    kind, size = case.split()
    hashed = kind == "hashed"
    n = 0 if size == "empty" else int(size)
    extent = ((0, 0, 0), (9, 9, 9)) if n == 729 else ((0, 0, 0), (max(n, 1), 1, 1))
    ctx, m = make_map(gpu_ctx_factory, hashed, 0.25, extent)
    if n == 729:
        _, pts, nrm = block9()
    else:
        pts, nrm = line_cells(0, max(n, 1))
    if n:
        info = insert_both(ctx, m, pts, nrm, EYE, case)
        assert info["n_cells_new"] == n == info["n_occupied"]
        half = prune_both(ctx, m, (0.125, 0.125, 0.125), 1.0 if n == 729 else 0.25 * (n // 2), "half")      # cells 0 .. n // 2 of a line stay
        assert half["n_occupied"] == (n // 2 + 1 if n != 729 else 54)      # (x^2 + y^2 + z^2 <= 16 in cells >= 0: 54 of them)
        state_is(ctx, m, hashed, "half")
    gone = prune_both(ctx, m, FAR, 0.0, "everything")
    assert gone["n_occupied"] == 0 and gone["n_vacated"] == (n if hashed else 0)
    assert len(state_is(ctx, m, hashed, "emptied")[0]) == 0
    again = insert_both(ctx, m, pts, nrm, EYE, "again")
    assert again["n_cells_new"] == len(pts) == again["n_occupied"]
    e = state_is(ctx, m, hashed, "inserted again")
    ref, _ = make_map(gpu_ctx_factory, hashed, 0.25, extent)
    ref.set_source(pts, nrm, None); ref.voxel_map_insert(1, EYE)
    same_entries(e, entries_of(ref, hashed), "a fresh map with that insert")
    if hashed and n:                                 # (2 (0 + n + n) > 256 from n = 65: the insert compacted first; below, the vacated slots stay charged)
        now = ctx.voxel_map_prune((0.0, 0.0, 0.0), ALL)
        assert (now["n_vacated"], now["n_compacted"]) == ((0, 1) if n >= 65 else (n, 0)), now


def test_chains_through_vacated_slots(gpu_ctx_factory):
    """A 256-slot table with 40 cells that share home slot 0 and 40 whose home is slot 255 (the chain wraps).  A prune removes the half of
    them further from the origin; the table keeps its size, so the survivors sit behind vacated slots.  Every survivor is still found (a
    system with one source point per cell has exactly the survivors valid, the removed cells' points alone none), and re-inserting the
    removed cells finds their keys: the entries are exact again and the table is still 256 slots."""
    cells, h = homes_in_256()
    r = np.random.default_rng(11)
    cc = np.concatenate([cells[h == 0][:40], cells[h == 255][:40]])
    assert [HR.home(HR.pack(c), 256) for c in cc] == [0] * 40 + [255] * 40
    cc = cc[r.permutation(80)]
    pts = ((cc + 0.5) * 0.25).astype(f32)
    nrm = r.normal(size=(80, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    d = np.sort(np.linalg.norm(pts.astype(f64), axis=1))
    radius = float(f32(0.5 * (d[39] + d[40])))
    ctx, m = make_map(gpu_ctx_factory, True, 0.25)
    insert_both(ctx, m, pts, nrm, EYE, "chains")
    full = state_is(ctx, m, True, "chains")
    info = prune_both(ctx, m, (0.0, 0.0, 0.0), radius, "the far half")
    keep = PR.kept(cc, 0.25, (0.0, 0.0, 0.0), radius)
    assert info["n_removed"] == 80 - keep.sum() and 32 <= keep.sum() <= 48 and info["capacity"] == 256 and info["n_vacated"] == info["n_removed"]
    homes_kept = {HR.home(HR.pack(c), 256) for c in cc[keep]}
    assert homes_kept == {0, 255}                    # (survivors in both chains)
    e = state_is(ctx, m, True, "pruned")
    assert {tuple(int(v) for v in c) for c in e[0]} == {tuple(int(v) for v in c) for c in cc[keep]}
    sums, counts = ctx.voxel_map_system(EYE, voxel_size=0.25, min_points=1)      # (the source: all 80 points)
    rc, rs, rabs = HR.system(m, pts, nrm, EYE, EPS, 1)
    assert tuple(counts) == (80, int(keep.sum())) == tuple(rc)
    assert (np.abs(sums - rs) <= max(rc[1], 1) * 2.0 ** -52 * rabs).all()
    ctx.set_source(pts[~keep], nrm[~keep], None)
    _, counts = ctx.voxel_map_system(EYE, voxel_size=0.25, min_points=1)
    assert tuple(counts) == (int((~keep).sum()), 0)
    back = insert_both(ctx, m, pts[~keep], nrm[~keep], EYE, "the removed cells again")
    assert back["n_cells_new"] == (~keep).sum() and back["n_occupied"] == 80
    again = state_is(ctx, m, True, "exact again")
    same_entries(again, full, "as before the prune")
    now = ctx.voxel_map_prune((0.0, 0.0, 0.0), ALL)
    assert now["capacity"] == 256 and now["n_compacted"] == 0 and now["n_vacated"] == info["n_removed"]


def shifted(k):
    P = np.eye(4, dtype=f32); P[0, 3] = 50.0 * k
    return P


@functools.lru_cache(maxsize=None)
def compaction_plan():
    """The rounds of the compaction test on the restatement alone: K such that two compactions have happened.  Returns (K, the state after
    every round: (capacity, occupied, vacated, compacted, grown))."""
    pts, n = crafted()
    m = HR.create(0.25, 256)
    states = []
    for k in range(40):
        PR.insert(m, pts, n, shifted(k)); PR.prune(m, shifted(k)[:3, 3], 10.0)
        states.append((m["capacity"], len(m["cells"]), m["n_vacated"], m.get("n_compacted", 0), m["n_grown"]))
        if m.get("n_compacted", 0) >= 2:
            break
    return len(states) - 1, states


def test_compaction(gpu_ctx_factory):
    """From 256 slots: the crafted cloud inserted at a pose shifted by k x 50 m, then a prune about that position with 10 m, k = 0 .. K.
    The restatement alone shows two compactions and a table that ends as large as it was after the second round; the device shows the
    same capacity, vacated and compacted counts at every round, exact entries, nothing unplaced.  Without pruning the same inserts end in
    a strictly larger table.  icp_voxel_map_compact and a reserve with vacated slots leave the entries unchanged."""
    pts, n = crafted()
    K, plan = compaction_plan()
    print("K = %d; (capacity, occupied, vacated, compacted, grown) per round: %s" % (K, plan))
    assert plan[-1][3] >= 2 and plan[-1][0] == plan[1][0]
    ctx, m = make_map(gpu_ctx_factory, True, 0.25)
    for k in range(K + 1):
        insert_both(ctx, m, pts, n, shifted(k), "round %d" % k)
        info = prune_both(ctx, m, shifted(k)[:3, 3], 10.0, "round %d" % k)
        assert (info["capacity"], info["n_occupied"], info["n_vacated"], info["n_compacted"]) == plan[k][:4], (k, info, plan[k])
        if k in (0, 1, K // 2, K):
            state_is(ctx, m, True, "round %d" % k)
    hinfo = ctx.voxel_map_hashed()[0]
    assert hinfo["n_unplaced"] == 0 and hinfo["capacity"] == plan[-1][0] and hinfo["n_grown"] == plan[-1][4]
    plain, pm = make_map(gpu_ctx_factory, True, 0.25)
    for k in range(K + 1):
        plain.set_source(pts, n, None); plain.voxel_map_insert(1, shifted(k)); HR.insert(pm, pts, n, shifted(k))
    grown = plain.voxel_map_hashed()[0]
    print("without pruning: %s; with: %s" % (grown, hinfo))
    assert grown["capacity"] == pm["capacity"] > hinfo["capacity"] and grown["n_occupied"] > hinfo["n_occupied"]
    # compact and reserve with vacated slots
    insert_both(ctx, m, pts[:500], n[:500], shifted(K + 1), "a last round")
    prune_both(ctx, m, shifted(K + 1)[:3, 3], 10.0, "a last round")
    assert m["n_vacated"] > 0
    e = state_is(ctx, m, True, "before compact")
    ctx.voxel_map_compact(); PR.compact(m)
    same_entries(state_is(ctx, m, True, "compacted"), e, "compact keeps the entries")
    ctx.voxel_map_compact(); PR.compact(m)
    state_is(ctx, m, True, "compacted twice")
    prune_both(ctx, m, shifted(K + 1)[:3, 3], 1.2, "a smaller radius")
    assert m["n_vacated"] > 0
    e = state_is(ctx, m, True, "before reserve")
    assert len(e[0]) > 0
    ctx.voxel_map_reserve(m["capacity"]); PR.reserve(m, m["capacity"])
    state_is(ctx, m, True, "reserve to the same size")
    ctx.voxel_map_reserve(2 * m["capacity"]); PR.reserve(m, 2 * m["capacity"])
    assert m["n_vacated"] == 0
    same_entries(state_is(ctx, m, True, "reserved"), e, "reserve keeps the entries")


@functools.lru_cache(maxsize=None)
def near_scans():
    """The six scans as a laser of 3 m range sees them: some 3 200 to 3 700 points each."""
    out = []
    for xyz, nrm in small_scans():
        keep = np.linalg.norm(xyz.astype(f64), axis=1) < 3.0
        out.append((np.ascontiguousarray(xyz[keep]), np.ascontiguousarray(nrm[keep])))
    return out


def same_records(a, b, what=""):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y)
        for i in x:
            same = same_bits(x[i], y[i]) if i == "pose" else (u64(x[i]) == u64(y[i])).all() if isinstance(x[i], float) else x[i] == y[i]
            assert same, (what, k, i, x[i], y[i])


@pytest.mark.parametrize("hashed", [False, True])
def test_tracking_with_a_radius_that_removes_nothing(gpu_ctx_factory, hashed):
    """keep_radius = 50 m around a 3 m laser: no cell ever leaves, and the poses, the records and the final map are bit-identical to
    icp_track_scans_vmap's."""
    scans = near_scans()
    start = MF.truth(0).astype(f32)
    runs = []
    for radius in (None, 50.0):
        ctx = fresh_ctx(gpu_ctx_factory)
        if hashed:
            ctx.voxel_map_create_hashed(MF.VOXEL, 256)
        else:
            ctx.voxel_map_create(MF.VOXEL, *wide_extent())
        out = ctx.track_scans_vmap(scans, start, keep_radius=radius, **TRACK)
        assert len(out) == (3 if radius is None else 4) and out[2] == 0
        runs.append((out, entries_of(ctx, hashed)))
    (a, ea), (b, eb) = runs
    assert same_bits(a[0], b[0])
    same_records(a[1], b[1], "records")
    same_entries(ea, eb, "final map")
    assert len(b[3]) == 6 and all(p["n_removed"] == 0 and p["n_points_removed"] == 0 and p["n_vacated"] == 0 and p["n_occupied"] > 0 for p in b[3]), b[3]
    assert b[3][-1]["n_occupied"] == len(ea[0])


def test_tracking_with_a_local_map(gpu_ctx_factory):
    """keep_radius = 2 m, below the laser's 3 m range, so cells leave on every scan.  The hashed loop (from 256 slots, through
    eth.track_map) against the dense loop over a covering extent: statuses, counts and iterations exactly, poses within 1e-5 per step
    taken (the project's bound for that comparison; the measured difference is printed), equal prune records, final maps equal cell for
    cell.  Both final maps equal the restatement's given the device's poses, exactly, prune record for prune record; every kept cell lies
    within the radius of the last pose and no cell within it that the restatement holds is missing."""
    from icp_amd import eth
    scans = near_scans()
    start = MF.truth(0).astype(f32)
    R = 2.0
    dn, hs = fresh_ctx(gpu_ctx_factory), fresh_ctx(gpu_ctx_factory)
    dn.voxel_map_create(MF.VOXEL, *wide_extent())
    dpose, drecs, drc, dprunes = dn.track_scans_vmap(scans, start, keep_radius=R, **TRACK)
    poses, recs, rc, prunes = eth.track_map(hs, scans, start, voxel_size=MF.VOXEL, hashed=True, capacity=256, keep_radius=R, **{k: v for k, v in TRACK.items() if k != "voxel_size"})
    assert rc == drc == 0 and len(recs) == 5 and len(poses) == 6 and len(prunes) == len(dprunes) == 6
    for k, (a, b) in enumerate(zip(recs, drecs), 1):
        diff = float(np.abs(a["pose"] - b["pose"]).max())
        print("scan %d: %d iterations, n_valid %d -> %d, |pose - dense loop's| = %.3g" % (k, a["iterations"], a["n_valid_first"], a["n_valid_last"], diff))
        assert (a["status"], a["n_depth"], a["n_valid_first"], a["n_valid_last"], a["iterations"]) == (b["status"], b["n_depth"], b["n_valid_first"], b["n_valid_last"], b["iterations"]), k
        assert diff <= 1e-5 * a["iterations"], k
    shared = ("n_removed", "n_occupied", "n_points_removed")
    assert [[p[f] for f in shared] for p in prunes] == [[p[f] for f in shared] for p in dprunes], (prunes, dprunes)
    print("cells removed per scan: %s; occupied after: %s; hashed (capacity, vacated, compacted): %s" % (
        [p["n_removed"] for p in prunes], [p["n_occupied"] for p in prunes], [(p["capacity"], p["n_vacated"], p["n_compacted"]) for p in prunes]))
    info, e = hashed_entries(hs, "tracked")
    de = dense_entries(dn)
    same_entries(e, de, "hashed against the covering dense map")
    # the restatement, given each loop's own poses
    for name, ps, got, pr, m in (("hashed", poses, e, prunes, HR.create(MF.VOXEL, 256)), ("dense", [start] + [r["pose"] for r in drecs], de, dprunes, MR.create(MF.VOXEL, *wide_extent()))):
        want = PR.replay(m, scans, ps, [0] * 5, R)
        assert all(w["n_removed"] > 0 for w in want[1:]), [w["n_removed"] for w in want]
        assert pr == want, (name, pr, want)
        same_entries(got, PR.entries(m), name + " against the restatement")
        last = np.asarray(ps[-1], f32)[:3, 3]
        assert PR.kept(got[0], MF.VOXEL, last, R).all() and len(got[0]) > 100
        held = PR.entries(m)[0]
        inside = held[PR.kept(held, MF.VOXEL, last, R)]
        assert {tuple(c) for c in inside} <= {tuple(c) for c in got[0]}
    assert info["n_unplaced"] == 0


def test_tracking_skips_a_failed_scan(gpu_ctx_factory):
    """A scan that is all NaN in the middle: carried and skipped with its status and an all-zero prune entry, and the map is what the good
    scans, pruned, leave (the restatement given the device's poses), on both storages."""
    good = near_scans()
    nan = (np.full_like(good[2][0], np.nan), good[2][1])
    scans = [good[0], good[1], nan, good[2], good[3]]
    start = MF.truth(0).astype(f32)
    for hashed in (False, True):
        ctx = fresh_ctx(gpu_ctx_factory)
        if hashed:
            ctx.voxel_map_create_hashed(MF.VOXEL, 256); m = HR.create(MF.VOXEL, 256)
        else:
            ctx.voxel_map_create(MF.VOXEL, *wide_extent()); m = MR.create(MF.VOXEL, *wide_extent())
        pose, recs, rc, prunes = ctx.track_scans_vmap(scans, start, keep_radius=2.0, **TRACK)
        st = [r["status"] for r in recs]
        assert rc == ERR_NO_SOURCE and st == [0, ERR_NO_SOURCE, 0, 0] and "icp_track_scans_vmap_local" in ctx.lib.icp_last_error(ctx.h).decode()
        assert same_bits(recs[1]["pose"], recs[0]["pose"]) and prunes[2] == PR.ZERO_INFO and all(p["n_occupied"] > 0 for i, p in enumerate(prunes) if i != 2)
        want = PR.replay(m, scans, [start] + [r["pose"] for r in recs], st, 2.0)
        assert prunes == want, (prunes, want)
        same_entries(entries_of(ctx, hashed), PR.entries(m), "the good scans alone")


def test_eth_track_map_end_to_end(gpu_ctx_factory):
    """eth.track_map(hashed=True, keep_radius=2.0) on the six 3 m scans: four values; every scan tracked; the map is local (every cell within
    2 m of the last pose, fewer cells than the same run keeps without the radius); the poses stay close to the run without it."""
    from icp_amd import eth
    scans = near_scans()
    start = MF.truth(0).astype(f32)
    opt = {k: v for k, v in TRACK.items() if k != "voxel_size"}
    loc, full = fresh_ctx(gpu_ctx_factory), fresh_ctx(gpu_ctx_factory)
    poses, recs, rc, prunes = eth.track_map(loc, scans, start, voxel_size=MF.VOXEL, hashed=True, capacity=256, keep_radius=2.0, **opt)
    fposes, frecs, frc = eth.track_map(full, scans, start, voxel_size=MF.VOXEL, hashed=True, capacity=256, **opt)
    assert rc == frc == 0 and len(poses) == 6 and len(recs) == 5 and len(prunes) == 6 and all(r["status"] == 0 for r in recs)
    info, e = hashed_entries(loc, "local")
    finfo, _ = hashed_entries(full, "full")
    errs = [MF.pose_error(p, MF.truth(k)) for k, p in enumerate(poses)]
    ferrs = [MF.pose_error(p, MF.truth(k)) for k, p in enumerate(fposes)]
    print("local map: %d cells (full: %d), pose errors (rot, tr) %s; without the radius %s" % (info["n_occupied"], finfo["n_occupied"], errs[-1], ferrs[-1]))
    assert info["n_occupied"] == prunes[-1]["n_occupied"] < finfo["n_occupied"] and sum(p["n_removed"] for p in prunes) > 0
    assert PR.kept(e[0], MF.VOXEL, poses[-1][:3, 3], 2.0).all()


def test_refusals_change_nothing(gpu_ctx_factory):
    """Every ICP_ERR_INVALID_ARG of the new calls, with its reason, and the map as it was."""
    from icp_amd import binding
    pts, n = crafted()
    scans = near_scans()[:2]
    for hashed in (False, True):
        ctx = fresh_ctx(gpu_ctx_factory)
        lib, h = ctx.lib, ctx.h
        ce = np.zeros(3, f32)
        prune = lambda c, r: lib.icp_voxel_map_prune(h, np.asarray(c, f32).ctypes.data_as(C.c_void_p), C.c_float(r), None)
        why = lambda: lib.icp_last_error(h).decode()
        assert prune(ce, 1.0) == ERR_INVALID_ARG and "no voxel map" in why()
        assert lib.icp_voxel_map_compact(h) == ERR_INVALID_ARG and "no voxel map" in why()
        m = HR.create(0.25, 256) if hashed else MR.create(0.25, *COVER)
        if hashed:
            ctx.voxel_map_create_hashed(0.25, 256)
        else:
            ctx.voxel_map_create(0.25, *COVER)
        insert_both(ctx, m, pts, n, EYE)
        before = state_is(ctx, m, hashed, "before")
        for c, r, word in (((np.nan, 0, 0), 1.0, "centre"), ((0, np.inf, 0), 1.0, "centre"), ((0, 0, -np.inf), 1.0, "centre"), ((0, 0, 0), -1.0, "radius"),
                           ((0, 0, 0), np.nan, "radius"), ((0, 0, 0), np.inf, "radius")):
            assert prune(c, r) == ERR_INVALID_ARG and word in why(), (c, r, why())
        assert lib.icp_voxel_map_prune(h, None, C.c_float(1.0), None) == ERR_INVALID_ARG and "centre" in why()
        if not hashed:
            assert lib.icp_voxel_map_compact(h) == ERR_INVALID_ARG and "dense" in why()
        o = binding.vgicp_options(**TRACK)
        xs = [binding._f32(s[0]) for s in scans]; ns = [binding._f32(s[1]) for s in scans]
        xp = (C.c_void_p * 2)(*[binding._ptr(a) for a in xs]); npp = (C.c_void_p * 2)(*[binding._ptr(a) for a in ns]); cnt = (C.c_int32 * 2)(*[len(a) for a in xs])
        out = (binding.IcpSdfFrame * 1)(); pr = (binding.IcpVoxelMapPruneInfo * 2)()
        track = lambda r, p: lib.icp_track_scans_vmap_local(h, xp, npp, cnt, 2, C.byref(o), C.c_float(r), binding._ptr(p), out, pr)
        for r in (0.0, -1.0, np.nan, np.inf):
            assert track(r, binding.pose_to_c(EYE)) == ERR_INVALID_ARG and "keep_radius" in why(), r
        bad = EYE.copy(); bad[1, 3] = np.nan
        assert track(2.0, binding.pose_to_c(bad)) == ERR_INVALID_ARG and "translation" in why()
        o3 = binding.vgicp_options(voxel_size=0.3)
        assert lib.icp_track_scans_vmap_local(h, xp, npp, cnt, 2, C.byref(o3), C.c_float(2.0), binding._ptr(binding.pose_to_c(EYE)), out, pr) == ERR_INVALID_ARG and "voxel_size" in why()
        assert lib.icp_track_scans_vmap_local(h, xp, npp, cnt, 0, C.byref(o), C.c_float(2.0), binding._ptr(binding.pose_to_c(EYE)), out, pr) == ERR_INVALID_ARG
        same_entries(state_is(ctx, m, hashed, "after the refusals"), before, "nothing modified")
        # a prune without an info record is enqueued and takes effect all the same
        assert prune((0.125, 0.125, 0.125), 0.6) == 0
        PR.prune(m, (0.125, 0.125, 0.125), 0.6)
        state_is(ctx, m, hashed, "a prune that returns nothing")


def new_calls(ctx, d):
    """Every new call once, on both storages, on a context whose clouds are resident; the clouds are loaded again afterwards (the
    tracking loop leaves its last scan as the source)."""
    sc = [(d["src_pts"], d["src_nrm"]), (d["src_pts"], d["src_nrm"])]
    ctx.voxel_map_create_hashed(0.5, 256)
    assert ctx.voxel_map_insert(0, EYE)["n_cells_new"] > 10 and ctx.voxel_map_insert(1, EYE)["n_cells_touched"] > 10
    a = ctx.voxel_map_prune((0.0, 0.0, 0.0), 3.0)
    assert a["n_removed"] > 0 and a["n_vacated"] == a["n_removed"]
    ctx.voxel_map_compact()
    assert ctx.voxel_map_prune((0.0, 0.0, 0.0), 2.0)["n_compacted"] == 1
    ctx.voxel_map_reserve(1 << 16)
    out = ctx.track_scans_vmap(sc, EYE, keep_radius=4.0, voxel_size=0.5, n_iterations=3)
    assert len(out) == 4 and out[2] == 0
    ctx.voxel_map_create(0.5, (-10, -12, -2), (20, 24, 9))
    ctx.voxel_map_insert(0, EYE)
    assert ctx.voxel_map_prune((0.0, 0.0, 0.0), 3.0)["n_removed"] > 0
    out = ctx.track_scans_vmap(sc, EYE, keep_radius=4.0, voxel_size=0.5, n_iterations=3)
    assert len(out) == 4 and out[2] == 0
    S.load(ctx, d, colors=False)


def map_calls(ctx):
    """The existing map calls on both storages, after the map has been created again."""
    res = []
    for hashed in (False, True):
        if hashed:
            ctx.voxel_map_create_hashed(0.5, 256)
        else:
            ctx.voxel_map_create(0.5, (-10, -12, -2), (20, 24, 9))
        a = ctx.voxel_map_insert(0, EYE); b = ctx.voxel_map_insert(1, EYE)
        sums, counts = ctx.voxel_map_system(EYE, voxel_size=0.5)
        pose, rec, rc = ctx.voxel_map_align(EYE, voxel_size=0.5, n_iterations=5)
        res.append((a, b, sums, tuple(counts), pose, rec, rc, ctx.voxel_map_hashed() if hashed else ctx.voxel_map()))
    return res


@pytest.mark.parametrize("metric", [1, 3])
def test_untouched_paths(gpu_ctx_factory, metric):
    """A context that has made every new call and then created its map again, against a context that never made one: icp_voxel_map_insert,
    _system and _align on both storages, icp_vgicp_align on a target and icp_run return the same bytes."""
    from icp_amd import synth
    d = synth.eth_like_pair(0, 20, 64)
    runs = []
    for touched in (True, False):
        ctx = gpu_ctx_factory()
        S.configure(ctx, metric=metric, n_iterations=6, max_distance=0.5)
        S.load(ctx, d, colors=False)
        if touched:
            new_calls(ctx, d)
        mc = map_calls(ctx)
        if touched:
            new_calls(ctx, d)
        vg = ctx.vgicp_align(EYE, trace=True, voxel_size=0.5, n_iterations=5)
        if touched:
            new_calls(ctx, d)
        runs.append((mc, vg, ctx.run(EYE)))
    (ma, va, (pa, ra, rca)), (mb, vb, (pb, rb, rcb)) = runs
    for da, db in zip(ma, mb):
        assert da[0] == db[0] and da[1] == db[1] and np.array_equal(u64(da[2]), u64(db[2])) and da[3] == db[3] and same_bits(da[4], db[4]) and da[6] == db[6] == 0
        assert {k: v for k, v in da[5].items() if k != "pose"} == {k: v for k, v in db[5].items() if k != "pose"}
        assert da[7][0] == db[7][0] and all(np.array_equal(S.raw_bits(a), S.raw_bits(b)) for a, b in zip(da[7][1:], db[7][1:]))
    assert va[2] == vb[2] == 0 and same_bits(va[0], vb[0]) and len(va[3]) == len(vb[3]) == 5
    for a, b in zip(va[3], vb[3]):
        assert (a["n_valid"], a["status"]) == (b["n_valid"], b["status"]) and u64(a["cost"]) == u64(b["cost"]) and same_bits(a["pose"], b["pose"])
    assert rca == rcb == 0 and same_bits(pa, pb)
    S.assert_same_run(ra, rb)
