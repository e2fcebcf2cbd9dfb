"""The crafted cases of tests/htsdf_table_cases.py checked on the host: every key set has the homes and the size claimed, computed one key
at a time; linear probing occupies the same slots in any insertion order (the device tests lean on it); the displaced blocks are found
after the probes claimed; the inputs at the edge of the storable range are exact in fp32 and fall into the intended cells; the edge
frames store blocks at the extreme coordinate; and tests/htsdf_restatement.py's block-by-block cell equals its boxed one bit for bit."""
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_raycast_restatement as RR
import htsdf_restatement as HR
import htsdf_table_cases as TC
import sdf_restatement as SR
from support import same_bits

f32 = np.float32


def homes(coords, slots=TC.SLOTS):
    return [TC.home(TC.pack(c), slots) for c in coords]


def orders(keys):
    """Three insertion orders: as given, reversed, shuffled."""
    return [list(keys), list(keys)[::-1], [keys[i] for i in np.random.default_rng(9).permutation(len(keys))]]


def test_sets_have_the_homes_claimed():
    S = TC.sets()
    assert homes(S["WRAP"], 512) == [511] * 40 and homes(S["WRAP"]) == [255] * 40
    assert homes(S["ONE_HOME"]) == [0] * 40
    assert homes(S["RUN"]) == list(range(100, 148))
    full = {tuple(c) for c in S["FULL"].tolist()}
    assert len(S["FULL"]) == len(full) == TC.CAPACITY == 128
    assert full == {tuple(c) for k in ("WRAP", "ONE_HOME", "RUN") for c in S[k].tolist()}
    assert homes([S["NEW255"]]) == [255] and tuple(S["NEW255"].tolist()) not in full
    cr = TC.crowd()
    assert homes(cr["fillers"]) == TC.FILLER_HOMES and len(cr["fillers"]) == 112
    j = cr["junction"]
    assert {tuple(c) for c in j.tolist()} == {tuple(c) for c in HC.box_coords(cr["base"], (2, 2, 2)).tolist()}
    assert len({tuple(c) for c in np.concatenate([cr["fillers"], j]).tolist()}) == 120
    sc = TC.scene_crowd()
    _, rcam = HC.camera()
    blocks, _ = HR.touch(HR.HVolume(**HC.STRADDLE), HC.crafted_frame(), rcam, HC.TILTED)
    assert {tuple(c) for c in sc["scene"].tolist()} == blocks and len(blocks) == 42
    assert homes(sc["fillers"]) == [(sc["start"] + i) % 256 for i in range(80)] and sc["start"] == 235
    assert (np.abs(sc["fillers"]).max(1) >= 8).all() and np.abs(sc["scene"]).max() < 8
    for coords in list(S.values()) + [cr["fillers"], j, sc["fillers"]]:
        assert np.abs(coords).max() <= 40
    # the search's vectorised homes are home()'s
    cells, h256, h512 = TC.search_cube()
    pick = np.random.default_rng(1).integers(0, len(cells), 300)
    assert homes(cells[pick]) == h256[pick].tolist() and homes(cells[pick], 512) == h512[pick].tolist()


def test_occupied_slots_do_not_depend_on_the_order():
    """The SET of occupied slots after linear probing is the same for every insertion order (which key sits in which slot is not), in the
    256-slot table and in the 512-slot table a growth rehashes into."""
    S = TC.sets(); cr = TC.crowd(); sc = TC.scene_crowd()
    for name, coords in (("WRAP", S["WRAP"]), ("ONE_HOME", S["ONE_HOME"]), ("RUN", S["RUN"]), ("FULL", S["FULL"]),
                         ("CROWD", np.concatenate([cr["fillers"], cr["junction"]])), ("SCENE_CROWD", np.concatenate([sc["fillers"], sc["scene"]]))):
        keys = TC.keys_of(coords)
        for slots in (256, 512):
            seen = [frozenset(TC.occupied(o, slots).values()) for o in orders(keys)]
            assert seen[0] == seen[1] == seen[2] and len(seen[0]) == len(keys), (name, slots)


def test_chains_are_as_long_as_claimed():
    S = TC.sets(); cr = TC.crowd(); sc = TC.scene_crowd()
    # WRAP: one chain of 40 from the last slot, in both sizes; ONE_HOME: 40 from slot 0; FULL: WRAP and ONE_HOME form one cluster of 80
    for slots in (256, 512):
        p = TC.occupied(TC.keys_of(S["WRAP"]), slots)
        assert sorted(p.values()) == sorted([slots - 1] + list(range(39))) and TC.wraps(p, slots)
    assert sorted(TC.occupied(TC.keys_of(S["ONE_HOME"]), 256).values()) == list(range(40))
    assert sorted(TC.occupied(TC.keys_of(S["RUN"]), 256).values()) == list(range(100, 148))
    for o in orders(TC.keys_of(S["FULL"])):
        p = TC.occupied(o, 256)
        assert sorted(p.values()) == sorted([255] + list(range(79)) + list(range(100, 148))) and TC.wraps(p, 256)
        assert max(TC.probe_length(k, s, 256) for k, s in p.items()) >= 40
    p512 = TC.occupied(TC.keys_of(np.concatenate([S["FULL"], S["NEW255"][None]])), 512)
    assert TC.wraps(p512, 512) and len(p512) == 129
    # CROWD: the fillers first; the junction's blocks whose home lies in the fillers' run sit past slot 15
    fk, jk = TC.keys_of(cr["fillers"]), TC.keys_of(cr["junction"])
    run = set(TC.FILLER_HOMES)
    displaced = [k for k in jk if TC.home(k, 256) in run]
    assert len(displaced) >= 5 and sum(TC.home(k, 256) in TC.LONG_HOMES for k in displaced) == len(displaced) - 1
    p = TC.occupied(fk + jk, 256)
    assert [p[k] for k in fk] == TC.FILLER_HOMES
    lengths = [TC.probe_length(k, p[k], 256) for k in displaced]
    print("CROWD: %d displaced junction blocks, homes %s, slots %s, probes %s" % (len(displaced), [TC.home(k, 256) for k in displaced], [p[k] for k in displaced], lengths))
    assert all(p[k] > 15 for k in displaced) and min(lengths) > 16 and TC.wraps(p, 256)
    assert sum(TC.home(k, 256) >= 160 for k in displaced) >= 1                      # such a block's chain crosses slot 255
    for o in orders(jk):                                                            # any order: all but the one with a home in 1 .. 15
        q = TC.occupied(fk + o, 256)
        assert all(q[k] > 15 for k in displaced)
        assert sum(TC.probe_length(k, q[k], 256) > 16 for k in displaced) >= len(displaced) - 1
    # SCENE_CROWD: at least 16 of the 42 scene blocks behind the fillers' run
    fk, sk = TC.keys_of(sc["fillers"]), TC.keys_of(sc["scene"])
    inside = [k for k in sk if (TC.home(k, 256) - sc["start"]) % 256 < 80]
    p = TC.occupied(fk + sk, 256)
    lengths = [TC.probe_length(k, p[k], 256) for k in inside]
    print("SCENE_CROWD: %d of %d scene blocks displaced, longest probe %d, %d probes beyond 16 slots" % (len(inside), len(sk), max(lengths), sum(l > 16 for l in lengths)))
    assert len(inside) >= 16 and TC.wraps(p, 256)
    end = (sc["start"] + 80) % 256
    assert all((p[k] - end) % 256 < 128 for k in inside)                            # each one past the run's last slot
    assert sum(l > 16 for l in lengths) >= 8


def test_fillers_are_out_of_every_frame():
    """No frame of HC.frames() writes a voxel of SCENE_CROWD's fillers; the three frames together ask for 51 blocks, so with the 80 fillers
    a pool of 128 holds the first frame (38 blocks: 118) and grows once during the second (131)."""
    sc = TC.scene_crowd()
    _, rcam = HC.camera()
    hv = HR.HVolume(**HC.STRADDLE)
    hv.allocate(sc["fillers"])
    n_blocks = []
    for depth, pose in zip(HC.frames(), HC.POSES):
        HR.integrate(hv, depth, rcam, pose)
        n_blocks.append(len(hv.blocks))
    assert all(hv.blocks[tuple(c)][1].max() == 0 for c in sc["fillers"].tolist())
    assert n_blocks == [118, 131, 131] and n_blocks[0] <= TC.CAPACITY < n_blocks[1] <= 2 * TC.CAPACITY
    # the blocks the frames ask for are displaced as the scene's 42 are: the first frame's behind the fillers in the 256-slot table
    first, _ = HR.touch(HR.HVolume(**HC.STRADDLE), HC.frames()[0], rcam, HC.POSES[0])
    p = TC.occupied(TC.keys_of(sc["fillers"]) + TC.keys_of(sorted(first)), 256)
    lengths = [TC.probe_length(k, p[k], 256) for k in TC.keys_of(sorted(first))]
    print("first frame: %d blocks, %d found after more than 16 slots, longest probe %d" % (len(first), sum(l > 16 for l in lengths), max(lengths)))
    assert sum(l > 16 for l in lengths) >= 8 and TC.wraps(p, 256)


def test_contents_name_their_block():
    S = TC.sets()
    t, w = TC.contents(S["FULL"], holes=0.02)
    assert t.dtype == w.dtype == f32 and np.abs(t).max() < 1.5 and set(np.unique(w).tolist()) == {0.0, 1.0, 2.5, 7.0}
    assert 0.01 < (w == 0).mean() < 0.03 and (TC.contents(S["FULL"])[1] > 0).all()
    flat = t.reshape(128, -1)
    assert len({f.tobytes() for f in flat}) == 128
    assert max((flat[i] == flat[j]).mean() for i in range(0, 128, 7) for j in range(i + 1, 128, 11)) < 0.01
    again, _ = TC.contents(S["FULL"][::-1])
    assert same_bits(again[::-1], t)                                                # a function of the block, not of its place
    rgb, cw = TC.colours(S["FULL"])
    assert rgb.shape == (128, 8, 8, 8, 3) and rgb.max() == 255 and rgb.min() == 0 and set(np.unique(cw).tolist()) == {0.0, 1.0, 2.0, 4.0}


def test_edge_inputs_are_exact():
    for x, cell in zip(TC.SAMPLE_Q, TC.SAMPLE_CELL):
        assert float(f32(x)) == x and int(np.floor(f32(x))) == cell
    assert float(f32(-8388608.5)) != -8388608.5                                     # (why the last point is -8388609.0)
    assert float(HR.CELL_HI) == TC.SAMPLE_CELL[0] and float(HR.CELL_LO) == TC.SAMPLE_CELL[2]
    assert TC.SAMPLE_CELL[0] + 1 >> 3 == TC.B_HI and TC.SAMPLE_CELL[2] >> 3 == TC.B_LO
    for axis in range(3):
        pts, valid, cell = TC.edge_points(axis)
        assert pts.dtype == f32 and np.array_equal(np.floor(pts[:, axis]).astype(np.int64), cell)
        for k, other in enumerate(((axis + 1) % 3, (axis + 2) % 3)):
            fl = np.floor(pts[:, other]).astype(np.int64)
            assert ((fl >> 3) == TC.OTHER[k]).all() and ((fl & 7) <= 6).all()
            assert np.array_equal(pts[:, other] * 64, np.round(pts[:, other] * 64))
        for end in (+1, -1):
            _, pose = TC.edge_frame(axis, end)
            assert float(pose[axis, 3]) == TC.EDGE_TRANSLATION[axis][0 if end > 0 else 1]
        view = TC.edge_view(axis)
        assert np.array_equal(view[:3, 3].astype(np.float64), np.array(TC.edge_block(axis, +1)) * 8.0 + np.where(np.arange(3) == axis, 2.0, 4.0))
    # the alias: one block past E+ has, packed without a mask, the key of the trap block
    for axis in (0, 1):
        past = list(TC.edge_block(axis, +1)); past[axis] += 1
        assert TC.unmasked_key(past) == TC.pack(TC.trap_block(axis))
        assert all(v % 2 == 0 for a, v in enumerate(TC.edge_block(axis, +1)) if a != axis)
    pz = list(TC.edge_block(2, +1)); pz[2] += 1
    assert TC.trap_block(2) is None and (((pz[2] + TC.RANGE) << 42) >> 63) == 1      # z's overflow is bit 63: no 63-bit key has it


def test_edge_frames_store_the_extreme_block():
    _, rcam = TC.edge_camera()
    for axis in range(3):
        for end in (+1, -1):
            depth, pose = TC.edge_frame(axis, end)
            hv = HR.HVolume(**TC.EDGE)
            n = HR.integrate(hv, depth, rcam, pose)
            b = np.array(sorted(hv.blocks))
            extreme = TC.B_HI if end > 0 else TC.B_LO
            print("edge frame axis %d end %+d: %d blocks, %d at %d, %d voxels written, %d samples out of range" % (axis, end, len(b), (b[:, axis] == extreme).sum(), extreme, n, hv.n_out_of_range))
            assert (b[:, axis] == extreme).sum() >= 1 and n > 0
            assert (b >= TC.B_LO).all() and (b <= TC.B_HI).all()
            assert hv.n_out_of_range > 0                                            # every end: the translations were picked for it


def test_edge_view_ends_rays_inside_the_block():
    """The ray-cast restatement on E+ alone: some rays end at the surface inside the block, others run on through its last cells and out
    of the storable range; with the trap block beside it the image is the same."""
    _, rcam = TC.edge_camera()
    for axis in (0, 1):
        alone = RR.Blocks(*TC.edge_blocks(axis, ends=(+1,), trap=False), **TC.EDGE)
        both = RR.Blocks(*TC.edge_blocks(axis, ends=(+1,), trap=True), **TC.EDGE)
        trace = {}
        d, v, n, hits = RR.raycast(alone, rcam, TC.edge_view(axis), trace)
        d2, v2, n2, hits2 = RR.raycast(both, rcam, TC.edge_view(axis))
        print("edge view axis %d: %d hits, %d samples, %d out of range" % (axis, hits, trace["samples"], trace["out_of_range"]))
        assert 0 < hits < TC.EDGE_W * TC.EDGE_H and trace["out_of_range"] > 0
        assert hits == hits2 and same_bits(d, d2) and same_bits(v, v2) and same_bits(n, n2)
        a_world = TC.edge_view(axis)[axis, 3] + d[d > 0]
        assert ((a_world >= TC.B_HI * 8) & (a_world < TC.B_HI * 8 + 8)).all()


def test_gathered_cell_equals_the_boxed_cell(monkeypatch):
    """htsdf_restatement._cell's two paths on the inputs of tests/test_htsdf_host.py (NEG after three frames at 6000 lattice points, one
    step's sums on BOX), bit for bit; the edge blocks of an axis with the trap block in one volume take the gathered path, and on the
    edge block alone, whose box is small, both paths agree at the edge points."""
    _, rcam = HC.camera()
    hv = HR.HVolume(**HC.NEG)
    for depth, pose in zip(HC.frames(), HC.POSES):
        HR.integrate(hv, depth, rcam, pose)
    rng = np.random.default_rng(5)
    pts = (np.stack([rng.integers(-1300, 1300, 6000), rng.integers(-1000, 1000, 6000), rng.integers(700, 2800, 6000)], 1).astype(f32) / f32(1024)).astype(f32)
    pts[:4] = [[np.nan, 0, 1], [np.inf, 0, 1], [0, -np.inf, 1], [1e9, 0, 1]]
    assert 0 < HR.box_voxels(hv) <= HR.BOX_LIMIT
    a = HR._cell_box(hv, pts[:, 0], pts[:, 1], pts[:, 2]); b = HR._cell_gather(hv, pts[:, 0], pts[:, 1], pts[:, 2])
    assert np.array_equal(a[0], b[0]) and a[0].sum() > 300 and all(same_bits(x, y) for x, y in zip(a[1:], b[1:]))
    boxed = SR.sample(hv, pts)
    hb = HR.HVolume(**HC.BOX)
    for depth, pose in zip(HC.frames(), HC.POSES):
        HR.integrate(hb, depth, rcam, pose)
    cb, sb, _ = SR.system(hb, HC.crafted_frame(), rcam, HC.POSES[2])
    monkeypatch.setattr(HR, "BOX_LIMIT", 0)
    gathered = SR.sample(hv, pts)
    assert np.array_equal(boxed[2], gathered[2]) and same_bits(boxed[0], gathered[0]) and same_bits(boxed[1], gathered[1])
    cg, sg, _ = SR.system(hb, HC.crafted_frame(), rcam, HC.POSES[2])
    assert cb == cg and cb[1] > 500 and np.array_equal(sb.view(np.uint64), sg.view(np.uint64))
    monkeypatch.undo()
    empty = HR.HVolume(**HC.NEG)
    assert not HR._cell_gather(empty, pts[:, 0], pts[:, 1], pts[:, 2])[0].any() and not HR._cell_box(empty, pts[:, 0], pts[:, 1], pts[:, 2])[0].any()
    for axis in range(3):
        pts, valid, _ = TC.edge_points(axis)
        wide = TC.volume_of(TC.EDGE, *TC.edge_blocks(axis))
        assert HR.box_voxels(wide) > HR.BOX_LIMIT
        F, G, ok = SR.sample(wide, pts)
        assert np.array_equal(ok.astype(bool), valid) and (F[~valid] == 0).all() and (G[~valid] == 0).all()
        for end, sel in ((+1, slice(0, len(pts) // 2)), (-1, slice(len(pts) // 2, None))):
            one = TC.volume_of(TC.EDGE, *TC.edge_blocks(axis, ends=(end,), trap=False))
            assert HR.box_voxels(one) == 512
            p = pts[sel]
            x = HR._cell_box(one, p[:, 0], p[:, 1], p[:, 2]); y = HR._cell_gather(one, p[:, 0], p[:, 1], p[:, 2])
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[0], valid[sel]) and all(same_bits(u, v) for u, v in zip(x[1:], y[1:]))
            Fo, Go, oko = SR.sample(one, p)
            assert np.array_equal(oko, ok[sel]) and same_bits(Fo, F[sel]) and same_bits(Go, G[sel])
