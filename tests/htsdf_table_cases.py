"""Crafted key sets and scenes for the hashed TSDF volume's block table (tests/test_htsdf_table_host.py, tests/test_gpu_htsdf_table.py):
blocks found by search with the restated hash so that their probe chains are long, wrap round the end of the table, share one home slot or
sit behind a crowd of fillers; block contents that are a function of the block, so that a block read in place of another shows; and the
blocks, points, frames and views at the first and the last storable block coordinate.  The packing and the hash are hmap_restatement's
(the voxel map and the hashed TSDF share dev_hmap.hpp's helpers); the linear-probing simulation is here.  No device code."""
import functools
import numpy as np

import hmap_restatement as HM
import htsdf_cases as HC
import htsdf_restatement as HR
import tsdf_restatement as TS
from hmap_restatement import pack, home
from icp_amd.synth import tum_K, wavy_depth

f32 = np.float32
CAPACITY, SLOTS = 128, 256                          # block_capacity=128: a pool of 128 blocks behind a table of 256 slots
RANGE = HM.RANGE


# ------------------------------------------------------------------------------------------------ the table, simulated
def occupied(keys_in_order, slots):
    """Linear probing from home(key, slots), one key at a time in the order given: {key: slot}."""
    taken, out = set(), {}
    for k in keys_in_order:
        if k in out:
            continue
        s = home(k, slots)
        while s in taken:
            s = (s + 1) % slots
        taken.add(s); out[k] = s
    return out


def probe_length(key, slot, slots):
    """The slots a lookup of `key` examines when it sits in `slot`."""
    return (slot - home(key, slots)) % slots + 1


def wraps(placed, slots):
    """Whether some key of {key: slot} sits below its home: its chain crossed the last slot."""
    return any(s < home(k, slots) for k, s in placed.items())


def keys_of(coords):
    return [pack(c) for c in np.asarray(coords).reshape(-1, 3)]


@functools.lru_cache(None)
def search_cube():
    """Every block of -40 .. 39 cubed, z slowest, with its home in a 256-slot and in a 512-slot table (numpy uint64 arithmetic wraps as the
    contract's does; the host test recomputes every home that is used with home(), one key at a time)."""
    g = np.arange(-40, 40, dtype=np.int64)
    cz, cy, cx = [a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij")]
    key = ((cz + RANGE).astype(np.uint64) << np.uint64(42)) | ((cy + RANGE).astype(np.uint64) << np.uint64(21)) | (cx + RANGE).astype(np.uint64)
    with np.errstate(over="ignore"):
        m = key * np.uint64(HM.MUL)
    return np.stack([cx, cy, cz], 1), (m >> np.uint64(56)).astype(np.int64), (m >> np.uint64(55)).astype(np.int64)


def _nearest(cells, mask, corner, n=None, skip=()):
    """The blocks of cells[mask] not in `skip`, nearest first to a corner of the cube (ties in the cube's order)."""
    skip = {tuple(c) for c in np.asarray(skip).reshape(-1, 3).tolist()}
    c = cells[mask]
    c = c[np.argsort(((c - np.asarray(corner)) ** 2).sum(1), kind="stable")]
    c = np.array([x for x in c.tolist() if tuple(x) not in skip], np.int32).reshape(-1, 3)
    return c if n is None else c[:n]


def _one_per_home(homes, cells, h, skip=(), far=0, corner=(-40, -40, -40)):
    """For each of the homes the block nearest to the corner that is not in `skip` and lies at least `far` blocks from the origin on some axis."""
    out = []
    for want in homes:
        c = _nearest(cells, h == want, corner, skip=skip)
        out.append(c[np.abs(c).max(1) >= far][0])
    return np.array(out, np.int32).reshape(-1, 3)


LOW, HIGH = (-40, -40, -40), (39, 39, 39)           # WRAP is taken from around the cube's first corner, everything else from around its last


@functools.lru_cache(None)
def sets():
    """dict(WRAP, ONE_HOME, RUN, FULL, NEW255): (n, 3) int32 block coordinates.  WRAP lies around one corner of the search cube and the
    rest around the opposite one, so that a sphere about the first corner keeps WRAP alone."""
    cells, h256, h512 = search_cube()
    wrap = _nearest(cells, h512 == 511, LOW, 40)
    one = _nearest(cells, h256 == 0, HIGH, 40)
    run = _one_per_home(range(100, 148), cells, h256, corner=HIGH)
    full = np.concatenate([wrap, one, run])
    new255 = _one_per_home([255], cells, h256, skip=wrap, corner=HIGH)[0]
    return dict(WRAP=wrap, ONE_HOME=one, RUN=run, FULL=full, NEW255=new255)


FILLER_HOMES = list(range(160, 256)) + list(range(16))      # CROWD's 112 fillers, one per home
LONG_HOMES = set(range(160, 256)) | {0}                     # homes from which a key behind those fillers examines more than 16 slots


@functools.lru_cache(None)
def crowd():
    """dict(fillers (112, 3), junction (8, 3): a 2 x 2 x 2 box of adjacent blocks, base: its first block).  Among the junction's blocks at
    least 5 have their home inside the fillers' run: with the fillers in the table first, each of them lies at slot 16 or beyond.  The
    hash is multiplicative, so the homes of adjacent blocks differ by constants, and EVERY junction of the cube with 5 homes in the run has
    one of them in 1 .. 15 (from where slot 16 is at most 16 slots away).  The junction taken has exactly one such block, with the smallest
    home there is, and lists it LAST: in the order given every displaced block is found after more than 16 slots, and in any order all
    but that one are (their homes lie in LONG_HOMES)."""
    cells, h256, _ = search_cube()
    H = np.full((80, 80, 80), -1, np.int64)                 # [z, y, x] + 40
    H[cells[:, 2] + 40, cells[:, 1] + 40, cells[:, 0] + 40] = h256
    inrun = (H >= 160) | (H <= 15)
    short = (H >= 1) & (H <= 15)

    def box_sum(a):
        a = a.astype(np.int64)
        return sum(a[dz:79 + dz, dy:79 + dy, dx:79 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    good = (box_sum(inrun) >= 5) & (box_sum(short) == 1) & (box_sum(H >= 160) >= 1)
    short_home = np.where(good, box_sum(np.where(short, H, 0)), SLOTS)
    z, y, x = [int(v[0]) for v in np.nonzero(short_home == short_home.min())]
    base = np.array([x - 40, y - 40, z - 40], np.int32)
    junction = HC.box_coords(base, (2, 2, 2))
    hj = np.array([home(k, SLOTS) for k in keys_of(junction)])
    junction = junction[np.argsort((hj >= 1) & (hj <= 15), kind="stable")]
    fillers = _one_per_home(FILLER_HOMES, cells, h256, skip=junction)
    return dict(fillers=fillers, junction=junction, base=base)


@functools.lru_cache(None)
def scene_crowd():
    """dict(scene (42, 3): the blocks of HC.crafted_frame() from HC.TILTED in HC.STRADDLE, sorted; fillers (80, 3): one per home of 80
    consecutive homes from `start`, the start under which the most scene blocks have their home inside the run; each filler at least 8
    blocks from the origin on some axis, where no frame of HC.frames() reaches)."""
    _, rcam = HC.camera()
    blocks, oor = HR.touch(HR.HVolume(**HC.STRADDLE), HC.crafted_frame(), rcam, HC.TILTED)
    scene = np.array(sorted(blocks), np.int32)
    hs = np.array([home(k, SLOTS) for k in keys_of(scene)])
    inside = [int((((hs - s) % SLOTS) < 80).sum()) for s in range(SLOTS)]
    start = int(np.argmax(inside))
    cells, h256, _ = search_cube()
    fillers = _one_per_home([(start + i) % SLOTS for i in range(80)], cells, h256, far=8)
    return dict(scene=scene, fillers=fillers, start=start)


# ------------------------------------------------------------------------------------------------ contents that name their block
def _mix(x):
    """A 32-bit finaliser (Murmur3's) on uint64 arrays."""
    x = x & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def contents(coords, holes=0.0):
    """(tsdf, weight) (B, 8, 8, 8) for the blocks: the value of voxel `l` of block `b` is a hash of (b, l) mapped into (-1.5, 1.5) on a
    2^-16 lattice, its weight one of 1, 2.5, 7 by another hash; holes: the share of weights set to 0 (by a third)."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b = ((c[:, 0] + 64) | ((c[:, 1] + 64) << 7) | ((c[:, 2] + 64) << 14)).astype(np.uint64) & np.uint64(0x1FFFFF)
    l = np.arange(512, dtype=np.uint64)
    seed = _mix(b[:, None] * np.uint64(512) + l[None, :])
    t = ((seed >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.float64) / 65536.0 * 3.0 - 1.5
    w = np.array([1, 2.5, 7], f32)[(_mix(seed + np.uint64(1)) % np.uint64(3)).astype(np.int64)]
    if holes > 0:
        w = np.where((_mix(seed + np.uint64(2)) % np.uint64(10000)).astype(np.float64) < holes * 10000, f32(0), w)
    return t.astype(f32).reshape(-1, 8, 8, 8), w.astype(f32).reshape(-1, 8, 8, 8)


def colours(coords):
    """(rgb (B, 8, 8, 8, 3), cweight (B, 8, 8, 8)) that are a function of block and voxel: whole byte values, weights 1, 2 or 4, 3 % uncoloured."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b = ((c[:, 0] + 64) | ((c[:, 1] + 64) << 7) | ((c[:, 2] + 64) << 14)).astype(np.uint64) & np.uint64(0x1FFFFF)
    seed = _mix(b[:, None] * np.uint64(512) + np.arange(512, dtype=np.uint64)[None, :] + np.uint64(0x5555))
    rgb = np.stack([(_mix(seed + np.uint64(k)) & np.uint64(255)).astype(f32) for k in (3, 4, 5)], -1)
    cw = np.array([1, 2, 4], f32)[(_mix(seed + np.uint64(6)) % np.uint64(3)).astype(np.int64)]
    cw = np.where(_mix(seed + np.uint64(7)) % np.uint64(100) < np.uint64(3), f32(0), cw)
    return rgb.reshape(-1, 8, 8, 8, 3).astype(f32), cw.reshape(-1, 8, 8, 8).astype(f32)


def volume_of(opts, coords, tsdf, weight):
    """The restatement's volume holding exactly these blocks."""
    hv = HR.HVolume(**opts)
    for c, t, w in zip(np.asarray(coords).reshape(-1, 3), tsdf, weight):
        hv.blocks[tuple(int(x) for x in c)] = [np.asarray(t, f32), np.asarray(w, f32)]
    return hv


def sorted_by_key(coords, *arrays):
    """The blocks in icp_get_tsdf_hashed's order: z, then y, then x."""
    c = np.asarray(coords, np.int32).reshape(-1, 3)
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
    return (c[order],) + tuple(a[order] for a in arrays)


def block_lattice_points(opts, coords):
    """One lattice point inside every block (voxel (3, 2, 4) of it, where the eight corners of the cell lie in the block), and its cell."""
    o = np.asarray(opts["origin"], f32); s = f32(opts["voxel_size"])
    cells = np.asarray(coords, np.int64).reshape(-1, 3) * 8 + np.array([3, 2, 4])
    return (o + cells.astype(f32) * s).astype(f32), cells


# ------------------------------------------------------------------------------------------------ part A: the crowded junction
DYADIC = dict(origin=(0.5, -0.25, 1.0), voxel_size=0.125, truncation=0.375)      # q - o exact at lattice points, as in test_sample_in_every_class_of_cell


def junction_cells(seed=23, per_class=400):
    """Cells of CROWD's junction by class -- the cell inside one block, across a face, an edge, the corner (local coordinate 7 on 0, 1, 2, 3
    axes) -- per_class each, with the 27 cells around the junction's centre behind them; fractions on a 1/64 lattice.  Only the junction's
    own eight blocks hold values, so a cell that leaves the junction is invalid: on a crossed axis the first of the two blocks is taken three
    times in four.  Returns (points (n, 3) fp32, cells (n, 3) int64, class (n,))."""
    rng = np.random.default_rng(seed)
    base = crowd()["base"].astype(np.int64)
    cells, cls = [], []
    for n_cross in range(4):
        blk = rng.integers(0, 2, (per_class, 3))
        loc = rng.integers(0, 7, (per_class, 3))
        for i in range(per_class):
            ax = rng.permutation(3)[:n_cross]
            loc[i, ax] = 7
            blk[i, ax] = (rng.random(n_cross) < 0.25).astype(np.int64)
        cells.append((base + blk) * 8 + loc); cls.append(np.full(per_class, n_cross))
    centre = (base + 1) * 8 - 1
    around = np.array([[x, y, z] for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)]) + centre
    cells.append(around); cls.append(((around & 7) == 7).sum(1))
    cells = np.concatenate(cells); cls = np.concatenate(cls)
    frac = rng.integers(0, 64, cells.shape).astype(f32) / f32(64)
    o = np.asarray(DYADIC["origin"], f32); s = f32(DYADIC["voxel_size"])
    pts = (o + (cells.astype(f32) + frac) * s).astype(f32)
    assert np.array_equal(np.floor((pts - o) / s), cells.astype(f32))
    return pts, cells, cls


def junction_view():
    """(depth 64 x 48, pose): a camera 1.4 m in front of the junction's centre, looking along +z at it."""
    o = np.asarray(DYADIC["origin"], np.float64); s = DYADIC["voxel_size"]
    centre = o + (crowd()["base"].astype(np.float64) + 1) * 8 * s
    pose = np.eye(4, dtype=f32)
    pose[:3, 3] = (centre - np.array([0.0, 0.0, 1.4])).astype(f32)
    return wavy_depth(HC.W, HC.H, 1.4), pose


# ------------------------------------------------------------------------------------------------ part B: the first and last storable block
EDGE = dict(origin=(0.0, 0.0, 0.0), voxel_size=1.0, truncation=3.0, max_depth=8.0)      # cell f = floor(q); coordinates up to 2^23 exact
B_HI, B_LO = RANGE - 1, -RANGE
OTHER = (2, 4)                                      # the two coordinates of an edge block that are not at the edge: even, so that the alias is a storable block
SAMPLE_Q = (8388606.5, 8388607.5, -8388607.5, -8388609.0)
SAMPLE_CELL = ((1 << 23) - 2, (1 << 23) - 1, -(1 << 23), -(1 << 23) - 1)
SAMPLE_VALID = (True, False, True, False)
EDGE_W, EDGE_H = 16, 12


def edge_block(axis, end):
    """E+ (end = +1) or E- (end = -1) of an axis."""
    b = [0, 0, 0]
    b[axis] = B_HI if end > 0 else B_LO
    b[(axis + 1) % 3], b[(axis + 2) % 3] = OTHER
    return tuple(b)


def trap_block(axis):
    """The storable block whose key one block past E+ would have, were it packed unmasked: for x, (-2^20, by + 1, bz); for y,
    (bx, -2^20, bz + 1); z has none (its overflow leaves the key's 63 bits)."""
    e = edge_block(axis, +1)
    if axis == 0:
        return (B_LO, e[1] + 1, e[2])
    if axis == 1:
        return (e[0], B_LO, e[2] + 1)
    return None


def unmasked_key(c):
    """hm_key's arithmetic on coordinates that need not be storable: fields OR-ed without a mask, 64 bits kept."""
    x, y, z = (int(v) for v in c)
    return (((z + RANGE) << 42) | ((y + RANGE) << 21) | (x + RANGE)) & ((1 << 64) - 1)


def edge_contents(axis, end):
    """(tsdf, weight) (8, 8, 8) of E+ / E-: observed everywhere (weights 1, 2.5, 7), 0.25 .. 0.75 by a hash of block and voxel, except
    where the local coordinate on the NEXT axis is below 4: there the value falls along `axis` through 0 between local 4 and 5, a
    surface with free space on the low side.  The rest of the block stays positive up to its last layer, so a read one block
    past the edge that found the trap's -0.5 would change signs."""
    b = edge_block(axis, end)
    t, w = contents([b])
    t = (np.abs(t[0]) / f32(3) + f32(0.25)).astype(f32)
    l = np.arange(8)
    la = l.reshape([-1 if a == axis else 1 for a in (2, 1, 0)])                  # arrays are [z, y, x]
    lb = l.reshape([-1 if a == (axis + 1) % 3 else 1 for a in (2, 1, 0)])
    ramp = ((f32(4.5) - la.astype(f32)) * f32(0.25)).astype(f32)
    t = np.where(np.broadcast_to(lb < 4, t.shape), np.broadcast_to(ramp, t.shape), t).astype(f32)
    return t, w[0]


def trap_contents():
    return np.full((8, 8, 8), -0.5, f32), np.ones((8, 8, 8), f32)


def edge_blocks(axis, ends=(+1, -1), trap=True):
    """(coords, tsdf, weight) of the edge blocks of an axis, with the trap block behind them where the axis has one."""
    cc, tt, ww = [], [], []
    for end in ends:
        t, w = edge_contents(axis, end)
        cc.append(edge_block(axis, end)); tt.append(t); ww.append(w)
    if trap and trap_block(axis) is not None:
        t, w = trap_contents()
        cc.append(trap_block(axis)); tt.append(t); ww.append(w)
    return np.array(cc, np.int32), np.stack(tt), np.stack(ww)


def edge_points(axis, per_q=24, seed=31):
    """Points with q_axis in SAMPLE_Q and the other two coordinates inside the edge block (local cell 0 .. 6, fractions on a 1/64 lattice):
    (points (4 per_q, 3) fp32, expected valid (4 per_q,), intended cell on `axis` (4 per_q,))."""
    rng = np.random.default_rng(seed + axis)
    pts, valid, cell = [], [], []
    for q, f, ok in zip(SAMPLE_Q, SAMPLE_CELL, SAMPLE_VALID):
        p = np.zeros((per_q, 3), np.float64)
        p[:, axis] = q
        for k, other in enumerate(((axis + 1) % 3, (axis + 2) % 3)):
            p[:, other] = OTHER[k] * 8 + rng.integers(0, 7, per_q) + rng.integers(0, 64, per_q) / 64.0
        pts.append(p); valid += [ok] * per_q; cell += [f] * per_q
    return np.concatenate(pts).astype(f32), np.array(valid), np.array(cell, np.int64)


def edge_camera(w=EDGE_W, h=EDGE_H):
    from icp_amd import binding
    return binding.depth_camera(tum_K(w), w, h), TS.Camera(tum_K(w), w, h)


# translations along the axis from which the 16 x 12 frame stores blocks at the extreme coordinate (upper end, lower end)
# and, at the upper ends, has samples out of range; y's and the lower z's were picked on the host: x's and z's upper values leave y without a
# sample out of range, and the camera looks along +z, so only a start below the range puts samples of the lower z frame out of it
EDGE_TRANSLATION = {0: (8388604.0, -8388606.0), 1: (8388605.0, -8388607.0), 2: (8388604.0, -8388610.0)}


def edge_frame(axis, end):
    """(depth 16 x 12, pose): wavy_depth seen from a pure translation along `axis`."""
    pose = np.eye(4, dtype=f32)
    pose[axis, 3] = f32(EDGE_TRANSLATION[axis][0 if end > 0 else 1])
    return wavy_depth(EDGE_W, EDGE_H), pose


def edge_view(axis):
    """The pose of a 16 x 12 camera inside E+, two voxels behind its first layer and centred on it, looking along +axis: its rays run through
    the block's last cells and on past the storable range."""
    e = edge_block(axis, +1)
    R = {0: np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]]), 1: np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]]), 2: np.eye(3)}[axis]      # camera z -> +axis
    pose = np.eye(4, dtype=f32)
    pose[:3, :3] = R
    for a in range(3):
        pose[a, 3] = f32(e[a] * 8 + (2.0 if a == axis else 4.0))
    return pose


def edge_view_frame():
    """A 16 x 12 depth frame for edge_view: depths 4.35 .. 5.17 put about half of its points into the block's last storable cells and the
    rest into cell 2^23 - 1 on the axis."""
    return wavy_depth(EDGE_W, EDGE_H, 4.6)
