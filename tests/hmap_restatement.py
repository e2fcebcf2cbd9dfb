"""The hashed voxel map contract of include/icp_hip.h (icp_voxel_map_create_hashed / reserve / upload_hashed, icp_get_voxel_map_hashed, and
the insert, system, align and tracking calls on a hashed map) restated in numpy.  The map is a Python dict keyed by the cell's coordinates:
what the contract pins is the set of (key, count, sums, record), not where a cell is stored.  Every piece of arithmetic the hashed map shares
with the dense one -- the cell rule, the quantisation, the record, the sums of a step, the step and the stop -- is vgicp_restatement's and
vmap_restatement's, called here on a dense box around the cells concerned.  The key packing and the home-slot function are restated too, so
that tests can craft collisions.  Contains no device code."""
import numpy as np

import vgicp_restatement as VR
import vmap_restatement as MR

f32, f64 = np.float32, np.float64
OK = VR.OK
INFO = MR.INFO
RANGE = 1 << 20
EMPTY = (1 << 64) - 1
MUL = 0x9E3779B97F4A7C15
MIN_LOG2, MAX_LOG2 = 8, 26
BadOptions = MR.BadOptions


def storable(c):
    """(n,) bool: -2^20 <= c_a < 2^20 on every axis of the (n, 3) integer coordinates."""
    c = np.asarray(c, np.int64).reshape(-1, 3)
    return ((c >= -RANGE) & (c < RANGE)).all(1)


def pack(c):
    """The key of one storable cell (a Python int)."""
    x, y, z = (int(v) for v in c)
    assert all(-RANGE <= v < RANGE for v in (x, y, z))
    return ((z + RANGE) << 42) | ((y + RANGE) << 21) | (x + RANGE)


def unpack(key):
    return tuple(((int(key) >> (21 * a)) & 0x1FFFFF) - RANGE for a in range(3))


def home(key, capacity):
    """The home slot of a key in a table of `capacity` slots (a power of two)."""
    log2 = int(capacity).bit_length() - 1
    assert 1 << log2 == capacity
    return ((int(key) * MUL) & EMPTY) >> (64 - log2)


def capacity_for(capacity):
    """The capacity a request becomes: the next power of two, 2^8 at least; BadOptions outside 1 .. 2^26."""
    if capacity < 1 or capacity > (1 << MAX_LOG2):
        raise BadOptions("capacity must be in 1 .. 2^26")
    log2 = MIN_LOG2
    while (1 << log2) < capacity:
        log2 += 1
    return 1 << log2


def create(voxel_size, capacity=1 << 16):
    """icp_voxel_map_create_hashed: dict(voxel_size, capacity, cells {(x, y, z): [count, sums (9,) int64, record (9,) fp32]}, n_grown)."""
    vs = f32(voxel_size)
    if not (np.isfinite(vs) and vs > 0):
        raise BadOptions("voxel_size must be finite and > 0")
    return dict(voxel_size=vs, capacity=capacity_for(capacity), cells={}, n_grown=0)


def _room(m, n):
    """The room rule with the exact count: capacity >= 2 (occupied + n), doubling; BadOptions past 2^26."""
    need = 2 * (len(m["cells"]) + n)
    cap = m["capacity"]
    while cap < need:
        cap *= 2
    if cap > (1 << MAX_LOG2):
        raise BadOptions("more than 2^26 slots")
    if cap != m["capacity"]:
        m["capacity"] = cap; m["n_grown"] += 1


def reserve(m, capacity):
    cap = capacity_for(capacity)
    if cap > m["capacity"]:
        m["capacity"] = cap; m["n_grown"] += 1


def dense(m, coords=None):
    """The cells `coords` (every cell by default) as vmap_restatement's dense map over their bounding box: (map, index of each cell)."""
    cc = np.array(sorted(m["cells"]) if coords is None else [tuple(c) for c in coords], np.int64).reshape(-1, 3)
    if len(cc) == 0:
        return MR.create(m["voxel_size"], (0, 0, 0), (1, 1, 1)), np.zeros(0, np.int64)
    lo = cc.min(0); dims = cc.max(0) - lo + 1
    d = MR.create(m["voxel_size"], lo, dims)
    rel = cc - lo
    idx = (rel[:, 2] * dims[1] + rel[:, 1]) * dims[0] + rel[:, 0]
    for i, c in zip(idx, cc):
        e = m["cells"].get(tuple(int(v) for v in c))
        if e is not None:
            d["counts"][i] = e[0]; d["sums"][i] = e[1]; d["cells"][i] = e[2]
    d["n_occupied"] = int((d["counts"] > 0).sum())
    return d, idx


def _records(m, coords):
    """The records of the cells `coords` from their counts and sums: vmap_restatement.records on a box around them (one box per cell
    where one box around all of them would be too large)."""
    coords = [tuple(int(v) for v in c) for c in coords]
    if not coords:
        return
    cc = np.array(coords, np.int64)
    span = cc.max(0) - cc.min(0) + 1
    groups = [coords] if int(span[0]) * int(span[1]) * int(span[2]) <= (1 << 22) else [[c] for c in coords]
    for g in groups:
        d, idx = dense(m, g)
        MR.records(d, idx)
        for i, c in zip(idx, g):
            m["cells"][c][2] = d["cells"][i].copy()


def insert(m, points, normals, pose):
    """icp_voxel_map_insert on a hashed map, in place.  Returns icp_voxel_map_insert_info as a dict."""
    p = np.asarray(points, f32); n = np.asarray(normals, f32)
    _room(m, len(p))
    considered = np.isfinite(p).all(1)
    pt = VR.transform_points(pose, p); nt = VR.transform_normals(pose, n)
    enters = considered & np.isfinite(pt).all(1) & np.isfinite(nt).all(1)
    c, q, mm = VR.quantise(pt[enters], nt[enters], m["voxel_size"])
    inside = storable(c)
    add = np.concatenate([q, mm], 1)[inside]
    uc, inv = np.unique(c[inside], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    cnt = np.zeros(len(uc), np.int64); sm = np.zeros((len(uc), 9), np.int64)
    np.add.at(cnt, inv, 1); np.add.at(sm, inv, add)
    new = 0
    touched = []
    for k, cell in enumerate(uc):
        key = tuple(int(v) for v in cell)
        e = m["cells"].get(key)
        if e is None:
            e = m["cells"][key] = [0, np.zeros(9, np.int64), np.zeros(9, f32)]
            new += 1
        e[0] += int(cnt[k]); e[1] = e[1] + sm[k]
        touched.append(key)
    _records(m, touched)
    return dict(n_considered=int(considered.sum()), n_entered=int(enters.sum()), n_outside=int((~inside).sum()), n_cells_touched=len(touched),
                n_cells_new=new, n_occupied=len(m["cells"]))


def upload(m, coords, counts, sums):
    """icp_voxel_map_upload_hashed: the state replaced by the entries (count 0: not stored), every record computed."""
    cc = np.asarray(coords, np.int64).reshape(-1, 3); cn = np.asarray(counts, np.int64).reshape(-1); sm = np.asarray(sums, np.int64).reshape(-1, 9)
    if (cn < 0).any() or not storable(cc).all() or len(np.unique(cc, axis=0)) != len(cc):
        raise BadOptions("a negative count, a coordinate that is not storable, or a coordinate twice")
    m["cells"] = {}
    _room(m, len(cc))
    for c, k, s in zip(cc, cn, sm):
        if k > 0:
            m["cells"][tuple(int(v) for v in c)] = [int(k), s.copy(), np.zeros(9, f32)]
    _records(m, list(m["cells"]))


def entries(m):
    """icp_get_voxel_map_hashed: (coords (n, 3) int32, counts (n,) int32, sums (n, 9) int64, cells (n, 9) fp32), sorted by key."""
    keys = sorted(m["cells"], key=pack)
    n = len(keys)
    coords = np.array(keys, np.int32).reshape(n, 3)
    counts = np.array([m["cells"][k][0] for k in keys], np.int32)
    sums = np.array([m["cells"][k][1] for k in keys], np.int64).reshape(n, 9)
    cells = np.array([m["cells"][k][2] for k in keys], f32).reshape(n, 9)
    return coords, counts, sums, cells


def dense_entries(d):
    """The occupied cells of vmap_restatement's (or the device's) dense map (lo, dims, counts, sums, cells) as `entries` gives them: the
    dense index order is the key order."""
    lo = np.asarray(d["lo"], np.int64); dims = np.asarray(d["dims"], np.int64)
    occ = np.nonzero(np.asarray(d["counts"]) > 0)[0]
    coords = np.stack([occ % dims[0] + lo[0], (occ // dims[0]) % dims[1] + lo[1], occ // (dims[0] * dims[1]) + lo[2]], 1).astype(np.int32)
    return coords, np.asarray(d["counts"])[occ].astype(np.int32), np.asarray(d["sums"])[occ], np.asarray(d["cells"])[occ]


def system(m, src, src_normals, pose, eps, min_points=1, **_):
    """icp_voxel_map_system on a hashed map: vgicp_restatement.system on the box around the occupied cells (a point whose cell is not
    storable, or not in the map, is not valid either way)."""
    return VR.system(dense(m)[0], src, src_normals, pose, eps, min_points)


def align(m, src, src_normals, pose, eps, **kw):
    return VR.align(dense(m)[0], src, src_normals, pose, eps, **kw)


def track(m, scans, pose, eps, **kw):
    """icp_track_scans_vmap on a hashed map: vmap_restatement.track's loop."""
    cur = np.asarray(pose, f32).copy()
    insert(m, scans[0][0], scans[0][1], cur)
    poses, recs, first = [cur.copy()], [], OK
    for xyz, nrm in scans[1:]:
        cur, rec, _ = align(m, xyz, nrm, cur, eps, **kw)
        recs.append(rec); poses.append(cur.copy())
        if rec["status"] == OK:
            insert(m, xyz, nrm, cur)
        elif first == OK:
            first = rec["status"]
    return poses, recs, first
