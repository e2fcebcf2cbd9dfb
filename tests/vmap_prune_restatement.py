"""The local-map contract of include/icp_hip.h (icp_voxel_map_prune, icp_voxel_map_compact, icp_track_scans_vmap_local, and what a hashed
map's room rule, reserve and entries become once slots can be vacated) restated in numpy, on top of vmap_restatement's dense map and
hmap_restatement's hashed one.  A removed cell goes back to the cleared state; the hashed map carries two more numbers, n_vacated and
n_compacted (absent: 0).  Contains no device code."""
import numpy as np

import vgicp_restatement as VR
import vmap_restatement as MR
import hmap_restatement as HR

f32, f64 = np.float32, np.float64
OK = VR.OK
BadOptions = MR.BadOptions
PRUNE_INFO = ("n_removed", "n_occupied", "n_vacated", "n_compacted", "capacity", "n_points_removed")
ZERO_INFO = dict.fromkeys(PRUNE_INFO, 0)


def is_hashed(m):
    return "capacity" in m


def kept(coords, voxel_size, centre, radius):
    """(n,) bool for (n, 3) integer cell coordinates: d_a = ((float)c_a + 0.5f) * vs - centre_a, d2 = (d_x d_x + d_y d_y) + d_z d_z, kept iff
    d2 <= r2 with r2 = radius * radius, every operation rounded to fp32."""
    ce = np.asarray(centre, f32).reshape(3); r = f32(radius); vs = f32(voxel_size)
    if not np.isfinite(ce).all():
        raise BadOptions("centre must be finite")
    if not (np.isfinite(r) and r >= 0):
        raise BadOptions("radius must be finite and >= 0")
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        r2 = f32(r * r)
        d = ((c.astype(f32) + f32(0.5)) * vs).astype(f32) - ce
        d = d.astype(f32)
        sq = (d * d).astype(f32)
        d2 = ((sq[:, 0] + sq[:, 1]).astype(f32) + sq[:, 2]).astype(f32)
    return d2 <= r2


def dense_coords(m, idx):
    dims, lo = np.asarray(m["dims"], np.int64), np.asarray(m["lo"], np.int64)
    idx = np.asarray(idx, np.int64)
    return np.stack([idx % dims[0] + lo[0], (idx // dims[0]) % dims[1] + lo[1], idx // (dims[0] * dims[1]) + lo[2]], 1)


def prune(m, centre, radius):
    """icp_voxel_map_prune on either kind of map, in place.  Returns icp_voxel_map_prune_info as a dict."""
    if is_hashed(m):
        keys = [k for k, e in m["cells"].items() if e[0] > 0]
        keep = kept(np.array(keys, np.int64).reshape(-1, 3), m["voxel_size"], centre, radius)
        gone = [k for k, ok in zip(keys, keep) if not ok]
        pts = sum(m["cells"][k][0] for k in gone)
        for k in gone:
            del m["cells"][k]
        m["n_vacated"] = m.get("n_vacated", 0) + len(gone)
        return dict(n_removed=len(gone), n_occupied=len(m["cells"]), n_vacated=m["n_vacated"], n_compacted=m.get("n_compacted", 0), capacity=m["capacity"],
                    n_points_removed=int(pts))
    occ = np.nonzero(m["counts"] > 0)[0]
    keep = kept(dense_coords(m, occ), m["voxel_size"], centre, radius)
    gone = occ[~keep]
    pts = int(m["counts"][gone].astype(np.int64).sum())
    m["counts"][gone] = 0; m["sums"][gone] = 0; m["cells"][gone] = 0
    m["n_occupied"] = int(m["n_occupied"]) - len(gone)
    return dict(n_removed=len(gone), n_occupied=int(m["n_occupied"]), n_vacated=0, n_compacted=0, capacity=len(m["counts"]), n_points_removed=pts)


def _compacted(m, cap):
    if cap > m["capacity"]:
        m["n_grown"] += 1
    m["capacity"] = cap; m["n_vacated"] = 0; m["n_compacted"] = m.get("n_compacted", 0) + 1


def room(m, n):
    """The room rule before n points go in: capacity >= 2 (occupied + vacated + n).  Where it fails: nothing vacated, the table doubles
    until capacity >= 2 (occupied + n); otherwise it is compacted into the smallest power of two >= capacity with 2 (occupied + n) <=
    0.75 capacity.  BadOptions past 2^26 slots."""
    occ, vac, cap = len(m["cells"]), m.get("n_vacated", 0), m["capacity"]
    if 2 * (occ + vac + n) <= cap:
        return
    if vac == 0:
        return HR._room(m, n)
    while 4 * 2 * (occ + n) > 3 * cap:
        cap *= 2
    if cap > (1 << HR.MAX_LOG2):
        raise BadOptions("more than 2^26 slots")
    _compacted(m, cap)


def insert(m, points, normals, pose):
    """icp_voxel_map_insert on a map that may have been pruned (either kind)."""
    if not is_hashed(m):
        return MR.insert(m, points, normals, pose)
    room(m, len(np.asarray(points)))
    return HR.insert(m, points, normals, pose)       # (its own rule, without the vacated slots, then holds already)


def reserve(m, capacity):
    cap = HR.capacity_for(capacity)
    if cap > m["capacity"]:
        if m.get("n_vacated", 0) > 0:
            _compacted(m, cap)
        else:
            HR.reserve(m, capacity)


def compact(m):
    """icp_voxel_map_compact: the vacated slots dropped at the current capacity; a no-op with none."""
    if m.get("n_vacated", 0) > 0:
        _compacted(m, m["capacity"])


def entries(m):
    return HR.entries(m) if is_hashed(m) else HR.dense_entries(m)


def track_local(m, scans, pose, eps, keep_radius, **kw):
    """icp_track_scans_vmap_local over [(xyz, normals)] on either kind of map: (poses: one per scan, records of scans 1 .., first error,
    prune infos: one per scan, all zero for a skipped scan)."""
    r = f32(keep_radius)
    if not (np.isfinite(r) and r > 0):
        raise BadOptions("keep_radius must be finite and > 0")
    align = HR.align if is_hashed(m) else MR.align
    cur = np.asarray(pose, f32).copy()
    insert(m, scans[0][0], scans[0][1], cur)
    prunes = [prune(m, cur[:3, 3], r)]
    poses, recs, first = [cur.copy()], [], OK
    for xyz, nrm in scans[1:]:
        cur, rec, _ = align(m, xyz, nrm, cur, eps, **kw)
        recs.append(rec); poses.append(cur.copy())
        if rec["status"] == OK:
            insert(m, xyz, nrm, cur)
            prunes.append(prune(m, cur[:3, 3], r))
        else:
            prunes.append(dict(ZERO_INFO))
            if first == OK:
                first = rec["status"]
    return poses, recs, first, prunes


def replay(m, scans, poses, statuses, keep_radius):
    """The map and the prune infos that the inserts and prunes of a tracked sequence leave, GIVEN the poses (one per scan) and the
    statuses of scans 1 .. : what the device's final map is compared with."""
    prunes = []
    for k, ((xyz, nrm), P) in enumerate(zip(scans, poses)):
        if k > 0 and statuses[k - 1] != OK:
            prunes.append(dict(ZERO_INFO)); continue
        P = np.asarray(P, f32)
        insert(m, xyz, nrm, P)
        prunes.append(prune(m, P[:3, 3], f32(keep_radius)))
    return prunes
