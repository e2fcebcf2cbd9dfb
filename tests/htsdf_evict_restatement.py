"""Streaming the hashed TSDF volume (include/icp_hip.h) restated in numpy on tests/htsdf_restatement.py's HVolume, which
is imported and not edited: the evict predicate in fp32 operation for operation, evict and insert on the dict of blocks, the view's reach,
and the local tracking loop beside the unbounded one.  Written from the contract alone; contains no table, no pool and no device code."""
import math
import numpy as np

import htsdf_restatement as HR
import sdf_restatement as SR

f32 = np.float32
INFO = ("n_evicted", "n_blocks", "n_moved", "capacity", "n_held", "n_inserted", "n_present", "n_grown")


class BadOptions(ValueError):
    pass


def kept(coords, origin, voxel_size, centre, radius):
    """(n,) bool for (n, 3) block coordinates: p_a = o_a + ((float)(8 b_a) + 3.5f) s, d_a = p_a - centre_a,
    d2 = (d_x d_x + d_y d_y) + d_z d_z, kept iff d2 <= r2 with r2 = radius * radius, every operation rounded to fp32."""
    ce = np.asarray(centre, f32).reshape(3); r = f32(radius); s = f32(voxel_size); o = np.asarray(origin, f32).reshape(3)
    if not np.isfinite(ce).all():
        raise BadOptions("centre must be finite")
    if not (np.isfinite(r) and r >= 0):
        raise BadOptions("radius must be finite and >= 0")
    b = np.asarray(coords, np.int64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        r2 = f32(r * r)
        g = (b * 8).astype(f32) + f32(3.5)
        p = o + (g * s).astype(f32)
        d = (p.astype(f32) - ce).astype(f32)
        sq = (d * d).astype(f32)
        d2 = ((sq[:, 0] + sq[:, 1]).astype(f32) + sq[:, 2]).astype(f32)
    return d2 <= r2


def evict(vol, centre, radius):
    """icp_tsdf_evict_blocks on an HVolume: the blocks that are not kept leave vol.blocks.  Returns (n_evicted, {coords: [tsdf, weight]} of
    the evicted blocks)."""
    keys = list(vol.blocks)
    if not keys:
        kept(np.zeros((0, 3)), vol.o, vol.s, centre, radius)
        return 0, {}
    k = kept(np.array(keys, np.int64), vol.o, vol.s, centre, radius)
    out = {b: vol.blocks.pop(b) for b, m in zip(keys, k) if not m}
    if out:
        vol._box = None
    return len(out), out


def insert(vol, blocks):
    """icp_tsdf_insert_blocks: ADDS {coords: [tsdf, weight]}; a resident key, or one that is not storable, refuses the call with nothing modified."""
    for b in blocks:
        if not all(-HR.RANGE <= x < HR.RANGE for x in b):
            raise BadOptions("a block coordinate is not storable")
    present = [b for b in blocks if b in vol.blocks]
    if present:
        raise BadOptions("%d blocks are resident already" % len(present))
    for b, (t, w) in blocks.items():
        vol.blocks[b] = [np.asarray(t, f32).copy(), np.asarray(w, f32).copy()]
    if blocks:
        vol._box = None


def view_reach(cam, vol):
    """binding.tsdf_view_reach: (max_depth + truncation) sqrt(1 + a_max^2 + b_max^2) + 8 s sqrt(3), in double."""
    a = max(abs(0.0 - cam.cx), abs(cam.width - 1.0 - cam.cx)) / abs(float(cam.fx))
    b = max(abs(0.0 - cam.cy), abs(cam.height - 1.0 - cam.cy)) / abs(float(cam.fy))
    return (float(vol.max_d) + float(vol.trunc)) * math.sqrt(1.0 + a * a + b * b) + 8.0 * float(vol.s) * math.sqrt(3.0)


def track_local(vol, frames, cam, pose0, keep_radius, **kw):
    """tsdf_local.track_depth_sdf_local: HR.track with streaming.  Frame 0 integrated at pose0, then evicted about its translation into the
    store; frame k aligned from the current pose and, on success, the stored blocks within keep_radius of the new translation inserted,
    the frame integrated, the volume evicted.  Returns (poses after every frame, records of frames 1 .., per frame
    dict(n_inserted, n_evicted, n_resident, n_stored), the store: {coords: [tsdf, weight]})."""
    reach = view_reach(cam, vol)
    if not (math.isfinite(reach) and math.isfinite(keep_radius) and keep_radius >= reach):
        raise BadOptions("keep_radius must be finite and at least the view's reach")
    store = {}
    pose = np.asarray(pose0, f32).copy()

    def stream(n_in):
        n_ev, out = evict(vol, pose[:3, 3], keep_radius)
        assert not (set(out) & set(store))
        store.update(out)
        return dict(n_inserted=n_in, n_evicted=n_ev, n_resident=len(vol.blocks), n_stored=len(store))

    HR.integrate(vol, frames[0], cam, pose)
    poses, recs, evs = [pose.copy()], [], [stream(0)]
    for k in range(1, len(frames)):
        pose, rec, _ = SR.align(vol, frames[k], cam, pose, **kw)
        if rec["status"] == SR.OK:
            keys = list(store)
            back = {}
            if keys:
                m = kept(np.array(keys, np.int64), vol.o, vol.s, pose[:3, 3], keep_radius)
                back = {b: store.pop(b) for b, mm in zip(keys, m) if mm}
            insert(vol, back)
            HR.integrate(vol, frames[k], cam, pose)
            evs.append(stream(len(back)))
        else:
            evs.append(dict(n_inserted=0, n_evicted=0, n_resident=0, n_stored=0))
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs, evs, store


def union_blocks(vol, store):
    """The resident and the stored blocks together in icp_get_tsdf_hashed's layout (they never share a key)."""
    assert not (set(vol.blocks) & set(store))
    u = HR.HVolume(**vol.options())
    u.blocks = dict(vol.blocks); u.blocks.update(store)
    return u.sorted_blocks()
