"""Direct SDF tracking on a hashed TSDF volume that holds only what is in reach: after every fused frame the blocks
beyond `keep_radius` of the camera are streamed out to a host-side `BlockStore`, and the stored blocks within it are streamed in again
before the next frame is fused.  Device memory and the integrate's cost are then bounded by the radius, the model is complete on the host,
and with keep_radius >= reach + the largest step between consecutive poses the poses and records are bit for bit those of
`Context.track_depth_sdf` on an unbounded hashed volume.  A composition of public calls: the store is host memory.
A coloured hashed volume streams its colours with its blocks: the store keeps them when it is given them."""
import numpy as np

from . import binding

f32 = np.float32


def block_centres_kept(coords, centre, radius, origin, voxel_size):
    """icp_tsdf_evict_blocks' predicate in numpy fp32, operation for operation: (n,) bool for (n, 3) block coordinates."""
    ce = np.asarray(centre, f32).reshape(3); o = np.asarray(origin, f32).reshape(3); s = f32(voxel_size); r = f32(radius)
    if not np.isfinite(ce).all():
        raise ValueError("centre must be finite")
    if not (np.isfinite(r) and r >= 0):
        raise ValueError("radius must be finite and >= 0")
    b = np.asarray(coords, np.int64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        r2 = f32(r * r)
        p = (o + (((8 * b).astype(f32) + f32(3.5)) * s).astype(f32)).astype(f32)
        d = (p - ce).astype(f32)
        sq = (d * d).astype(f32)
        d2 = ((sq[:, 0] + sq[:, 1]).astype(f32) + sq[:, 2]).astype(f32)
    return d2 <= r2


class BlockStore:
    """The blocks that are not on the device: a host dictionary from block coordinates (bx, by, bz) to (tsdf, weight), each (8, 8, 8)
    float32 indexed [z, y, x] -- and, once blocks were added with colours, to (tsdf, weight, rgb (8, 8, 8, 3), cweight (8, 8, 8)).  A store
    holds blocks of one kind: `colored` says which (None while it is empty and has held nothing)."""

    def __init__(self):
        self._blocks = {}
        self.colored = None

    def __len__(self):
        return len(self._blocks)

    @property
    def nbytes(self):
        return len(self._blocks) * (12288 if self.colored else 4096)

    def add(self, coords, tsdf, weight, rgb=None, cweight=None):
        """Stores the blocks `coords` (n, 3) with `tsdf` and `weight` (n, 8, 8, 8), copied; with `rgb` (n, 8, 8, 8, 3) and `cweight`
        (n, 8, 8, 8), their colours too.  A key the store holds already raises: a block is either on the device or here, never both;
        blocks with colours into a store of blocks without, or the reverse, is a ValueError."""
        cc = np.asarray(coords, np.int64).reshape(-1, 3)
        t = np.asarray(tsdf, f32).reshape(-1, 8, 8, 8); w = np.asarray(weight, f32).reshape(-1, 8, 8, 8)
        if not (len(cc) == len(t) == len(w)):
            raise ValueError("coords (n, 3), tsdf and weight (n, 8, 8, 8) must agree in n")
        if (rgb is None) != (cweight is None):
            raise ValueError("rgb and cweight go together")
        colored = rgb is not None
        if self.colored is not None and self.colored != colored:
            raise ValueError("the store holds blocks %s colours: it cannot take blocks %s" % (("with", "without") if self.colored else ("without", "with")))
        if colored:
            c = np.asarray(rgb, f32).reshape(-1, 8, 8, 8, 3); cw = np.asarray(cweight, f32).reshape(-1, 8, 8, 8)
            if not (len(cc) == len(c) == len(cw)):
                raise ValueError("coords (n, 3), rgb (n, 8, 8, 8, 3) and cweight (n, 8, 8, 8) must agree in n")
        keys = [tuple(int(x) for x in b) for b in cc]
        for k in keys:
            if k in self._blocks:
                raise KeyError("block %s is in the store already" % (k,))
        if len(set(keys)) != len(keys):
            raise KeyError("a block coordinate occurs twice")
        self.colored = colored
        for i, k in enumerate(keys):
            self._blocks[k] = (t[i].copy(), w[i].copy()) + ((c[i].copy(), cw[i].copy()) if colored else ())

    def _pack(self, keys, blocks):
        shapes = ((8, 8, 8), (8, 8, 8)) + (((8, 8, 8, 3), (8, 8, 8)) if self.colored else ())
        if not keys:
            return (np.zeros((0, 3), np.int32),) + tuple(np.zeros((0,) + sh, f32) for sh in shapes)
        return (np.array(keys, np.int32),) + tuple(np.stack([blocks[k][j] for k in keys]) for j in range(len(shapes)))

    def take_within(self, centre, radius, origin, voxel_size):
        """Removes and returns the stored blocks that icp_tsdf_evict_blocks(centre, radius) would keep, as (coords, tsdf, weight) -- with
        (rgb, cweight) behind them from a store of coloured blocks -- sorted by key."""
        keys = sorted(self._blocks, key=lambda b: (b[2], b[1], b[0]))
        if not keys:
            return self._pack([], {})
        keep = block_centres_kept(np.array(keys, np.int64), centre, radius, origin, voxel_size)
        out = [k for k, m in zip(keys, keep) if m]
        packed = self._pack(out, self._blocks)
        for k in out:
            del self._blocks[k]
        return packed

    def blocks(self):
        """(coords (n, 3) int32, tsdf, weight (n, 8, 8, 8)) of everything stored -- with (rgb (n, 8, 8, 8, 3), cweight (n, 8, 8, 8)) behind them
        from a store of coloured blocks --, sorted by key (z, then y, then x)."""
        return self._pack(sorted(self._blocks, key=lambda b: (b[2], b[1], b[0])), self._blocks)


EVICT_RECORD = ("n_inserted", "n_evicted", "n_moved", "n_resident", "n_stored", "capacity")


def track_depth_sdf_local(ctx, frames, cam, keep_radius, pose=None, store=None, rgbx_frames=None, color_weight=0.0, color_huber=0.0, **sdf_options):
    """`Context.track_depth_sdf` on the context's hashed volume (it exists) with streaming: frame 0 is integrated at `pose` (identity by
    default) and the volume evicted about the pose's translation; frame k is aligned from the previous pose and, on success, the stored
    blocks within keep_radius of the new translation are inserted, the frame integrated, and the volume evicted about that translation
    into the store.  A failed frame is carried and skipped: no insert, no integrate, no evict, an all-zero evict record.
    keep_radius below `binding.tsdf_view_reach(cam, options)` is a ValueError, and so is an infinite reach (set max_depth).
    rgbx_frames (n, h*w, 4), on a COLOURED hashed volume: every frame is fused with its colours, the colours stream with their blocks (the
    reach is the same: the colour is read and written only in cells and voxels the geometry touches), and with color_weight > 0 every
    frame is aligned with the photometric term (color_huber: its Huber bound), as `Context.track_depth_sdf` does; the records are then the
    colour ones.  rgbx_frames on a volume without colours, or color_weight > 0 without rgbx_frames, is a ValueError.
    Returns (pose, records of frames 1 .., status: the first failed frame's or 0, evict records of frames 0 .. as dicts of EVICT_RECORD, store)."""
    o = ctx.tsdf_hashed_options
    reach = binding.tsdf_view_reach(cam, o)
    if not np.isfinite(reach):
        raise ValueError("the view's reach is infinite: create the volume with a finite max_depth")
    if not (np.isfinite(keep_radius) and keep_radius >= reach):
        raise ValueError("keep_radius %g is below the reach of a frame, %g (binding.tsdf_view_reach): the frame's own blocks would leave" % (keep_radius, reach))
    # the integrate rounds a voxel's projection to the nearest pixel, so it reaches half a pixel past the outermost pixel centres; the
    # reach's block diagonal of slack (8 s sqrt(3), of which the derivation uses 4.5) covers that as long as the half pixel is small
    half_pixel = (float(o.max_depth) + float(o.truncation)) * 0.5 * (1.0 / abs(cam.fx) + 1.0 / abs(cam.fy))
    if half_pixel > 3.5 * float(o.voxel_size) * np.sqrt(3.0):
        raise ValueError("a pixel at max_depth + truncation is wider than the reach's slack covers (%g m against %g m): use smaller max_depth or larger voxels"
                         % (2 * half_pixel, 7.0 * float(o.voxel_size) * np.sqrt(3.0)))
    colored = rgbx_frames is not None
    if colored and not ctx.tsdf_has_color():
        raise ValueError("rgbx_frames need a coloured hashed volume: create it with tsdf_create_hashed(color=True)")
    if color_weight != 0 and not colored:
        raise ValueError("color_weight > 0 needs the frames' colour frames (rgbx_frames)")
    photo = dict(rgbx=None, color_weight=0.0, color_huber=0.0)
    store = BlockStore() if store is None else store
    origin, vs = tuple(o.origin), o.voxel_size
    frames = np.asarray(frames)
    pose = np.eye(4, dtype=f32) if pose is None else np.asarray(pose, f32).copy()

    def stream(pose, n_inserted):
        info, *ev = (ctx.tsdf_evict_blocks_color if colored else ctx.tsdf_evict_blocks)(pose[:3, 3], keep_radius, hold=True)
        store.add(*ev)
        return dict(n_inserted=n_inserted, n_evicted=info["n_evicted"], n_moved=info["n_moved"], n_resident=info["n_blocks"], n_stored=len(store), capacity=info["capacity"])

    ctx.tsdf_integrate(frames[0], cam, pose, rgbx=rgbx_frames[0] if colored else None)
    evs = [stream(pose, 0)]
    recs, status = [], 0
    for k in range(1, len(frames)):
        if colored:
            photo = dict(rgbx=rgbx_frames[k], color_weight=color_weight, color_huber=color_huber)
        pose, rec, rc = ctx.tsdf_align_depth(frames[k], cam, pose, **photo, **sdf_options)
        recs.append(rec)
        if rc != 0:
            status = status or rc
            evs.append(dict.fromkeys(EVICT_RECORD, 0))
            continue
        ins = store.take_within(pose[:3, 3], keep_radius, origin, vs)
        if len(ins[0]):
            (ctx.tsdf_insert_blocks_color if colored else ctx.tsdf_insert_blocks)(*ins)
        ctx.tsdf_integrate(frames[k], cam, pose, rgbx=rgbx_frames[k] if colored else None)
        evs.append(stream(pose, len(ins[0])))
    return pose, recs, status, evs, store


def restore(ctx, store):
    """Replaces the context's hashed volume by the union of its resident blocks and the stored ones (`Context.tsdf_upload_blocks`): the
    whole model, for `Context.tsdf_mesh_hashed` or a save.  The store is left as it is.  Returns the number of blocks.  A store of coloured
    blocks puts them back with their colours (the context's volume is then a coloured one)."""
    colored = bool(store.colored)
    _, *res = ctx.tsdf_blocks(colors=True) if colored else ctx.tsdf_blocks()
    sto = store.blocks()
    both = [np.concatenate([a, b]) for a, b in zip(res, sto)]
    cc = both[0]
    order = np.lexsort((cc[:, 0], cc[:, 1], cc[:, 2]))
    ctx.tsdf_upload_blocks(*[a[order] for a in both])
    return len(cc)
