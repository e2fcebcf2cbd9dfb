"""The ray-cast of the hashed TSDF volume (include/icp_hip.h) restated in numpy fp32.  Written from the contract
alone: the march, the per-sample arithmetic, the end rule, zh and the normal of icp_tsdf_raycast, with the cell read through the hashed
volume's addressing -- a voxel is a signed global coordinate, it lies in block g >> 3, and a voxel of a block that does not exist reads
(0, 0).  Every fp32 operation is one numpy float32 operation in the order the contract writes it, so the device is compared bit for bit.
Contains no table, no box and no device code.

`trace` (a dict, optional) receives what the tests assert about their own cases: every evaluated sample classified by the number of
distinct blocks its cell touches and by validity, the samples out of the storable range, and the events of the end rule."""
import numpy as np

f32 = np.float32
MINF = f32(-np.inf)
RANGE = 1 << 20
CELL_LO, CELL_HI = f32(-(1 << 23)), f32((1 << 23) - 2)


class Blocks:
    """The hashed volume as the contract sees it: blocks (B, 3) int with tsdf and weight (B, 8, 8, 8) indexed [z, y, x], in any order."""

    def __init__(self, coords, tsdf, weight, origin, voxel_size=0.05, truncation=0.25, min_depth=0.3, max_depth=8.0, ray_step=0.0, **_):
        c = np.asarray(coords, np.int64).reshape(-1, 3)
        key = ((c[:, 2] + RANGE) << 42) | ((c[:, 1] + RANGE) << 21) | (c[:, 0] + RANGE)
        order = np.argsort(key)
        self.key = key[order]
        assert len(np.unique(self.key)) == len(self.key)
        self.F = np.asarray(tsdf, f32).reshape(-1, 512)[order]
        self.W = np.asarray(weight, f32).reshape(-1, 512)[order]
        self.o = np.asarray(origin, f32)
        self.s, self.trunc = f32(voxel_size), f32(truncation)
        self.min_d, self.max_d = f32(min_depth), f32(max_depth)
        self.step = f32(self.trunc / f32(2)) if f32(ray_step) == 0 else f32(ray_step)

    def voxel(self, gx, gy, gz):
        """(F, W, block exists) of the voxels at signed global coordinates (int64 arrays)."""
        bx, by, bz = gx >> 3, gy >> 3, gz >> 3
        key = ((bz + RANGE) << 42) | ((by + RANGE) << 21) | (bx + RANGE)
        if len(self.key) == 0:
            z = np.zeros(len(gx), f32)
            return z, z.copy(), np.zeros(len(gx), bool)
        at = np.minimum(np.searchsorted(self.key, key), len(self.key) - 1)
        there = self.key[at] == key
        loc = (gz & 7) * 64 + (gy & 7) * 8 + (gx & 7)
        return np.where(there, self.F[at, loc], f32(0)), np.where(there, self.W[at, loc], f32(0)), there


def _lerp(a, b, t):
    return a + t * (b - a)


def cell(vol, qx, qy, qz):
    """The cell of world points q: (valid, corners c[dx + 2 dy + 4 dz] (8, n), tx, ty, tz, in range (n,), distinct blocks touched (n,),
    corners whose block is missing (n,), the block of the lowest corner (n, 3), whether that block exists (n,))."""
    n = len(qx)
    with np.errstate(all="ignore"):
        g = [(q - vol.o[a]) / vol.s for a, q in enumerate((qx, qy, qz))]
        fl = [np.floor(x) for x in g]
        ok = np.ones(n, bool)
        for a in range(3):
            ok &= (fl[a] >= CELL_LO) & (fl[a] <= CELL_HI)                 # in float, before any cast
        t = [g[a] - fl[a] for a in range(3)]
        i = [np.where(ok, fl[a], 0).astype(np.int64) for a in range(3)]
    c = np.zeros((8, n), f32)
    valid = ok.copy()
    missing = np.zeros(n, np.int64)
    base = None
    for k in range(8):
        F, W, there = vol.voxel(i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + (k >> 2))
        c[k] = F
        valid &= W > 0
        missing += ~there
        base = there if k == 0 else base
    crossing = [(i[a] & 7) == 7 for a in range(3)]
    touched = (1 << (crossing[0].astype(np.int64) + crossing[1] + crossing[2]))
    return valid, c, t[0], t[1], t[2], ok, touched, missing, np.stack([x >> 3 for x in i], 1), base


def raycast(vol, cam, pose, trace=None):
    """The hashed volume seen from pose (4x4 camera -> world).  Returns (depth (h, w), vertices (w*h, 3), normals (w*h, 3), hits)."""
    P = np.asarray(pose, f32)
    n = cam.width * cam.height
    uu, vv = np.meshgrid(np.arange(cam.width, dtype=f32), np.arange(cam.height, dtype=f32))
    a = ((uu.reshape(-1) - cam.cx) / cam.fx).astype(f32); b = ((vv.reshape(-1) - cam.cy) / cam.fy).astype(f32)
    dw = [P[r, 0] * a + (P[r, 1] * b + P[r, 2] * f32(1)) for r in range(3)]
    alive = np.ones(n, bool); prev_valid = np.zeros(n, bool); ended = np.zeros(n, bool)
    f_prev = np.zeros(n, f32); z_prev = np.zeros(n, f32); f_end = np.zeros(n, f32)
    seen_valid = np.zeros(n, bool)
    last = np.full((n, 3), -(1 << 31), np.int64)                    # the per-lane cache of the kernel, modelled for the trace alone
    if trace is not None:
        trace.update(classes={(t, v): 0 for t in (1, 2, 4, 8) for v in (True, False)}, one_missing={True: 0, False: 0}, out_of_range=0, samples=0,
                     nan_passed=0, first_valid_nonpositive=0, crossing_behind_invalid=0, no_block=0, base_missing=0, cached=0, probes=0)
    k = 0
    with np.errstate(all="ignore"):
        while alive.any():
            z = f32(vol.min_d + f32(k) * vol.step)
            if not (z <= vol.max_d):
                break
            idx = np.nonzero(alive)[0]
            valid, c, tx, ty, tz, inr, touched, missing, blk, base = cell(vol, *[P[r, 3] + z * dw[r][idx] for r in range(3)])
            e0 = _lerp(_lerp(c[0], c[1], tx), _lerp(c[2], c[3], tx), ty)
            e1 = _lerp(_lerp(c[4], c[5], tx), _lerp(c[6], c[7], tx), ty)
            F = _lerp(e0, e1, tz)
            end = valid & (F <= 0)
            if trace is not None:
                trace["samples"] += len(idx); trace["out_of_range"] += int((~inr).sum())
                trace["no_block"] += int((inr & (missing == 8)).sum())
                # the kernel's savings, none of which changes a result: the lowest corner's block is looked up first, through a one-entry
                # cache per ray; the other touched - 1 blocks only when it exists (at most: a missing neighbour ends the lookups early)
                same = inr & (blk == last[idx]).all(1)
                trace["cached"] += int(same.sum()); trace["base_missing"] += int((inr & ~base).sum())
                trace["probes"] += int((inr & ~same).sum()) + int(((touched - 1) * (inr & base)).sum())
                last[idx[inr]] = blk[inr]
                for t in (1, 2, 4, 8):
                    for v in (True, False):
                        trace["classes"][(t, v)] += int((inr & (touched == t) & (valid == v)).sum())
                one = inr & (missing == 1)                     # exactly one corner's block missing: a cell on a corner of the block grid, 7 of its 8 blocks there
                trace["one_missing"][False] += int((one & ~valid).sum())
                trace["one_missing"][True] += int((one & valid).sum())      # (stays 0: that corner reads W = 0)
                trace["nan_passed"] += int((valid & np.isnan(F)).sum())
                trace["first_valid_nonpositive"] += int((end & ~seen_valid[idx]).sum())
                trace["crossing_behind_invalid"] += int((end & seen_valid[idx] & ~prev_valid[idx]).sum())
            seen_valid[idx] |= valid
            ended[idx[end]] = True; f_end[idx[end]] = F[end]; alive[idx[end]] = False
            go = ~end
            prev_valid[idx[go]] = valid[go]
            upd = go & valid
            f_prev[idx[upd]] = F[upd]; z_prev[idx[upd]] = z
            k += 1
        cand = np.nonzero(ended & prev_valid & (f_prev > 0))[0]
        depth = np.full(n, MINF, f32); vert = np.full((n, 3), MINF, f32); nrm = np.full((n, 3), MINF, f32)
        fp, fe = f_prev[cand], f_end[cand]
        zh = z_prev[cand] + vol.step * (fp / (fp - fe))
        valid, c, tx, ty, tz = cell(vol, *[P[r, 3] + zh * dw[r][cand] for r in range(3)])[:5]
        gx = _lerp(_lerp(c[1] - c[0], c[3] - c[2], ty), _lerp(c[5] - c[4], c[7] - c[6], ty), tz)
        gy = _lerp(_lerp(c[2] - c[0], c[3] - c[1], tx), _lerp(c[6] - c[4], c[7] - c[5], tx), tz)
        gz = _lerp(_lerp(c[4] - c[0], c[5] - c[1], tx), _lerp(c[6] - c[2], c[7] - c[3], tx), ty)
        nc = [-(P[0, r] * gx + (P[1, r] * gy + P[2, r] * gz)) for r in range(3)]
        sq = nc[0] * nc[0] + (nc[1] * nc[1] + nc[2] * nc[2])
        ln = np.sqrt(sq)
        m = [x / ln for x in nc]
        hit = valid & np.isfinite(m[0]) & np.isfinite(m[1]) & np.isfinite(m[2])
        h = cand[hit]
        depth[h] = zh[hit]
        vert[h, 0] = a[h] * zh[hit]; vert[h, 1] = b[h] * zh[hit]; vert[h, 2] = zh[hit]
        for r in range(3):
            nrm[h, r] = m[r][hit]
    if trace is not None:
        trace["hits"] = int(len(h)); trace["ended_without_hit"] = int(ended.sum()) - int(len(h))
    return depth.reshape(cam.height, cam.width), vert, nrm, int(len(h))
