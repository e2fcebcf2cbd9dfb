"""icp_tsdf_integrate_cloud of include/icp_hip.h restated in numpy fp32: a cloud's rays walked through the truncation
band, every sample's nearest voxel observed into integer accumulators, the fold into (tsdf, weight), and the hashed volume's touch.  Written
from the contract alone; every fp32 operation is one numpy float32 operation in the order the contract writes it, so the device is
compared bit for bit.  The hashed storage is htsdf_restatement.HVolume (blocks in a dict), the dense one the plain arrays of DVolume.
Contains no table, no atomics and no device code: the accumulators are Python-side int64 sums, which no order can change."""
import math
import numpy as np

import htsdf_restatement as HR

f32, f64, i64 = np.float32, np.float64, np.int64
SCALE = f32(32768.0)
VOX_LO, VOX_HI = f32(-(1 << 23)), f32((1 << 23) - 1)      # voxels whose block is storable
INFO = ("n_points", "n_rays", "n_updated", "n_blocks", "n_samples", "n_outside")


class DVolume:
    """The dense volume: tsdf and weight (nz, ny, nx) float32, voxel (0, 0, 0) centred on `origin`."""

    def __init__(self, dims, origin, voxel_size=0.05, truncation=0.25, max_weight=64.0, min_depth=0.3, max_depth=8.0, **_):
        self.dims = tuple(int(d) for d in dims)
        self.o = np.asarray(origin, f32)
        self.s, self.trunc, self.max_w, self.max_d = f32(voxel_size), f32(truncation), f32(max_weight), f32(max_depth)
        nx, ny, nz = self.dims
        self.tsdf = np.zeros((nz, ny, nx), f32); self.weight = np.zeros((nz, ny, nx), f32)


def n_steps(vol):
    """M = ceil(2 truncation / s), in double."""
    return int(math.ceil(2.0 * float(vol.trunc) / float(vol.s)))


def sensor_centre(pose, origin=None):
    P = np.asarray(pose, f32); e = np.zeros(3, f32) if origin is None else np.asarray(origin, f32)
    return np.array([(P[r, 0] * e[0] + (P[r, 1] * e[1] + P[r, 2] * e[2])) + P[r, 3] for r in range(3)], f32)


def rays(vol, pts, pose, origin=None):
    """(c (3,), u (n, 3), r (n,), usable (n,)) of the cloud's points."""
    P = np.asarray(pose, f32); p = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    c = sensor_centre(pose, origin)
    with np.errstate(all="ignore"):
        fin = np.isfinite(p).all(1)
        d = [((P[r, 0] * p[:, 0] + (P[r, 1] * p[:, 1] + P[r, 2] * p[:, 2])) + P[r, 3]) - c[r] for r in range(3)]
        r2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])
        r = np.sqrt(r2)
        usable = fin & np.isfinite(r) & (r > 0) & (r <= vol.max_d)
        u = np.stack([d[a] / r for a in range(3)], 1)
    return c, u.astype(f32), r.astype(f32), usable


def walk(vol, pts, pose, origin=None):
    """The walk of every ray: dict(n_points, n_rays, n_samples, n_outside, sampled (K, 3) int64: the voxel of every counted sample,
    voxels (J, 3) int64 and k (J,) int64: the observations)."""
    dense = isinstance(vol, DVolume)
    c, u, r, usable = rays(vol, pts, pose, origin)
    n = len(r)
    prev = np.zeros((n, 3), i64); have = np.zeros(n, bool)
    sampled, ovox, ok_ = [], [], []
    n_samples = n_outside = 0
    hi = [f32(d - 1) for d in vol.dims] if dense else [VOX_HI] * 3
    lo = [f32(0)] * 3 if dense else [VOX_LO] * 3
    with np.errstate(all="ignore"):
        for m in range(n_steps(vol) + 1):
            t = np.fmin((r - vol.trunc) + f32(m) * vol.s, r + vol.trunc)
            act = usable & (t > 0)
            g = [np.floor(((c[a] + t * u[:, a]) - vol.o[a]) / vol.s + f32(0.5)) for a in range(3)]
            inr = np.ones(n, bool)
            for a in range(3):
                inr &= (g[a] >= lo[a]) & (g[a] <= hi[a])
            n_outside += int((act & ~inr).sum())
            act &= inr
            gi = np.stack([np.where(act, g[a], 0).astype(i64) for a in range(3)], 1)
            dup = have & (gi == prev).all(1)
            prev[act] = gi[act]; have |= act
            act &= ~dup
            n_samples += int(act.sum())
            sampled.append(gi[act])
            gf = [g[a] for a in range(3)]
            x = [vol.o[a] + gf[a] * vol.s for a in range(3)]
            e = [x[a] - c[a] for a in range(3)]
            proj = e[0] * u[:, 0] + (e[1] * u[:, 1] + e[2] * u[:, 2])
            sdf = r - proj
            obs = act & ~(sdf < -vol.trunc)
            f = np.fmin(f32(1), sdf / vol.trunc)
            k = np.rint(f * SCALE)
            ovox.append(gi[obs]); ok_.append(k[obs].astype(i64))
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, i64)
    return dict(n_points=n, n_rays=int(usable.sum()), n_samples=n_samples, n_outside=n_outside, sampled=cat(sampled, (0, 3)), voxels=cat(ovox, (0, 3)),
                k=cat(ok_, (0,)))


def accumulate(voxels, k):
    """(unique voxels (V, 3), S (V,) int64, N (V,) int64): the integer accumulators of one scan."""
    if len(voxels) == 0:
        return np.zeros((0, 3), i64), np.zeros(0, i64), np.zeros(0, i64)
    uv, inv = np.unique(voxels, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    S = np.zeros(len(uv), i64); N = np.zeros(len(uv), i64)
    np.add.at(S, inv, k); np.add.at(N, inv, 1)
    return uv, S, N


def fold_values(D, W, S, N, max_w):
    fbar = (S.astype(f64) / (N.astype(f64) * 32768.0)).astype(f32)
    with np.errstate(all="ignore"):
        return ((W * D + fbar) / (W + f32(1))).astype(f32), np.fmin(W + f32(1), max_w).astype(f32)


def touch(vol, pts, pose, origin=None):
    """The blocks the hashed touch asks for: a set of block coordinates.  Allocates nothing."""
    w = walk(vol, pts, pose, origin)
    return set(map(tuple, np.unique(w["sampled"] >> 3, axis=0).tolist())) if len(w["sampled"]) else set()


def integrate(vol, pts, pose, origin=None):
    """icp_tsdf_integrate_cloud on an HVolume or a DVolume, in place.  Returns icp_tsdf_cloud_info as a dict."""
    w = walk(vol, pts, pose, origin)
    uv, S, N = accumulate(w["voxels"], w["k"])
    if isinstance(vol, DVolume):
        if len(uv):
            ix = (uv[:, 2], uv[:, 1], uv[:, 0])
            vol.tsdf[ix], vol.weight[ix] = fold_values(vol.tsdf[ix], vol.weight[ix], S, N, vol.max_w)
        n_blocks = 0
    else:
        if len(w["sampled"]):
            vol.allocate(np.unique(w["sampled"] >> 3, axis=0))
        vol.n_out_of_range += w["n_outside"]
        if len(uv):
            ub, inv = np.unique(uv >> 3, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            order = np.argsort(inv, kind="stable")
            ends = np.cumsum(np.bincount(inv, minlength=len(ub)))
            for j, b in enumerate(ub):
                sel = order[(ends[j - 1] if j else 0):ends[j]]
                loc = uv[sel] & 7
                ix = (loc[:, 2], loc[:, 1], loc[:, 0])
                D, W = vol.blocks[tuple(int(x) for x in b)]
                D[ix], W[ix] = fold_values(D[ix], W[ix], S[sel], N[sel], vol.max_w)
            vol._box = None
        n_blocks = len(vol.blocks)
    return dict(n_points=w["n_points"], n_rays=w["n_rays"], n_updated=len(uv), n_blocks=n_blocks, n_samples=w["n_samples"], n_outside=w["n_outside"])
