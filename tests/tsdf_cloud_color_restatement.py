"""icp_tsdf_integrate_cloud_color of include/icp_hip.h restated in numpy fp32: the colours of a cloud fused into a
coloured TSDF volume, dense or hashed, with its geometry.  Written from the contract alone, by composition: the geometry is
tsdf_carve_restatement.integrate under the carve options (tsdf_cloud_restatement's with carving off), the rays are
tsdf_cloud_restatement.rays, the hashed colours live where htsdf_color_restatement keeps them (vol.colors); what is stated here is only
what the contract adds -- the UNCARVED colour walk with its band rule, the integer sums of the points' bytes, and the colour fold.  The
sums are Python-side int64, which no order can change.  Contains no table, no atomics and no device code."""
import numpy as np

import htsdf_color_restatement as HC
import tsdf_carve_restatement as CV
import tsdf_cloud_restatement as CR
from tsdf_cloud_restatement import DVolume, f32, f64, i64, VOX_LO, VOX_HI

MAX_POINTS = 1 << 24


def add_color(vol):
    """Colours for a volume: a DVolume gets rgb (nz, ny, nx, 3) and wc (nz, ny, nx), all zero; an HVolume htsdf_color_restatement's dict."""
    if isinstance(vol, DVolume):
        nx, ny, nz = vol.dims
        vol.rgb = np.zeros((nz, ny, nx, 3), f32); vol.wc = np.zeros((nz, ny, nx), f32)
        return vol
    return HC.add_color(vol)


def color_walk(vol, pts, rgba, pose, origin=None):
    """The colour walk of every ray, m = 0 .. M, whatever the carve options are: (voxels (Q, 3) int64, c (Q, 3) int64: the bytes of the
    point behind every colouring sample)."""
    dense = isinstance(vol, DVolume)
    c, u, r, usable = CR.rays(vol, pts, pose, origin)
    cols = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)[:, :3].astype(i64)      # alpha is not read
    n = len(r)
    assert len(cols) == n
    prev = np.zeros((n, 3), i64); have = np.zeros(n, bool)
    ovox, ocol = [], []
    hi = [f32(d - 1) for d in vol.dims] if dense else [VOX_HI] * 3
    lo = [f32(0)] * 3 if dense else [VOX_LO] * 3
    with np.errstate(all="ignore"):
        for m in range(CR.n_steps(vol) + 1):
            t = np.fmin((r - vol.trunc) + f32(m) * vol.s, r + vol.trunc)
            act = usable & (t > 0)
            g = [np.floor(((c[a] + t * u[:, a]) - vol.o[a]) / vol.s + f32(0.5)) for a in range(3)]
            for a in range(3):
                act &= (g[a] >= lo[a]) & (g[a] <= hi[a])
            gi = np.stack([np.where(act, g[a], 0).astype(i64) for a in range(3)], 1)
            dup = have & (gi == prev).all(1)
            prev[act] = gi[act]; have |= act
            act &= ~dup
            x = [vol.o[a] + g[a] * vol.s for a in range(3)]
            e = [x[a] - c[a] for a in range(3)]
            proj = e[0] * u[:, 0] + (e[1] * u[:, 1] + e[2] * u[:, 2])
            sdf = r - proj
            paint = act & ~(sdf < -vol.trunc) & ~(sdf > vol.trunc)
            ovox.append(gi[paint]); ocol.append(cols[paint])
    return (np.concatenate(ovox) if ovox else np.zeros((0, 3), i64)), (np.concatenate(ocol) if ocol else np.zeros((0, 3), i64))


def accumulate(voxels, cols):
    """(unique voxels (V, 3), S (V, 3) int64, NC (V,) int64): the integer accumulators of one scan."""
    if len(voxels) == 0:
        return np.zeros((0, 3), i64), np.zeros((0, 3), i64), np.zeros(0, i64)
    uv, inv = np.unique(voxels, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    S = np.zeros((len(uv), 3), i64); N = np.zeros(len(uv), i64)
    np.add.at(S, inv, cols); np.add.at(N, inv, 1)
    assert N.max() <= MAX_POINTS and S.max() < (1 << 32)
    return uv, S, N


def fold_values(C, Wc, S, N, max_w):
    """C (V, 3), Wc (V,) -> the folded pair."""
    cbar = (S.astype(f64) / N.astype(f64)[:, None]).astype(f32)
    with np.errstate(all="ignore"):
        return ((Wc[:, None] * C + cbar) / (Wc[:, None] + f32(1))).astype(f32), np.fmin(Wc + f32(1), max_w).astype(f32)


def fold(vol, uv, S, N):
    if not len(uv):
        return
    if isinstance(vol, DVolume):
        ix = (uv[:, 2], uv[:, 1], uv[:, 0])
        vol.rgb[ix], vol.wc[ix] = fold_values(vol.rgb[ix], vol.wc[ix], S, N, vol.max_w)
        return
    ub, inv = np.unique(uv >> 3, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for j, b in enumerate(ub):
        b = tuple(int(x) for x in b)
        assert b in vol.blocks, b                      # the touch is exact: a colouring sample's block is resident
        sel = np.nonzero(inv == j)[0]
        loc = uv[sel] & 7
        ix = (loc[:, 2], loc[:, 1], loc[:, 0])
        C, Wc = HC._colors_of(vol, b)
        C[ix], Wc[ix] = fold_values(C[ix], Wc[ix], S[sel], N[sel], vol.max_w)
    vol._cbox = None


def integrate(vol, pts, rgba, pose, origin=None, distance=0.0, min_range=0.0):
    """icp_tsdf_integrate_cloud_color on a coloured HVolume or DVolume under the carve options, in place.  Returns (icp_tsdf_cloud_info
    as a dict, dict(n_steps, n_carved), n_colored).  ValueError where the call is refused for its size."""
    if len(pts) > MAX_POINTS:
        raise ValueError("more than 2^24 points")
    info, stats = CV.integrate(vol, pts, pose, origin, distance, min_range)      # (allocates the touch's blocks)
    uv, S, N = accumulate(*color_walk(vol, pts, rgba, pose, origin))
    fold(vol, uv, S, N)
    return info, stats, len(uv)


def colors_of(vol):
    """The volume's colours as the device returns them: dense (rgb, wc); hashed htsdf_color_restatement.sorted_colors."""
    return (vol.rgb, vol.wc) if isinstance(vol, DVolume) else HC.sorted_colors(vol)


def track(vol, scans, colors, pose0, distance=0.0, min_range=0.0, **kw):
    """icp_track_scans_sdf_color: tsdf_carve_restatement.track with every fuse the coloured one.  Returns (poses, records, infos, status,
    n_colored of every scan -- 0 for a skipped one)."""
    import sdf_cloud_restatement as SC
    pose = np.asarray(pose0, f32).copy()
    info, _, nc = integrate(vol, scans[0], colors[0], pose, None, distance, min_range)
    poses, recs, infos, ncs, status = [pose.copy()], [], [info], [nc], SC.OK
    for k in range(1, len(scans)):
        pose, rec, _ = SC.align(vol, scans[k], pose, **kw)
        if rec["status"] == SC.OK:
            info, _, nc = integrate(vol, scans[k], colors[k], pose, None, distance, min_range)
            infos.append(info); ncs.append(nc)
        else:
            infos.append(dict(SC.ZERO_INFO)); ncs.append(0)
            if status == SC.OK:
                status = rec["status"]
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs, infos, status, ncs
