"""Free-space carving of the cloud fuses (icp_set_tsdf_carve_options of include/icp_hip.h) restated in numpy fp32:
tsdf_cloud_restatement's walk started J steps in front of the band, m = -J .. M, literally as the contract writes it -- every sample of
every ray is visited, nothing is jumped over, and an m < 0 sample is applied only where the voxel has storage (dense: in the box; hashed:
its block resident after this call's touch).  Written from the contract alone; every fp32 operation is one numpy float32 operation in the
order the contract writes it, so the device is compared bit for bit.  With distance 0 it is tsdf_cloud_restatement.integrate."""
import math
import numpy as np

import tsdf_cloud_restatement as CR
from tsdf_cloud_restatement import DVolume, f32, f64, i64, SCALE, VOX_LO, VOX_HI

MAX_STEPS = 65536
STATS = ("n_steps", "n_carved")


def carve_steps(vol, distance):
    """J = ceil(min(distance, max_depth) / s) in double, of the fp32 option; 0 = off.  ValueError beyond the cap (the call is refused)."""
    d = float(f32(distance))
    if not d > 0.0:
        return 0
    j = math.ceil(min(d, float(vol.max_d)) / float(vol.s))
    if not j <= MAX_STEPS:
        raise ValueError("carving would walk more than %d steps per ray" % MAX_STEPS)
    return int(j)


def walk(vol, pts, pose, origin=None, distance=0.0, min_range=0.0):
    """The walk of every ray, m = -J .. M: dict(n_points, n_rays, n_samples, n_outside: of the m >= 0 samples; touched (B, 3) int64: the
    blocks the hashed touch asks for; rays (Q,), m (Q,), voxels (Q, 3) int64, k (Q,) int64: every observation that passed the sdf test,
    in walk order per step, whether or not the voxel has storage; n_steps: J)."""
    dense = isinstance(vol, DVolume)
    J = carve_steps(vol, distance); mr = f32(min_range)
    c, u, r, usable = CR.rays(vol, pts, pose, origin)
    n = len(r)
    prev = np.zeros((n, 3), i64); have = np.zeros(n, bool)
    orays, om, ovox, ok_, touched = [], [], [], [], []
    n_samples = n_outside = 0
    hi = [f32(d - 1) for d in vol.dims] if dense else [VOX_HI] * 3
    lo = [f32(0)] * 3 if dense else [VOX_LO] * 3
    with np.errstate(all="ignore"):
        for m in range(-J, CR.n_steps(vol) + 1):
            t = np.fmin((r - vol.trunc) + f32(m) * vol.s, r + vol.trunc)
            ia = np.nonzero(usable & ((t > 0) if m >= 0 else (t > mr)))[0]      # the rays that have this sample; everything below is theirs alone
            if not len(ia):
                continue
            t, ua, ra = t[ia], u[ia], r[ia]
            g = [np.floor(((c[a] + t * ua[:, a]) - vol.o[a]) / vol.s + f32(0.5)) for a in range(3)]
            inr = np.ones(len(ia), bool)
            for a in range(3):
                inr &= (g[a] >= lo[a]) & (g[a] <= hi[a])
            if m >= 0:
                n_outside += int((~inr).sum())
            gi = np.stack([np.where(inr, g[a], 0).astype(i64) for a in range(3)], 1)
            if m >= 0:
                touched.append(gi[inr] >> 3)
            act = inr & ~(have[ia] & (gi == prev[ia]).all(1))
            prev[ia[inr]] = gi[inr]; have[ia[inr]] = True
            if m >= 0:
                n_samples += int(act.sum())
            x = [vol.o[a] + g[a] * vol.s for a in range(3)]
            e = [x[a] - c[a] for a in range(3)]
            proj = e[0] * ua[:, 0] + (e[1] * ua[:, 1] + e[2] * ua[:, 2])
            sdf = ra - proj
            obs = act & ~(sdf < -vol.trunc)
            f = np.fmin(f32(1), sdf / vol.trunc)
            k = np.rint(f * SCALE)
            orays.append(ia[obs]); om.append(np.full(int(obs.sum()), m, i64)); ovox.append(gi[obs]); ok_.append(k[obs].astype(i64))
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, i64)
    tb = cat(touched, (0, 3))
    return dict(n_points=n, n_rays=int(usable.sum()), n_samples=n_samples, n_outside=n_outside, n_steps=J,
                touched=np.unique(tb, axis=0) if len(tb) else tb, rays=cat(orays, (0,)), m=cat(om, (0,)), voxels=cat(ovox, (0, 3)), k=cat(ok_, (0,)))


def stored(vol, w):
    """Which of the walk's observations are applied: all of the band's; of the carve samples those whose voxel has storage -- in a dense
    volume every in-range voxel, in a hashed one a voxel whose block is resident after the touch."""
    keep = np.ones(len(w["m"]), bool)
    if isinstance(vol, DVolume) or not len(keep):
        return keep
    resident = set(vol.blocks) | set(map(tuple, w["touched"].tolist()))
    ub, inv = np.unique(w["voxels"] >> 3, axis=0, return_inverse=True)
    has = np.array([tuple(int(x) for x in b) in resident for b in ub], bool)
    return (w["m"] >= 0) | has[inv.reshape(-1)]


def fold(vol, uv, S, N):
    """tsdf_cloud_restatement.integrate's fold of the accumulators into the volume, dense or hashed (every block resident)."""
    if not len(uv):
        return
    if isinstance(vol, DVolume):
        ix = (uv[:, 2], uv[:, 1], uv[:, 0])
        vol.tsdf[ix], vol.weight[ix] = CR.fold_values(vol.tsdf[ix], vol.weight[ix], S, N, vol.max_w)
        return
    ub, inv = np.unique(uv >> 3, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for j, b in enumerate(ub):
        sel = np.nonzero(inv == j)[0]
        loc = uv[sel] & 7
        ix = (loc[:, 2], loc[:, 1], loc[:, 0])
        D, W = vol.blocks[tuple(int(x) for x in b)]
        D[ix], W[ix] = CR.fold_values(D[ix], W[ix], S[sel], N[sel], vol.max_w)
    vol._box = None


def accumulate(vol, w):
    """(unique voxels (V, 3), S, N, n_carved) of the applied observations."""
    keep = stored(vol, w)
    uv, S, N = CR.accumulate(w["voxels"][keep], w["k"][keep])
    return uv, S, N, int((keep & (w["m"] < 0)).sum())


def integrate(vol, pts, pose, origin=None, distance=0.0, min_range=0.0):
    """icp_tsdf_integrate_cloud under the carve options, on an HVolume or a DVolume, in place.  Returns (icp_tsdf_cloud_info as a dict,
    dict(n_steps, n_carved))."""
    w = walk(vol, pts, pose, origin, distance, min_range)
    uv, S, N, n_carved = accumulate(vol, w)
    n_blocks = 0
    if not isinstance(vol, DVolume):
        if len(w["touched"]):
            vol.allocate(w["touched"])
        vol.n_out_of_range += w["n_outside"]
        n_blocks = len(vol.blocks)
    fold(vol, uv, S, N)
    info = dict(n_points=w["n_points"], n_rays=w["n_rays"], n_updated=len(uv), n_blocks=n_blocks, n_samples=w["n_samples"], n_outside=w["n_outside"])
    return info, dict(n_steps=w["n_steps"], n_carved=n_carved)


def track(vol, scans, pose0, distance=0.0, min_range=0.0, **kw):
    """icp_track_scans_sdf with the carve options: sdf_cloud_restatement.track with every fuse carving.  Returns (poses, records, infos,
    status, the carve stats of every scan -- None for a skipped one)."""
    import sdf_cloud_restatement as SC
    pose = np.asarray(pose0, f32).copy()
    info, st = integrate(vol, scans[0], pose, None, distance, min_range)
    poses, recs, infos, stats, status = [pose.copy()], [], [info], [st], SC.OK
    for k in range(1, len(scans)):
        pose, rec, _ = SC.align(vol, scans[k], pose, **kw)
        if rec["status"] == SC.OK:
            info, st = integrate(vol, scans[k], pose, None, distance, min_range)
            infos.append(info); stats.append(st)
        else:
            infos.append(dict(SC.ZERO_INFO)); stats.append(None)
            if status == SC.OK:
                status = rec["status"]
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs, infos, status, stats
