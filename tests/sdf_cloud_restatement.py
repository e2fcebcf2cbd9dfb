"""The contract of a laser scan aligned to the TSDF volume (include/icp_hip.h: icp_tsdf_cloud_system, icp_tsdf_align_cloud,
icp_track_scans_sdf) restated in numpy.  Written from the contract alone: every fp32 operation is one numpy
float32 operation in the order the contract writes it, everything after the conversion to fp64 is numpy float64.  `system` returns, next
to every sum, the sum of the absolute values of its terms, which bounds what another summation order may change.  The cell, the field and
the gradient are sdf_restatement's (a dense Volume below, or htsdf_restatement.HVolume), Jacobian, solve, step, stop and composition are
sdf_restatement's, the fuse inside `track` is tsdf_cloud_restatement.integrate.  Contains no device code."""
import numpy as np

import htsdf_restatement as HR      # (also makes sdf_restatement read either storage)
import sdf_restatement as SR
import tsdf_cloud_restatement as CR

f32, f64 = np.float32, np.float64
OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = SR.OK, SR.ERR_NO_SOURCE, SR.ERR_NO_CORRESPONDENCES
HVolume = HR.HVolume


class Volume(CR.DVolume):
    """The dense volume both restatements read: tsdf_cloud_restatement's arrays under the names tsdf_restatement's cell uses."""

    def __init__(self, dims, origin, **kw):
        super().__init__(dims, origin, **kw)
        self.nx, self.ny, self.nz = self.dims


def options(**kw):
    o = SR.options(**kw)
    if o["stride"] != 1:
        raise ValueError("stride must be 1")
    return o


def point_terms(vol, pts, pose):
    """Every point of the cloud at `pose` (4x4 scan frame -> world, fp32): dict of considered (n,), valid (n,), q (n, 3) fp32, F (n,) fp32,
    r (n,) and g (n, 3) fp64 (metres, per metre)."""
    P = np.asarray(pose, f32)
    p = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    with np.errstate(all="ignore"):
        considered = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        q = [(P[r, 0] * x + (P[r, 1] * y + P[r, 2] * z)) + P[r, 3] for r in range(3)]
        cell, F, gx, gy, gz = SR._field_and_gradient(vol, q[0], q[1], q[2])
        valid = considered & cell & (np.abs(F) < f32(1))
        r = F.astype(f64) * f64(vol.trunc)
        scale = f64(vol.trunc) / f64(vol.s)
        g = np.stack([gx.astype(f64) * scale, gy.astype(f64) * scale, gz.astype(f64) * scale], 1)
    return dict(considered=considered, valid=valid, q=np.stack(q, 1).astype(f32), F=F, r=r, g=g)


def terms_of(t, huber=0.0):
    """The 28 terms of every valid point: (28, n_valid) fp64."""
    m = t["valid"]
    r = t["r"][m]; J = SR.jacobian(t["q"][m], t["g"][m])
    w = np.ones(len(r), f64)
    if f32(huber) > 0:
        h = f64(f32(huber)); ar = np.abs(r)
        with np.errstate(all="ignore"):
            w = np.where(ar <= h, 1.0, h / ar)
    wJ = w[:, None] * J
    terms = np.empty((28, len(r)), f64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            terms[k] = wJ[:, i] * J[:, j]; k += 1
    for i in range(6):
        terms[21 + i] = -(wJ[:, i] * r)
    terms[27] = (w * r) * r
    return terms


def system(vol, pts, pose, huber=0.0, **_):
    """icp_tsdf_cloud_system: ((n_depth, n_valid), sums (28,) fp64, sum of |term| per sum (28,))."""
    t = point_terms(vol, pts, pose)
    terms = terms_of(t, huber)
    return (int(t["considered"].sum()), int(t["valid"].sum())), terms.sum(1), np.abs(terms).sum(1)


def align(vol, pts, pose, **kw):
    """icp_tsdf_align_cloud: (pose, record, trace).  A failed alignment carries the pose it started with."""
    o = options(**kw)
    start = np.asarray(pose, f32).copy(); cur = start.copy()
    rec = dict(n_depth=0, n_valid_first=0, n_valid_last=0, iterations=0, status=OK, cost_first=0.0, cost_last=0.0)
    trace = []
    for it in range(o["n_iterations"]):
        counts, sums, _ = system(vol, pts, cur, **o)
        if it == 0:
            rec.update(n_depth=counts[0], n_valid_first=counts[1], cost_first=float(sums[27]))
        rec.update(n_valid_last=counts[1], cost_last=float(sums[27]), iterations=it + 1)
        new, x = (None, None) if counts[0] == 0 else SR.step(sums, counts, cur, **o)
        if new is None:
            rec["status"] = ERR_NO_SOURCE if counts[0] == 0 else ERR_NO_CORRESPONDENCES
            trace.append(dict(n_valid=counts[1], status=rec["status"], cost=float(sums[27]), pose=cur.copy()))
            cur = start.copy()
            break
        cur = new
        trace.append(dict(n_valid=counts[1], status=OK, cost=float(sums[27]), pose=cur.copy()))
        if SR.stopped(x, **o):
            break
    rec["pose"] = cur.copy()
    return cur, rec, trace


ZERO_INFO = dict.fromkeys(CR.INFO, 0)


def track(vol, scans, pose0, **kw):
    """icp_track_scans_sdf: scan 0 fused at pose0; scan k aligned to the volume built so far and, on success, fused at the pose found; a
    scan that fails is skipped and carries the pose.  Returns (poses: one per scan, records of scans 1 .., infos: one per scan, a
    skipped scan's all zero, status: the first per-scan error, or 0)."""
    pose = np.asarray(pose0, f32).copy()
    poses, recs, infos, status = [pose.copy()], [], [CR.integrate(vol, scans[0], pose)], OK
    for k in range(1, len(scans)):
        pose, rec, _ = align(vol, scans[k], pose, **kw)
        if rec["status"] == OK:
            infos.append(CR.integrate(vol, scans[k], pose))
        else:
            infos.append(dict(ZERO_INFO))
            if status == OK:
                status = rec["status"]
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs, infos, status
