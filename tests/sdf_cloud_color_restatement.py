"""The contract of a coloured laser scan aligned to the coloured TSDF volume with a photometric term (include/icp_hip.h:
icp_tsdf_cloud_system_color, icp_tsdf_align_cloud_color, icp_track_scans_sdf_photometric) restated in numpy.
Written from the contract alone, by composition: the geometric row of a point is sdf_cloud_restatement.point_terms', the intensity field,
the rows and the Huber weight are sdf_color_restatement's (on a hashed volume through htsdf_color_restatement's intensity view), step and
stop are sdf_restatement's, the fuse inside `track` is tsdf_cloud_color_restatement.integrate.  What is stated here is only what the
contract adds: the point's own colour word in place of the pixel's, and the moved point in place of the back-projected pixel.  `system`
returns, next to every sum, the sum of the absolute values of its terms (a coloured point's term is geometric + photometric, one number),
which bounds what another summation order may change.  Contains no device code."""
import numpy as np

import htsdf_color_restatement as HC      # (also makes sdf_color_restatement._intensity_field read either storage)
import sdf_cloud_restatement as SC
import sdf_color_restatement as PC
import sdf_restatement as SR
import tsdf_cloud_color_restatement as CC

f32, f64 = np.float32, np.float64
OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = SR.OK, SR.ERR_NO_SOURCE, SR.ERR_NO_CORRESPONDENCES


def point_terms(vol, pts, rgba, pose):
    """sdf_cloud_restatement.point_terms (considered, valid, q, F, r, g) with, per point: colored (n,), r_c (n,) and h (n, 3) in fp64, S."""
    t = SC.point_terms(vol, pts, pose)
    q = t["q"]
    _, all8, S, hx, hy, hz = PC._intensity_field(vol, q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())
    px = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4).astype(np.int64)
    assert len(px) == len(q)
    with np.errstate(all="ignore"):
        Ip = (px[:, 0] + px[:, 1] + px[:, 2]).astype(f64) / f64(765.0)      # the fourth byte is not read
        rc = S.astype(f64) / f64(765.0) - Ip
        den = f64(765.0) * f64(vol.s)
        h = np.stack([hx.astype(f64) / den, hy.astype(f64) / den, hz.astype(f64) / den], 1)
    t.update(colored=t["valid"] & all8 & np.isfinite(S), r_c=rc, h=h, S=S)
    return t


def terms_of(t, huber=0.0, weight=0.1, color_huber=0.0):
    """The 29 terms of every valid point: (29, n_valid) fp64; a coloured point's are geometric + photometric, entry 28 photometric alone."""
    m = t["valid"]
    with np.errstate(all="ignore"):
        r = t["r"][m]
        geo = PC._rows(PC._huber(r, huber), SR.jacobian(t["q"][m], t["g"][m]), r)
        c = t["colored"][m]
        rc = t["r_c"][m][c]
        wc = (f64(f32(weight)) * f64(f32(weight))) * PC._huber(rc, color_huber)
        pho = PC._rows(wc, SR.jacobian(t["q"][m][c], t["h"][m][c]), rc)
        terms = np.zeros((29, len(r)), f64)
        terms[:28] = geo
        terms[:28, c] = geo[:, c] + pho
        terms[28, c] = pho[27]
    return terms


def system(vol, pts, rgba, pose, huber=0.0, weight=0.1, color_huber=0.0, **_):
    """icp_tsdf_cloud_system_color: ((n_depth, n_valid, n_color), sums (29,) fp64, sum of |term| per sum (29,))."""
    t = point_terms(vol, pts, rgba, pose)
    terms = terms_of(t, huber, weight, color_huber)
    return (int(t["considered"].sum()), int(t["valid"].sum()), int(t["colored"].sum())), terms.sum(1), np.abs(terms).sum(1)


def align(vol, pts, rgba, pose, weight=0.1, color_huber=0.0, **kw):
    """icp_tsdf_align_cloud_color: (pose, record, trace); sdf_cloud_restatement.align's loop on the 29 sums with the colour records."""
    o = SC.options(**kw)
    start = np.asarray(pose, f32).copy(); cur = start.copy()
    rec = dict(n_depth=0, n_valid_first=0, n_valid_last=0, n_color_first=0, n_color_last=0, iterations=0, status=OK, cost_first=0.0, cost_last=0.0,
               cost_color_first=0.0, cost_color_last=0.0)
    trace = []
    for it in range(o["n_iterations"]):
        counts, sums, _ = system(vol, pts, rgba, cur, weight=weight, color_huber=color_huber, **o)
        if it == 0:
            rec.update(n_depth=counts[0], n_valid_first=counts[1], n_color_first=counts[2], cost_first=float(sums[27]), cost_color_first=float(sums[28]))
        rec.update(n_valid_last=counts[1], n_color_last=counts[2], cost_last=float(sums[27]), cost_color_last=float(sums[28]), iterations=it + 1)
        new, x = (None, None) if counts[0] == 0 else SR.step(sums, counts, cur, **o)
        row = dict(n_valid=counts[1], n_color=counts[2], cost=float(sums[27]), cost_color=float(sums[28]))
        if new is None:
            rec["status"] = ERR_NO_SOURCE if counts[0] == 0 else ERR_NO_CORRESPONDENCES
            trace.append(dict(row, status=rec["status"], pose=cur.copy()))
            cur = start.copy()
            break
        cur = new
        trace.append(dict(row, status=OK, pose=cur.copy()))
        if SR.stopped(x, **o):
            break
    rec["pose"] = cur.copy()
    return cur, rec, trace


def track(vol, scans, colors, pose0, distance=0.0, min_range=0.0, **kw):
    """icp_track_scans_sdf_photometric: tsdf_cloud_color_restatement.track with the photometric alignment.  Returns (poses, records, infos,
    status, n_colored of every scan -- 0 for a skipped one)."""
    pose = np.asarray(pose0, f32).copy()
    info, _, nc = CC.integrate(vol, scans[0], colors[0], pose, None, distance, min_range)
    poses, recs, infos, ncs, status = [pose.copy()], [], [info], [nc], OK
    for k in range(1, len(scans)):
        pose, rec, _ = align(vol, scans[k], colors[k], pose, **kw)
        if rec["status"] == OK:
            info, _, nc = CC.integrate(vol, scans[k], colors[k], pose, None, distance, min_range)
            infos.append(info); ncs.append(nc)
        else:
            infos.append(dict(SC.ZERO_INFO)); ncs.append(0)
            if status == OK:
                status = rec["status"]
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs, infos, status, ncs
