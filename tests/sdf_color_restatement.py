"""The contract of direct SDF tracking with a photometric term (include/icp_hip.h: icp_tsdf_sample_color, icp_tsdf_sdf_system_color,
icp_tsdf_align_depth_color, icp_track_depth_sdf_color) restated in numpy.  Written from the contract alone, on top of sdf_restatement (SR:
sampling, the geometric terms, the solve and the pose composition), tsdf_restatement (TS) and tsdf_color_restatement (TC: the colour array
and its integration).  Every fp32 operation is one numpy float32 operation in the order the contract writes it, everything after the
conversion to fp64 is numpy float64.  `sample_color` is compared with the device bit for bit; `system` returns, next to every sum, the sum
of the absolute values of its terms, which bounds what another summation order may change.  Contains no device code."""
import numpy as np

import sdf_restatement as SR
import tsdf_color_restatement as TC
import tsdf_restatement as TS

f32, f64 = np.float32, np.float64
OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = SR.OK, SR.ERR_NO_SOURCE, SR.ERR_NO_CORRESPONDENCES
COLOR_DEFAULTS = dict(weight=0.1, huber=0.0)


def color_options(**kw):
    o = dict(COLOR_DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError("icp_sdf_color_options has no field %r" % k)
        o[k] = v
    return o


def _intensity_field(vol, qx, qy, qz):
    """(cell inside the volume, all eight Wc > 0, S, H_x, H_y, H_z) at fp32 world points; S and H raw where the cell is not usable."""
    with np.errstate(all="ignore"):
        g = [(q - vol.o[a]) / vol.s for a, q in enumerate((qx, qy, qz))]
        fl = [np.floor(x) for x in g]
        inside = np.ones(len(qx), bool)
        for a, n in enumerate((vol.nx, vol.ny, vol.nz)):
            inside &= (fl[a] >= 0) & (fl[a] <= f32(n - 2))
        tx, ty, tz = [g[a] - fl[a] for a in range(3)]
        i = [np.where(inside, fl[a], 0).astype(np.int64) for a in range(3)]
        s = np.empty((8, len(qx)), f32)
        all8 = inside.copy()
        for k in range(8):
            dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
            c = vol.rgb[i[2] + dz, i[1] + dy, i[0] + dx]
            s[k] = (c[:, 0] + c[:, 1]) + c[:, 2]
            all8 &= vol.wc[i[2] + dz, i[1] + dy, i[0] + dx] > 0
        L = TS._lerp
        S = L(L(L(s[0], s[1], tx), L(s[2], s[3], tx), ty), L(L(s[4], s[5], tx), L(s[6], s[7], tx), ty), tz)
        hx = L(L(s[1] - s[0], s[3] - s[2], ty), L(s[5] - s[4], s[7] - s[6], ty), tz)
        hy = L(L(s[2] - s[0], s[3] - s[1], tx), L(s[6] - s[4], s[7] - s[5], tx), tz)
        hz = L(L(s[4] - s[0], s[5] - s[1], tx), L(s[6] - s[2], s[7] - s[3], tx), ty)
    return inside, all8, S, hx, hy, hz


def sample_color(vol, points):
    """icp_tsdf_sample_color: (S (n,), H (n, 3) per voxel, valid (n,) uint8).  valid: the cell lies inside the volume and its eight Wc > 0;
    an invalid point reads 0; a NaN is the canonical quiet NaN."""
    p = np.ascontiguousarray(points, f32).reshape(-1, 3)
    _, valid, S, hx, hy, hz = _intensity_field(vol, p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy())
    Hh = np.stack([hx, hy, hz], 1)
    S = np.where(valid, S, f32(0)); Hh = np.where(valid[:, None], Hh, f32(0))
    return SR._canonical(S), SR._canonical(Hh), valid.astype(np.uint8)


def pixel_terms(vol, depth, rgbx, cam, pose, stride=1):
    """SR.pixel_terms (usable, valid, q, r, g, u, v) with, per sampled pixel: colored (n,), r_c (n,) and h (n, 3) in fp64."""
    t = SR.pixel_terms(vol, depth, cam, pose, stride)
    q = t["q"]
    _, all8, S, hx, hy, hz = _intensity_field(vol, q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())
    px = np.ascontiguousarray(rgbx, np.uint8).reshape(-1, 4)[t["v"] * cam.width + t["u"]].astype(np.int64)
    with np.errstate(all="ignore"):
        Ip = (px[:, 0] + px[:, 1] + px[:, 2]).astype(f64) / f64(765.0)
        rc = S.astype(f64) / f64(765.0) - Ip
        den = f64(765.0) * f64(vol.s)
        h = np.stack([hx.astype(f64) / den, hy.astype(f64) / den, hz.astype(f64) / den], 1)
    t.update(colored=t["valid"] & all8 & np.isfinite(S), r_c=rc, h=h, S=S)
    return t


def _rows(w, J, r):
    """The 28 lane terms of a row set: (w J_i) J_j, -((w J_i) r), (w r) r."""
    terms = np.empty((28, len(r)), f64)
    wJ = w[:, None] * J
    k = 0
    for i in range(6):
        for j in range(i, 6):
            terms[k] = wJ[:, i] * J[:, j]; k += 1
    for i in range(6):
        terms[21 + i] = -(wJ[:, i] * r)
    terms[27] = (w * r) * r
    return terms


def _huber(r, huber):
    w = np.ones(len(r), f64)
    if f32(huber) > 0:
        h = f64(f32(huber)); ar = np.abs(r)
        with np.errstate(all="ignore"):
            w = np.where(ar <= h, 1.0, h / ar)
    return w


def system(vol, depth, rgbx, cam, pose, stride=1, huber=0.0, weight=0.1, color_huber=0.0, **_):
    """icp_tsdf_sdf_system_color: ((n_depth, n_valid, n_color), sums (29,) fp64, sum of |geometric term| + |photometric term| per sum (29,)).
    huber: icp_sdf_options'; weight, color_huber: icp_sdf_color_options' weight and huber."""
    t = pixel_terms(vol, depth, rgbx, cam, pose, stride)
    m = t["valid"]
    with np.errstate(all="ignore"):
        r = t["r"][m]
        geo = _rows(_huber(r, huber), SR.jacobian(t["q"][m], t["g"][m]), r)
        c = t["colored"][m]
        rc = t["r_c"][m][c]
        wc = (f64(f32(weight)) * f64(f32(weight))) * _huber(rc, color_huber)
        pho = _rows(wc, SR.jacobian(t["q"][m][c], t["h"][m][c]), rc)
        terms = np.zeros((29, len(r)), f64); mag = np.zeros((29, len(r)), f64)
        terms[:28] = geo; mag[:28] = np.abs(geo)
        terms[:28, c] = geo[:, c] + pho; mag[:28, c] += np.abs(pho)
        terms[28, c] = pho[27]; mag[28, c] = np.abs(pho[27])
    return (int(t["usable"].sum()), int(m.sum()), int(t["colored"].sum())), terms.sum(1), mag.sum(1)


def align(vol, depth, rgbx, cam, pose, weight=0.1, color_huber=0.0, **kw):
    """icp_tsdf_align_depth_color: (pose, record, trace); SR.align's loop on the 29 sums."""
    o = SR.options(**kw)
    start = np.asarray(pose, f32).copy(); cur = start.copy()
    rec = dict(n_depth=0, n_valid_first=0, n_valid_last=0, n_color_first=0, n_color_last=0, iterations=0, status=OK, cost_first=0.0, cost_last=0.0,
               cost_color_first=0.0, cost_color_last=0.0)
    trace = []
    for it in range(o["n_iterations"]):
        counts, sums, _ = system(vol, depth, rgbx, cam, cur, weight=weight, color_huber=color_huber, **o)
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


def track(vol, frames, rgbx_frames, cam, pose0, **kw):
    """icp_track_depth_sdf_color: frame 0 integrated with its colours at pose0; frame k aligned from the current pose and, on success,
    integrated with its colours at the pose found.  Returns (poses after every frame, frame 0 included; records of frames 1 ..)."""
    pose = np.asarray(pose0, f32).copy()
    TC.integrate_color(vol, frames[0], rgbx_frames[0], cam, pose)
    poses, recs = [pose.copy()], []
    for k in range(1, len(frames)):
        pose, rec, _ = align(vol, frames[k], rgbx_frames[k], cam, pose, **kw)
        if rec["status"] == OK:
            TC.integrate_color(vol, frames[k], rgbx_frames[k], cam, pose)
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs


def smooth_colors(vol):
    """A fixture of the tests, not part of the contract: a colour array that is a smooth function of the voxel's position, per channel a
    sinusoid of amplitude <= 60 bytes and wavelength >= 1.5 m.  At 0.1 m voxels s = R + G + B changes by less than 64 per voxel along
    any axis, which the Jacobian test asserts.  Every voxel coloured (Wc = 1)."""
    TC.add_color(vol)
    x = (vol.o[0] + np.arange(vol.nx) * f64(vol.s))[None, None, :]; y = (vol.o[1] + np.arange(vol.ny) * f64(vol.s))[None, :, None]
    z = (vol.o[2] + np.arange(vol.nz) * f64(vol.s))[:, None, None]
    r = 128 + 60 * np.sin(2 * np.pi * (x + 0.3 * y) / 1.7) + 0 * z
    g = 120 + 50 * np.cos(2 * np.pi * (y - 0.2 * x + 0.1 * z) / 1.5)
    b = 110 + 40 * np.sin(2 * np.pi * (0.6 * x + 0.5 * y + 0.3 * z) / 2.1 + 1.0)
    vol.rgb = np.stack([r, g, b], -1).astype(f32)
    vol.wc = np.ones((vol.nz, vol.ny, vol.nx), f32)
    return vol
