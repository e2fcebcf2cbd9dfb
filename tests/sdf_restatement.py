"""The direct SDF tracking contract of include/icp_hip.h (icp_tsdf_sample, icp_tsdf_sdf_system, icp_tsdf_align_depth) restated in numpy.
Written from the contract alone: every fp32 operation is one numpy float32 operation in the order the contract writes it, everything after
the conversion to fp64 is numpy float64.  `sample` is compared with the device bit for bit; `system` returns, next to every sum, the sum of
the absolute values of its terms, which bounds what another summation order may change.  Contains no device code."""
import numpy as np

import tsdf_restatement as TS

f32, f64 = np.float32, np.float64
QNAN = np.uint32(0x7FC00000)
OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES = 0, 4, 8
DEFAULTS = dict(stride=1, n_iterations=20, min_valid=64, huber=0.0, stop_rotation=1e-5, stop_translation=1e-5)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError("icp_sdf_options has no field %r" % k)
        o[k] = v
    return o


def _canonical(a):
    """A NaN is stored as the canonical quiet NaN (its payload depends on the hardware's operand choice)."""
    a = np.ascontiguousarray(a, f32).copy()
    a.view(np.uint32)[np.isnan(a)] = QNAN
    return a


def _field_and_gradient(vol, qx, qy, qz):
    """(cell valid, F, Gx, Gy, Gz) at fp32 world points, F and G raw (whatever the arithmetic gives where the cell is invalid)."""
    valid, c, tx, ty, tz = TS._cell(vol, qx, qy, qz)
    L = TS._lerp
    with np.errstate(all="ignore"):
        e0 = L(L(c[0], c[1], tx), L(c[2], c[3], tx), ty)
        e1 = L(L(c[4], c[5], tx), L(c[6], c[7], tx), ty)
        F = L(e0, e1, tz)
        gx = L(L(c[1] - c[0], c[3] - c[2], ty), L(c[5] - c[4], c[7] - c[6], ty), tz)
        gy = L(L(c[2] - c[0], c[3] - c[1], tx), L(c[6] - c[4], c[7] - c[5], tx), tz)
        gz = L(L(c[4] - c[0], c[5] - c[1], tx), L(c[6] - c[2], c[7] - c[3], tx), ty)
    return valid, F, gx, gy, gz


def sample(vol, points):
    """icp_tsdf_sample: (F (n,), G (n, 3) per voxel, valid (n,) uint8) at world points (n, 3).  valid: the cell lies inside the volume and
    its eight corners are observed; an invalid point reads F = 0 and G = 0; a NaN is the canonical quiet NaN."""
    p = np.ascontiguousarray(points, f32).reshape(-1, 3)
    valid, F, gx, gy, gz = _field_and_gradient(vol, p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy())
    G = np.stack([gx, gy, gz], 1)
    F = np.where(valid, F, f32(0)); G = np.where(valid[:, None], G, f32(0))
    return _canonical(F), _canonical(G), valid.astype(np.uint8)


def pixel_terms(vol, depth, cam, pose, stride=1):
    """Every sampled pixel of the frame at `pose` (4x4 camera -> world, fp32): dict of usable (n,), valid (n,), q (n, 3) fp32, r (n,) and
    g (n, 3) fp64 (metres, per metre), u, v."""
    P = np.asarray(pose, f32)
    d_img = np.ascontiguousarray(depth, f32).reshape(cam.height, cam.width)
    uu, vv = np.meshgrid(np.arange(0, cam.width, stride), np.arange(0, cam.height, stride))
    u = uu.reshape(-1); v = vv.reshape(-1)
    d = d_img[v, u]
    with np.errstate(all="ignore"):
        usable = np.isfinite(d) & (d > 0) & (d <= vol.max_d)
        a = (u.astype(f32) - cam.cx) / cam.fx; b = (v.astype(f32) - cam.cy) / cam.fy
        x = a * d; y = b * d
        q = [(P[r, 0] * x + (P[r, 1] * y + P[r, 2] * d)) + P[r, 3] for r in range(3)]
        cell, F, gx, gy, gz = _field_and_gradient(vol, q[0], q[1], q[2])
        valid = usable & cell & (np.abs(F) < f32(1))
        r = F.astype(f64) * f64(vol.trunc)
        scale = f64(vol.trunc) / f64(vol.s)
        g = np.stack([gx.astype(f64) * scale, gy.astype(f64) * scale, gz.astype(f64) * scale], 1)
    return dict(usable=usable, valid=valid, q=np.stack(q, 1).astype(f32), r=r, g=g, u=u, v=v)


def jacobian(q, g):
    """J = (q x g, g) in fp64, rows (n, 6)."""
    q = np.asarray(q).astype(f64)
    return np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2], q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0],
                     g[:, 0], g[:, 1], g[:, 2]], 1)


def system(vol, depth, cam, pose, stride=1, huber=0.0, **_):
    """icp_tsdf_sdf_system: ((n_depth, n_valid), sums (28,) fp64, sum of |term| per sum (28,)).  Terms: (w J_i) J_j at the upper-triangle
    position i 6 - i (i - 1) / 2 + (j - i); -((w J_i) r) at 21 + i; (w r) r at 27."""
    t = pixel_terms(vol, depth, cam, pose, stride)
    m = t["valid"]
    r = t["r"][m]; J = jacobian(t["q"][m], t["g"][m])
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
    return (int(t["usable"].sum()), int(m.sum())), terms.sum(1), np.abs(terms).sum(1)


def delta(x):
    """dT = [Rx Ry Rz | t] of the six-vector in the library's fp32 order: angles and translations rounded to fp32, sines and cosines in fp64
    rounded once, the two 3 x 3 products as e0 + (e1 + e2)."""
    al, be, ga = (f32(v) for v in x[:3])
    ca, sa = f32(np.cos(f64(al))), f32(np.sin(f64(al)))
    cb, sb = f32(np.cos(f64(be))), f32(np.sin(f64(be)))
    cg, sg = f32(np.cos(f64(ga))), f32(np.sin(f64(ga)))
    z, o = f32(0), f32(1)
    Rx = np.array([[o, z, z], [z, ca, -sa], [z, sa, ca]], f32)
    Ry = np.array([[cb, z, sb], [z, o, z], [-sb, z, cb]], f32)
    Rz = np.array([[cg, -sg, z], [sg, cg, z], [z, z, o]], f32)

    def mul3(A, B):
        out = np.empty((3, 3), f32)
        for r in range(3):
            for c in range(3):
                out[r, c] = f32(f32(A[r, 0] * B[0, c]) + f32(f32(A[r, 1] * B[1, c]) + f32(A[r, 2] * B[2, c])))
        return out
    D = np.eye(4, dtype=f32)
    D[:3, :3] = mul3(mul3(Rx, Ry), Rz)
    D[:3, 3] = [f32(v) for v in x[3:6]]
    return D


def left_compose(D, pose):
    """dT pose in fp32, each element sequential over k: ((D_r0 P_0c + D_r1 P_1c) + D_r2 P_2c) + D_r3 P_3c."""
    D = np.asarray(D, f32); P = np.asarray(pose, f32)
    out = np.empty((4, 4), f32)
    for r in range(4):
        for c in range(4):
            acc = f32(D[r, 0] * P[0, c])
            for k in range(1, 4):
                acc = f32(acc + f32(D[r, k] * P[k, c]))
            out[r, c] = acc
    return out


RANK_CUT = 6.0 * 2.0 ** -23                       # 6 eps_f32: the point-to-plane solve's singular-value cut


def solve(sums):
    """The six-vector of the 27 sums in fp64: H x = b where the rank rule keeps all six directions (every eigenvalue of H above
    (6 eps_f32)^2 of the largest); else the truncated eigen-solve, the sum over the kept directions of v (v . b) / lambda."""
    H = np.zeros((6, 6), f64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = sums[k]; k += 1
    b = np.asarray(sums[21:27], f64)
    lam, V = np.linalg.eigh(H)
    keep = lam > RANK_CUT * RANK_CUT * lam.max()
    if keep.all():
        return np.linalg.solve(H, b)
    x = np.zeros(6, f64)
    for j in np.nonzero(keep)[0]:
        x += V[:, j] * ((V[:, j] @ b) / lam[j])
    return x


def step(sums, counts, pose, min_valid=64, **_):
    """One Gauss-Newton step: (new pose or None when the step fails, x).  Fails with n_valid < min_valid or a non-finite solution."""
    if counts[1] < min_valid:
        return None, None
    try:
        x = solve(sums)
    except np.linalg.LinAlgError:
        return None, None
    new = left_compose(delta(x), pose)
    if not (np.isfinite(x).all() and np.isfinite(new).all()):
        return None, x
    return new, x


def stopped(x, stop_rotation=1e-5, stop_translation=1e-5, **_):
    if not (f32(stop_rotation) > 0 and f32(stop_translation) > 0):
        return False
    return bool((np.abs(x[:3]) <= f64(f32(stop_rotation))).all() and (np.abs(x[3:]) <= f64(f32(stop_translation))).all())


def align(vol, depth, cam, pose, **kw):
    """icp_tsdf_align_depth: (pose, record, trace).  A failed frame carries the pose it started with."""
    o = options(**kw)
    start = np.asarray(pose, f32).copy(); cur = start.copy()
    rec = dict(n_depth=0, n_valid_first=0, n_valid_last=0, iterations=0, status=OK, cost_first=0.0, cost_last=0.0)
    trace = []
    for it in range(o["n_iterations"]):
        counts, sums, _ = system(vol, depth, cam, cur, **o)
        if it == 0:
            rec.update(n_depth=counts[0], n_valid_first=counts[1], cost_first=float(sums[27]))
        rec.update(n_valid_last=counts[1], cost_last=float(sums[27]), iterations=it + 1)
        new, x = (None, None) if counts[0] == 0 else step(sums, counts, cur, **o)
        if new is None:
            rec["status"] = ERR_NO_SOURCE if counts[0] == 0 else ERR_NO_CORRESPONDENCES
            trace.append(dict(n_valid=counts[1], status=rec["status"], cost=float(sums[27]), pose=cur.copy()))
            cur = start.copy()
            break
        cur = new
        trace.append(dict(n_valid=counts[1], status=OK, cost=float(sums[27]), pose=cur.copy()))
        if stopped(x, **o):
            break
    rec["pose"] = cur.copy()
    return cur, rec, trace


def track(vol, frames, cam, pose0, **kw):
    """icp_track_depth_sdf without colours: frame 0 integrated at pose0; frame k aligned from the current pose and, on success, integrated
    at the pose found.  Returns (poses after every frame, frame 0 included; records of frames 1 ..)."""
    pose = np.asarray(pose0, f32).copy()
    TS.integrate(vol, frames[0], cam, pose)
    poses, recs = [pose.copy()], []
    for k in range(1, len(frames)):
        pose, rec, _ = align(vol, frames[k], cam, pose, **kw)
        if rec["status"] == OK:
            TS.integrate(vol, frames[k], cam, pose)
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs
