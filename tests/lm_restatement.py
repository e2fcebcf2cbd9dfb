"""fp64 numpy restatement of the non-linear optimiser (CeresICPOptimizer, ICPOptimizer.h:181-483), written from the contract in
DESIGN.md ("The non-linear optimiser"): the residual blocks of constraints.h with their autodiff Jacobians, and one ceres::Solve
(Levenberg-Marquardt, monotonic, Jacobi scaling, Ceres' default tolerances) per ICP iteration.  Test infrastructure only.

  blocks(...)            the residual blocks one ICP iteration forms from its records (validity rules of prepareConstraints*)
  evaluate(x, b)         cost = 1/2 f^T f, J^T J, J^T f of those blocks at x (Jets over the rotation, as autodiff)
  solve(ev, opts)        one Solve from x = 0: x, the summary and the per-iteration decisions
  compose(x, pose)       estimatedPose = float(AngleAxisToRotationMatrix(x), t) * estimatedPose in fp32
"""
import numpy as np

CONVERGENCE, NO_CONVERGENCE, FAILURE, NO_RESIDUALS = 0, 1, 2, 3
DBL_EPS = np.finfo(np.float64).eps
LAMBDA_POINT = float(np.float32(0.1))


def default_options():
    return dict(initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32, min_relative_decrease=1e-3,
                min_lm_diagonal=1e-6, max_lm_diagonal=1e32, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
                max_num_iterations=10, max_num_consecutive_invalid_steps=5, jacobi_scaling=1)


# ---- Jets over the three rotation parameters: array (4, ...) = value, d/dx0, d/dx1, d/dx2 (ceres::Jet rules) ----
def jconst(a):
    a = np.asarray(a, np.float64)
    z = np.zeros_like(a)
    return np.stack([a, z, z, z])


def jmul(f, g):
    return np.stack([f[0] * g[0], f[0] * g[1] + f[1] * g[0], f[0] * g[2] + f[2] * g[0], f[0] * g[3] + f[3] * g[0]])


def jsqrt(f):
    t = np.sqrt(f[0]); d = 2.0 * t
    return np.stack([t, f[1] / d, f[2] / d, f[3] / d])


def jcos(f):
    s = -np.sin(f[0])
    return np.stack([np.cos(f[0]), s * f[1], s * f[2], s * f[3]])


def jsin(f):
    c = np.cos(f[0])
    return np.stack([np.sin(f[0]), c * f[1], c * f[2], c * f[3]])


def jrecip(g):
    m = -1.0 / (g[0] * g[0])
    return np.stack([1.0 / g[0], g[1] * m, g[2] * m, g[3] * m])


def rotation(x):
    """The point-independent part of ceres::AngleAxisRotatePoint at x, with derivatives."""
    a = [np.array([x[k], k == 0, k == 1, k == 2], np.float64) for k in range(3)]
    theta2 = jmul(a[0], a[0]) + jmul(a[1], a[1]) + jmul(a[2], a[2])
    big = theta2[0] > DBL_EPS
    if big:
        theta = jsqrt(theta2)
        c, s = jcos(theta), jsin(theta)
        ti = jrecip(theta)
        w = [jmul(a[k], ti) for k in range(3)]
    else:
        c, s, w = jconst(1.0), jconst(0.0), a
    return dict(big=big, c=c, s=s, omc=jconst(1.0) - c, w=w, t=np.asarray(x[3:6], np.float64))


def rotate(R, p, sign=1.0):
    """R(sign x) p for points p (N, 3) float64: three Jets (4, N).  sign -1 = apply_inv_rotation (the cross term changes sign)."""
    w = [wk[:, None] for wk in R["w"]]
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    cr = [w[1] * p2 - w[2] * p1, w[2] * p0 - w[0] * p2, w[0] * p1 - w[1] * p0]
    out = []
    if R["big"]:
        c, s, omc = R["c"][:, None], R["s"][:, None], R["omc"][:, None]
        tmp = jmul((w[0] * p0 + w[1] * p1) + w[2] * p2, np.broadcast_to(omc, (4, len(p))))
        for k in range(3):
            out.append((c * p[:, k] + jmul(cr[k], np.broadcast_to(s, (4, len(p)))) * sign) + jmul(np.broadcast_to(w[k], (4, len(p))), tmp))
    else:
        for k in range(3):
            out.append(jconst(p[:, k]) + cr[k] * sign)
    return out


def blocks(metric, src_t, nrm_t, tgt, tgt_nrm, matches):
    """Residual-block inputs of one ICP iteration: src_t / nrm_t the transformed (fp32) source points / normals of the matched set,
    tgt / tgt_nrm the target cloud, matches the records after weighting + rejection.  Pairs with idx >= 0 and a finite source and
    target point; `second` marks the ones with a second block (point-to-plane: finite target normal, symmetric: both normals finite)."""
    idx = matches["idx"].astype(np.int64)
    ok = idx >= 0
    s = np.asarray(src_t, np.float32)[ok]; j = idx[ok]
    q = np.asarray(tgt, np.float32)[j]
    fin = np.isfinite(s).all(1) & np.isfinite(q).all(1)
    s, q, j = s[fin], q[fin], j[fin]
    w = matches["weight"][ok][fin].astype(np.float32)
    nq = np.asarray(tgt_nrm, np.float32)[j] if metric != 0 else np.zeros_like(q)
    npt = np.asarray(nrm_t, np.float32)[ok][fin] if metric == 2 else np.zeros_like(q)
    if metric == 1:
        second = np.isfinite(nq).all(1)
    elif metric == 2:
        second = np.isfinite(nq).all(1) & np.isfinite(npt).all(1)
    else:
        second = np.zeros(len(s), bool)
    return dict(metric=metric, s=s, q=q, nq=nq, np=npt, w=w, second=second)


def residuals(x, b):
    """Rows of the problem at x: (f (R,), J (R, 6)) in block order (pair by pair: 3 point rows, then the second block)."""
    R = rotation(x)
    s, q = b["s"].astype(np.float64), b["q"].astype(np.float64)
    w = b["w"].astype(np.float64)
    lw, l1 = LAMBDA_POINT * w, 1.0 * w
    o = rotate(R, s)
    st = [o[k] + jconst(R["t"][k])[:, None] for k in range(3)]
    rows_f, rows_J = [], []
    n = len(s)
    for k in range(3):
        e = (st[k] - jconst(q[:, k])) * lw
        J = np.zeros((n, 6)); J[:, 0:3] = e[1:].T; J[:, 3 + k] = lw
        rows_f.append(e[0]); rows_J.append(J)
    if b["metric"] != 0:
        if b["metric"] == 1:
            m = b["nq"].astype(np.float64)
            d = [st[k] - jconst(q[:, k]) for k in range(3)]
        else:
            m = b["nq"].astype(np.float64) + b["np"].astype(np.float64)
            u = rotate(R, q, -1.0)
            d = [st[k] - u[k] for k in range(3)]
        sec = ((d[0] * m[:, 0] + d[1] * m[:, 1]) + d[2] * m[:, 2]) * l1
        J = np.zeros((n, 6)); J[:, 0:3] = sec[1:].T; J[:, 3:6] = m * l1[:, None]
        sel = b["second"]
        rows_f.append(sec[0][sel]); rows_J.append(J[sel])
    return np.concatenate(rows_f), np.concatenate(rows_J)


def evaluate(x, b):
    f, J = residuals(np.asarray(x, np.float64), b)
    return 0.5 * float(f @ f), J.T @ J, J.T @ f


def n_blocks(b):
    return len(b["s"]) + int(b["second"].sum())


def solve(ev, opts=None, nblocks=1):
    """One ceres::Solve from x = 0.  ev(x) -> (cost, JtJ (6,6), Jtf (6,)).  Returns (x, summary, decisions); decisions is the list of
    'accept' / 'reject' / 'invalid' per LM iteration."""
    o = default_options()
    o.update(opts or {})
    summ = dict(iterations=0, successful_steps=0, unsuccessful_steps=0, invalid_steps=0, termination=NO_RESIDUALS, n_residual_blocks=nblocks,
                accepted_steps_mask=0, invalid_steps_mask=0,
                initial_cost=0.0, final_cost=0.0, trust_region_radius=o["initial_trust_region_radius"], x=np.zeros(6))
    decisions = []
    if nblocks <= 0:
        return np.zeros(6), summ, decisions
    x = np.zeros(6)
    cost, H, g = ev(x)
    summ["initial_cost"] = cost
    radius, factor = o["initial_trust_region_radius"], 2.0
    if not (np.isfinite(cost) and np.isfinite(H).all() and np.isfinite(g).all()):
        summ.update(termination=FAILURE, final_cost=cost)
        return np.zeros(6), summ, decisions
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H))) if o["jacobi_scaling"] else np.ones(6)
    it, succ, unsucc, inval, consec = 0, 0, 0, 0, 0
    success = True
    reason = None
    x_norm = 0.0
    while True:
        # FinalizeIterationAndCheckIfMinimizerCanContinue
        if success:
            succ += 1
            gmax = float(np.max(np.abs(g)))
        else:
            unsucc += 1
        if it >= o["max_num_iterations"]:
            reason = NO_CONVERGENCE; break
        if success and gmax <= o["gradient_tolerance"]:
            reason = CONVERGENCE; break
        if radius < o["min_trust_region_radius"]:
            reason = CONVERGENCE; break
        it += 1
        Hs = H * scale[:, None] * scale[None, :]
        gs = scale * g
        A = Hs + np.diag(np.clip(np.diag(Hs), o["min_lm_diagonal"], o["max_lm_diagonal"]) / radius)
        valid = True
        try:
            L = np.linalg.cholesky(A)
            y = np.linalg.solve(L.T, np.linalg.solve(L, gs))
            valid = bool(np.isfinite(y).all())
        except np.linalg.LinAlgError:
            valid = False
        if valid:
            step = -y
            mcc = -(step @ gs + 0.5 * step @ Hs @ step)
            valid = bool(mcc > 0.0 and np.isfinite(mcc))
        if not valid:
            inval += 1; consec += 1
            decisions.append("invalid")
            if consec >= o["max_num_consecutive_invalid_steps"]:
                reason = FAILURE; break
            radius /= factor; factor *= 2.0
            success = False
            continue
        consec = 0
        delta = step * scale
        cand = x + delta
        cc, Hc, gc = ev(cand)
        if not np.isfinite(cc):
            cc = np.finfo(np.float64).max
        if np.linalg.norm(delta) <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            reason = CONVERGENCE; decisions.append("parameter_tolerance"); break
        if abs(cost - cc) <= o["function_tolerance"] * cost:
            reason = CONVERGENCE; decisions.append("function_tolerance"); break
        rho = (cost - cc) / mcc
        if rho > o["min_relative_decrease"]:
            x, cost, H, g = cand, cc, Hc, gc
            x_norm = float(np.linalg.norm(x))
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), o["max_trust_region_radius"])
            factor = 2.0
            success = True
            decisions.append("accept")
        else:
            radius /= factor; factor *= 2.0
            success = False
            decisions.append("reject")
    xf = np.zeros(6) if reason == FAILURE else x
    acc = sum(1 << k for k, d in enumerate(decisions[:32]) if d == "accept")
    inv = sum(1 << k for k, d in enumerate(decisions[:32]) if d == "invalid")
    summ.update(iterations=it, successful_steps=succ, unsuccessful_steps=unsucc, invalid_steps=inval, termination=reason,
                final_cost=cost, trust_region_radius=radius, x=xf.copy(), accepted_steps_mask=acc, invalid_steps_mask=inv)
    return xf, summ, decisions


def solve_blocks(b, opts=None):
    return solve(lambda x: evaluate(x, b), opts, n_blocks(b))


def angle_axis_to_matrix(x):
    """ceres::AngleAxisToRotationMatrix in fp64 (row, col)."""
    t2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
    if t2 > DBL_EPS:
        th = np.sqrt(t2); wx, wy, wz = x[0] / th, x[1] / th, x[2] / th
        c, s = np.cos(th), np.sin(th); o = 1.0 - c
        return np.array([[c + wx * wx * o, wx * wy * o - wz * s, wy * s + wx * wz * o],
                         [wz * s + wx * wy * o, c + wy * wy * o, -wx * s + wy * wz * o],
                         [-wy * s + wx * wz * o, wx * s + wy * wz * o, c + wz * wz * o]])
    return np.array([[1.0, -x[2], x[1]], [x[2], 1.0, -x[0]], [-x[1], x[0], 1.0]])


def compose(x, pose):
    """convertToMatrix(x) * pose (ICPOptimizer.h:309) as the fp32 Matrix4f product, sequential over k."""
    D = np.eye(4, dtype=np.float32)
    D[:3, :3] = angle_axis_to_matrix(np.asarray(x, np.float64)).astype(np.float32)
    D[:3, 3] = np.asarray(x[3:6], np.float64).astype(np.float32)
    P = np.asarray(pose, np.float32)
    out = D[:, 0:1] * P[0:1, :]
    for k in range(1, 4):
        out = (out + D[:, k:k + 1] * P[k:k + 1, :]).astype(np.float32)
    return out.astype(np.float32)


def transform_points(pts, pose):
    """transformPoints in fp32 with the device's operation order: ((R0 x + R1 y) + R2 z) + t."""
    P = np.asarray(pose, np.float32); p = np.asarray(pts, np.float32)
    return np.stack([((P[r, 0] * p[:, 0] + P[r, 1] * p[:, 1]) + P[r, 2] * p[:, 2]) + P[r, 3] for r in range(3)], 1).astype(np.float32)
