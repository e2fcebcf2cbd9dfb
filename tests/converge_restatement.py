"""Stopping on a converged pose (icp_set_convergence_options, include/icp_hip.h) restated in plain numpy: the measure of one iteration
and the eligibility / streak / stop arithmetic over the recorded poses of a run with the option off.  The operation order is the one the
header states, in fp64 on values widened from fp32; both measures are rounded once to fp32."""
import numpy as np

f32 = np.float32


def measure(A, B, dtype=f32):
    """(rotation, translation) of the step from pose B (searched at) to pose A (after the iteration); 4x4, (row, col).  dtype fp32: the
    contract -- fp32 poses in, fp32 measures out; dtype fp64: the same formulas with no rounding at either end (to check them on exact poses)."""
    A = np.asarray(A, dtype).astype(np.float64); B = np.asarray(B, dtype).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dR = np.empty((3, 3))
        for r in range(3):
            for c in range(3):
                dR[r, c] = (A[r, 0] * B[c, 0] + A[r, 1] * B[c, 1]) + A[r, 2] * B[c, 2]
        tb = B[:3, 3]
        dt = [A[r, 3] - ((dR[r, 0] * tb[0] + dR[r, 1] * tb[1]) + dR[r, 2] * tb[2]) for r in range(3)]
        v = (dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1])
        rot = np.inf if ((dR[0, 0] + dR[1, 1]) + dR[2, 2]) - 1.0 <= 0.0 else 0.5 * np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        tr = np.sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2])
        return dtype(rot), dtype(tr)


def met(rot, tr, opts):
    """The criterion; written so that a NaN fails it."""
    return bool(rot <= f32(opts["rotation"]) and tr <= f32(opts["translation"]))


def eligible(factors, statuses=None):
    """Per iteration: status ICP_OK, the decimation factor of the schedule's last iteration, and (i > 0) of the iteration before."""
    n = len(factors)
    return [bool((statuses is None or statuses[i] == 0) and factors[i] == factors[n - 1] and (i == 0 or factors[i] == factors[i - 1])) for i in range(n)]


def stop_index(poses, pose_in, factors, statuses, opts):
    """poses[i] = the pose after iteration i of the run with the option off.  Returns (n_run, converged, trace) with trace one
    (rotation, translation, eligible, streak) per iteration that runs."""
    n = len(poses)
    assert len(factors) == n
    el = eligible(list(factors), statuses)
    patience, min_it = int(opts.get("patience", 1)), int(opts.get("min_iterations", 1))
    trace, streak = [], 0
    for i in range(n):
        rot, tr = measure(poses[i], pose_in if i == 0 else poses[i - 1])
        streak = streak + 1 if el[i] and met(rot, tr, opts) else 0
        trace.append((rot, tr, int(el[i]), streak))
        if streak >= patience and i + 1 >= min_it:
            return i + 1, True, trace
    return n, False, trace
