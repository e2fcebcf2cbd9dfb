"""Initial poses for multi-start ICP (Context.run_multistart / icp_run_multistart).

ICP is local: from a poor initial pose it settles in a wrong minimum.  The usual remedy is to start it from several poses and keep the
best result; start_poses makes such a set -- the caller's initial pose composed with rotations about the source cloud's centroid.
"""
import numpy as np


def rotation(axis, deg):
    """3 x 3 rotation by `deg` degrees about the unit vector `axis` (Rodrigues, fp64)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(float(deg))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def start_poses(initial, yaw_deg=(0.0,), axis=(0.0, 0.0, 1.0), center=None, points=None):
    """One 4 x 4 float32 pose per angle of yaw_deg: initial composed from the left with the rotation by that angle about `axis` through
    the centroid c of the moved source, i.e. T_k = [R_k | c - R_k c] @ initial.  c = `center` when given, else the mean of the finite
    `points` (the source cloud) moved by `initial`, else the translation of `initial`.  An angle of 0 gives `initial` itself."""
    P = np.asarray(initial, dtype=np.float64).reshape(4, 4)
    if center is not None:
        c = np.asarray(center, dtype=np.float64).reshape(3)
    elif points is not None:
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        pts = pts[np.isfinite(pts).all(axis=1)]
        c = (pts.mean(axis=0) @ P[:3, :3].T + P[:3, 3]) if len(pts) else P[:3, 3].copy()
    else:
        c = P[:3, 3].copy()
    out = []
    for deg in yaw_deg:
        T = np.eye(4)
        if float(deg) != 0.0:
            R = rotation(axis, deg)
            T[:3, :3] = R
            T[:3, 3] = c - R @ c
        out.append((T @ P).astype(np.float32))
    return out
