"""The outcome fixture of free-space carving: tsdf_cloud_outcome_fixture's twelve scans of the room, with an extra
BOX standing in scans 0 .. 3 only -- intersected into those scans here, ray by ray; the room of icp_amd.synth is not edited -- fused at
their true poses by the numpy restatement (tests/tsdf_carve_restatement.py), once with carving off and once carved all the way to the
sensor.  Something that was scanned and then moved away: without carving it stays in the model for ever, because no later scan observes
anything in front of its own band; with carving the eight later scans vote it out.  What is asserted (conditions, not measurements):
  off   at least half of the valid probes inside the box are negative -- the box is in the model, the test can tell the difference;
  on    no valid probe inside the box is negative and none on its faces is below 0: no zero crossing is left;
  on    the room is still the surface tsdf_cloud_outcome_fixture.assert_surface asks for, with its own thresholds;
  on    carving has added no block."""
import functools
import numpy as np

import tsdf_cloud_outcome_fixture as CF

f32 = np.float32
# The box.  A ray writes a line ONE voxel wide (section 6ze), and these reduced scans have beams 1.5 x 3 degrees apart: beyond
# 0.1 m / tan(3 deg) = 1.9 m a scan's beams are further apart than a voxel and miss voxels outright.  A voxel that four scans saw from
# behind a face (f down to -1) needs MORE than four later scans through it before its average turns positive (consequence (c) of the
# contract), so the box has to stand where each later scan crosses every voxel of it: within 1.9 m of the later poses, which stay around
# (0.1 .. 0.9, -1.4 .. -1.75, 1.15).  This one is 1.3 to 1.9 m from them, clear of the room's own boxes and of every sensor position.
# (The issue's example box, [0.6, 1.2] x [0.6, 1.2] x [0, 1], stands 2.3 to 2.8 m from every pose: there 6 of 1345 valid inside probes
# and 4 of 957 face probes stay negative with carving on, each at a voxel fewer than five later beams cross -- recorded in DESIGN.md 6zg.)
BOX_LO, BOX_HI = np.array([0.7, -0.8, 0.0]), np.array([1.3, -0.2, 1.0])
BOX_SCANS = 4                   # the box stands in scans 0 .. BOX_SCANS - 1
MIN_HITS = 50                   # rays of each of those scans that must end on it
CARVE = dict(distance=float("inf"), min_range=0.0)


def box_hits(points, pose):
    """(hit (n,) bool, t (n,)): which rays sensor -> point (sensor frame, fp64) meet the box before their point, and where."""
    T = np.asarray(pose, np.float64)
    c = T[:3, 3]
    d = np.asarray(points, np.float64) @ T[:3, :3].T
    r = np.linalg.norm(d, axis=1)
    u = d / r[:, None]
    with np.errstate(all="ignore"):
        t0, t1 = (BOX_LO - c) / u, (BOX_HI - c) / u
    tin, tout = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    return (tin < tout) & (tin > 0) & (tin < r), tin


@functools.lru_cache(maxsize=None)
def scans():
    """(clouds, poses, hits: the number of rays of every scan that end on the box).  The clouds of scans 0 .. 3 are CF's with every ray
    that meets the box cut short at its face (no range noise on those returns)."""
    clouds, poses, _ = CF.scans()
    out, hits = [], []
    for k, (p, T) in enumerate(zip(clouds, poses)):
        p = p.copy()
        if k < BOX_SCANS:
            hit, t = box_hits(p, T)
            q = p[hit].astype(np.float64)
            p[hit] = (q / np.linalg.norm(q, axis=1)[:, None] * t[hit, None]).astype(f32)
            hits.append(int(hit.sum()))
        else:
            hits.append(0)
        out.append(p)
    return out, poses, hits


@functools.lru_cache(maxsize=None)
def model(carved):
    """(the restatement's HVolume after the twelve scans, the info of every scan, the carve stats of every scan).  Shared: do not modify."""
    import htsdf_restatement as HR
    import tsdf_carve_restatement as CV
    clouds, poses, _ = scans()
    vol = HR.HVolume(**CF.options())
    res = [CV.integrate(vol, c, T, None, **(CARVE if carved else {})) for c, T in zip(clouds, poses)]
    return vol, [r[0] for r in res], [r[1] for r in res]


def probes():
    """(inside: a grid of points at least a voxel inside the box, faces: points on its four side faces and its top).  Every probe keeps
    one voxel from the floor the box stands on: the floor is a surface of the room, its zero crossing belongs in the model, and half a
    voxel above it the true field is 0.125 with a centimetre of range noise on top -- the same voxel the mesh check shrinks the box by."""
    m = CF.VOXEL
    ax = [np.arange(BOX_LO[a] + m, BOX_HI[a] - m + 1e-9, m / 2) for a in range(3)]
    inside = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    fx = [np.arange(BOX_LO[a] + m / 2, BOX_HI[a] - m / 2 + 1e-9, m / 2) for a in range(3)]
    fx[2] = np.arange(BOX_LO[2] + m, BOX_HI[2] - m / 2 + 1e-9, m / 2)
    faces = []
    for a in (0, 1):
        for v in (BOX_LO[a], BOX_HI[a]):
            g = np.stack(np.meshgrid(fx[1 - a], fx[2], indexing="ij"), -1).reshape(-1, 2)
            p = np.empty((len(g), 3)); p[:, a] = v; p[:, 1 - a] = g[:, 0]; p[:, 2] = g[:, 1]
            faces.append(p)
    g = np.stack(np.meshgrid(fx[0], fx[1], indexing="ij"), -1).reshape(-1, 2)
    faces.append(np.column_stack([g, np.full(len(g), BOX_HI[2])]))
    return inside.astype(f32), np.concatenate(faces).astype(f32)


def box_figures(vol):
    """dict(inside_valid, inside_negative, faces_valid, faces_below_0, faces_min, faces_near: |F| < 0.25) of the field at the probes."""
    import htsdf_restatement as HR
    inside, faces = probes()
    Fi, _, vi = HR.sample(vol, inside); Ff, _, vf = HR.sample(vol, faces)
    vi, vf = vi.astype(bool), vf.astype(bool)
    return dict(inside_valid=int(vi.sum()), inside_negative=int((Fi[vi] < 0).sum()), faces_valid=int(vf.sum()), faces_below_0=int((Ff[vf] < 0).sum()),
                faces_min=float(Ff[vf].min()) if vf.any() else float("nan"), faces_near=int((np.abs(Ff[vf]) < 0.25).sum()))


def vertices_in_box(vertices, shrink=CF.VOXEL):
    """How many mesh vertices lie inside the box shrunk by `shrink` on every side (the floor side included)."""
    v = np.asarray(vertices, np.float64)
    return int(((v > BOX_LO + shrink) & (v < BOX_HI - shrink)).all(1).sum())


def assert_outcome():
    _, _, hits = scans()
    assert all(h >= MIN_HITS for h in hits[:BOX_SCANS]), hits
    off, on = model(False), model(True)
    fo, fn = box_figures(off[0]), box_figures(on[0])
    print("box rays per scan %s" % (hits[:BOX_SCANS],))
    print("carving off: %s, %d blocks" % (fo, len(off[0].blocks)))
    print("carving on:  %s, %d blocks, carved per scan %s" % (fn, len(on[0].blocks), [s["n_carved"] for s in on[2]]))
    assert fo["inside_valid"] > 0 and 2 * fo["inside_negative"] >= fo["inside_valid"], fo
    assert fn["inside_negative"] == 0 and fn["faces_below_0"] == 0 and fn["faces_valid"] > 0, fn
    share, median = CF.assert_surface(on[0])
    assert len(on[0].blocks) == len(off[0].blocks) and sorted(on[0].blocks) == sorted(off[0].blocks)
    return fo, fn, share, median


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__)); root = os.path.abspath(os.path.join(here, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert_outcome()
    print("room without carving:"); CF.assert_surface(model(False)[0])
