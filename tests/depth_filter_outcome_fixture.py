"""The outcome fixture of the bilateral depth filter (tests/test_depth_filter_host.py, tests/test_gpu_depth_filter.py):
what filtering buys on NOISY frames, measured with the numpy restatements alone.  Frames: the 41-frame, 60 degree pan of
tests/tsdf_outcome_fixture.py built with synth.depth_frame(..., sigma=SIGMA); filter: the default options at radius 3.

  * normals: on frame 0, the mean angle between the back-projected normals (the oracle's PointCloud constructor) and synth's true normals
    over the pixels that keep a normal both raw and filtered, and the number of pixels that keep one -- raw and filtered;
  * direct SDF tracking: the worst rotation and translation error of the pan tracked by tests/sdf_restatement.py at stride 4 with 20
    iterations, raw and filtered (the filtered run aligns the filtered frame and fuses the raw one, as the library does).

SIGMA starts from 2 mm (a Kinect at 1.5 to 2 m) and is the value at which the UNFILTERED run still returns OK for every frame; it is written
into the JSON.  Run as a script (CPU only, a few minutes) it writes tests/golden/depth_filter_outcome.json."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "depth_filter_outcome.json")
f32 = np.float32
SIGMA = 0.002
FILTER = dict(radius=3, sigma_space=4.5, sigma_range=0.03)
OPTIONS = dict(stride=4, n_iterations=20)
MAX_DISTANCE = 0.1                       # the back-projection's edge test (PointCloud's maxDistance), as everywhere in the tests


def noisy_frames(sigma=SIGMA, n_frames=None):
    """tsdf_outcome_fixture.fixture() with depth noise: (K, depth (n, H, W), gt, the true camera-frame normals of frame 0 (H * W, 3))."""
    import tsdf_outcome_fixture as OF
    from icp_amd import synth
    n = OF.N_FRAMES if n_frames is None else n_frames
    K = synth.tum_K(OF.W)
    T = [synth.camera_pose(0) @ synth.make_pose((0, np.deg2rad(1.5 * k), 0), (0.01 * k, 0, 0)) for k in range(n)]
    made = [synth.depth_frame(Tk, K.astype(np.float64), OF.W, OF.H, 0x7A11 + k, 0.05, sigma=sigma) for k, Tk in enumerate(T)]
    depth = np.stack([m[0][:, 2].reshape(OF.H, OF.W).copy() for m in made])
    gt = [(np.linalg.inv(T[0]) @ Tk).astype(f32) for Tk in T[1:]]
    return K, depth, gt, made[0][1]


def restatement_filter(depth):
    """`depth` (h, w) or (n, h, w) through the restatement with the library's own tables for FILTER."""
    import depth_filter_restatement as DF
    from icp_amd import binding
    S, R, ib = binding.depth_filter_tables(**FILTER)
    d = np.asarray(depth, f32)
    if d.ndim == 2:
        return DF.filter_depth(d, FILTER["radius"], S, R, ib)
    return np.stack([DF.filter_depth(x, FILTER["radius"], S, R, ib) for x in d])


def normal_measures(nrm_raw, nrm_filtered, nrm_true):
    """(mean angle raw [rad], mean angle filtered [rad], kept raw, kept filtered): a pixel keeps a normal when all three components are
    finite; the means run over the pixels that keep one in both (and have a true normal: not a hole of the frame)."""
    a, b, t = (np.asarray(x, np.float64).reshape(-1, 3) for x in (nrm_raw, nrm_filtered, nrm_true))
    ka, kb = np.isfinite(a).all(1), np.isfinite(b).all(1)
    both = ka & kb & np.isfinite(t).all(1)

    def mean_angle(n):
        n = n[both]; tt = t[both]
        c = (n * tt).sum(1) / (np.linalg.norm(n, axis=1) * np.linalg.norm(tt, axis=1))
        return float(np.arccos(np.clip(np.abs(c), 0.0, 1.0)).mean())      # (the angle between the lines: the sign convention plays no part)
    return mean_angle(a), mean_angle(b), int(ka.sum()), int(kb.sum())


def track(depth_align, depth_fuse, K):
    """sdf_restatement.track with the frame that is aligned and the frame that is fused apart.  Returns (poses, records)."""
    import sdf_restatement as SR
    import tsdf_restatement as TS
    import tsdf_outcome_fixture as OF
    vol = TS.Volume(**OF.VOLUME); cam = TS.Camera(K, OF.W, OF.H)
    pose = np.eye(4, dtype=f32)
    TS.integrate(vol, depth_fuse[0], cam, pose)
    poses, recs = [pose.copy()], []
    for k in range(1, len(depth_fuse)):
        pose, rec, _ = SR.align(vol, depth_align[k], cam, pose, **OPTIONS)
        if rec["status"] == SR.OK:
            TS.integrate(vol, depth_fuse[k], cam, pose)
        poses.append(pose.copy()); recs.append(rec)
    return poses, recs


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import tsdf_outcome_fixture as OF
    from oracle import oracle
    oracle.build()
    K, depth, gt, nrm_true = noisy_frames()
    filt = restatement_filter(depth)
    _, n_raw, _, _ = oracle.backproject(depth[0], None, K, max_distance=MAX_DISTANCE)
    _, n_filt, _, _ = oracle.backproject(filt[0], None, K, max_distance=MAX_DISTANCE)
    a_raw, a_filt, k_raw, k_filt = normal_measures(n_raw, n_filt, nrm_true)
    # for scale: the same measure on the frame WITHOUT noise (its own kept pixels) -- the reference's normal is (-du, -dv, 1) normalised with
    # du, dv in metres per PIXEL, not the surface normal, so the angle to the true normal is large whatever the noise is
    _, clean, _, _ = noisy_frames(sigma=0.0, n_frames=1)
    n_clean = oracle.backproject(clean[0], None, K, max_distance=MAX_DISTANCE)[1]
    a_clean, _, k_clean, _ = normal_measures(n_clean, n_clean, nrm_true)
    out = dict(sigma_m=SIGMA, filter=FILTER, frames=OF.N_FRAMES, width=OF.W, height=OF.H, stride=OPTIONS["stride"], n_iterations=OPTIONS["n_iterations"],
               normals=dict(raw_mean_angle_rad=a_raw, filtered_mean_angle_rad=a_filt, raw_kept=k_raw, filtered_kept=k_filt,
                            noise_free_mean_angle_rad=a_clean, noise_free_kept=k_clean))
    for name, align in (("raw", depth), ("filtered", filt)):
        poses, recs = track(align, depth, K)
        rot, tr, last = OF.worst_errors(poses, gt)
        out[name] = dict(worst_rotation_rad=rot, worst_translation_m=tr, last_rotation_rad=last[0], last_translation_m=last[1],
                         statuses=sorted(set(r["status"] for r in recs)), iterations=[r["iterations"] for r in recs])
    print(json.dumps(out))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
