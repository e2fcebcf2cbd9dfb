"""The outcome fixture of laser scans fused into the hashed TSDF volume (tests/test_gpu_tsdf_cloud.py): N_SCANS
synthetic tilting-laser scans of the room (icp_amd.synth.laser_scan at synth.scan_pose(k), beam counts reduced), each moved into its
sensor frame, fused at their true poses by the numpy restatement (tests/tsdf_cloud_restatement.py).  The device equals the restatement bit
for bit, so the GPU test compares its blocks with model()'s exactly; what makes the model worth comparing with is asserted here, on the
CPU: it is a SURFACE -- the field sampled at the noise-free points of a held-out scan is valid for at least half of them, and the median
distance it reports there is at most half a voxel."""
import functools
import numpy as np

f32 = np.float32
N_SCANS, HELD_OUT = 12, 12
N_TILT, N_BEAM = 60, 180
VOXEL, TRUNCATION, MAX_RANGE = 0.1, 0.4, 30.0
ORIGIN = (0.0, 0.0, 0.0)
MIN_VALID_SHARE, MAX_MEDIAN_VOXELS = 0.5, 0.5


def options():
    return dict(origin=ORIGIN, voxel_size=VOXEL, truncation=TRUNCATION, max_depth=MAX_RANGE)


def sensor_frame(points, pose):
    """World points in the frame of `pose` (sensor -> world), fp64, rounded once."""
    T = np.linalg.inv(np.asarray(pose, np.float64))
    return (np.asarray(points, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(f32)


@functools.lru_cache(maxsize=None)
def scans():
    """(clouds: N_SCANS arrays (n, 3) fp32 in the sensor frame, poses: N_SCANS 4x4 fp32 sensor -> world, normals: the clouds' normals in
    the sensor frame, for a tracker)."""
    from icp_amd import synth
    clouds, poses, normals = [], [], []
    for k in range(N_SCANS):
        T = synth.scan_pose(k)
        pts, nrm, _ = synth.laser_scan(T, 0xE7A0 + k, n_tilt=N_TILT, n_beam=N_BEAM)
        clouds.append(sensor_frame(pts, T)); poses.append(T.astype(f32))
        normals.append((nrm.astype(np.float64) @ T[:3, :3]).astype(f32))      # R^T n
    return clouds, poses, normals


@functools.lru_cache(maxsize=None)
def held_out_points():
    """The noise-free points of scan HELD_OUT, in the world frame."""
    from icp_amd import synth
    return synth.laser_scan(synth.scan_pose(HELD_OUT), 0, n_tilt=N_TILT, n_beam=N_BEAM, sigma=0.0)[0]


@functools.lru_cache(maxsize=None)
def model():
    """(the restatement's HVolume after the N_SCANS scans, the info of every scan).  Shared: do not modify."""
    import htsdf_restatement as HR
    import tsdf_cloud_restatement as CR
    clouds, poses, _ = scans()
    vol =HR.HVolume(**options())
    infos = [CR.integrate(vol, c, T) for c, T in zip(clouds, poses)]
    return vol, infos


def surface_figures(vol):
    """(share of the held-out points whose cell is valid, median |F| truncation over those, in metres)."""
    import htsdf_restatement as HR
    F, _, valid = HR.sample(vol, held_out_points())
    ok = valid.astype(bool)
    return float(ok.mean()), float(np.median(np.abs(F[ok].astype(np.float64))) * float(vol.trunc)) if ok.any() else float("inf")


def assert_surface(vol):
    share, median = surface_figures(vol)
    print("held-out scan: %.1f %% of %d points valid, median |F| truncation %.4f m (voxel %.2f m)" % (100 * share, len(held_out_points()), median, VOXEL))
    assert share >= MIN_VALID_SHARE, share
    assert median <= MAX_MEDIAN_VOXELS * VOXEL, median
    return share, median


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__)); root = os.path.abspath(os.path.join(here, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    vol, infos = model()
    print("%d blocks, last scan %s" % (len(vol.blocks), infos[-1]))
    assert_surface(vol)
