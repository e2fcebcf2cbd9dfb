"""The outcome fixture of the photometric scan tracker (tests/test_gpu_sdf_cloud_color.py): a flat textured wall at
z = 2 m seen by a sensor that looks along +z and slides 2 cm per scan along x -- nine scans of 140 x 80 rays, the geometry of which leaves
the lateral pose free.  Tracked with 20 iterations, weight 0.1 and the colour Huber off into a volume of 5 cm voxels.  Run as a script (CPU
only) it tracks the scans twice with the numpy restatements, once with the photometric term (sdf_cloud_color_restatement.track) and once
without (tsdf_cloud_color_restatement.track: the same coloured fuses, the geometric alignment), asserts that the fixture separates the two
and writes tests/golden/sdf_cloud_color_outcome.json: the reference the device's bound is twice of."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sdf_cloud_color_outcome.json")
f32 = np.float32
N_SCANS, STEP_M, WALL_Z = 9, 0.02, 2.0
GRID = (140, 80)
VOXEL, TRUNCATION = 0.05, 0.15
DIMS, ORIGIN = (88, 48, 16), (-2.2, -1.2, 1.6)
OPTS = dict(origin=ORIGIN, voxel_size=VOXEL, truncation=TRUNCATION, max_weight=64.0, min_depth=0.3, max_depth=6.0)
OPTIONS = dict(n_iterations=20)
COLOR_OPTIONS = dict(weight=0.1, huber=0.0)
TRAVEL = STEP_M * (N_SCANS - 1)


def texture(x, y):
    """The wall's colour at world (x, y): three smooth sinusoids, wavelengths 0.7 .. 1.1 m, amplitudes 50 .. 70 bytes."""
    r = 128 + 70 * np.sin(2 * np.pi * (x + 0.4 * y) / 0.7)
    g = 125 + 60 * np.cos(2 * np.pi * (0.8 * x - 0.5 * y) / 0.9 + 0.5)
    b = 120 + 50 * np.sin(2 * np.pi * (0.6 * x + 0.9 * y) / 1.1 + 1.3)
    return np.clip(np.rint(np.stack([r, g, b], 1)), 0, 255).astype(np.uint8)


def fixture():
    """(scans: nine (11200, 3) fp32 clouds in the sensor frame, colours: nine (11200, 4) uint8, truth: nine 4x4 poses)."""
    rng = np.random.default_rng(20)
    scans, cols, truth = [], [], []
    for k in range(N_SCANS):
        a, b = np.meshgrid(np.linspace(-0.6, 0.6, GRID[0]), np.linspace(-0.35, 0.35, GRID[1]))
        a = a.reshape(-1) + rng.uniform(-0.002, 0.002, a.size); b = b.reshape(-1) + rng.uniform(-0.002, 0.002, b.size)
        z = WALL_Z + rng.normal(0.0, 0.002, a.size)
        p = np.stack([np.tan(a) * z, np.tan(b) * z, z], 1)
        T = np.eye(4, dtype=f32); T[0, 3] = STEP_M * k
        rgb = texture(p[:, 0] + STEP_M * k, p[:, 1])
        scans.append(p.astype(f32)); cols.append(np.ascontiguousarray(np.concatenate([rgb, np.full((len(p), 1), 255, np.uint8)], 1))); truth.append(T)
    return scans, cols, truth


def translation_errors(poses, truth):
    return [float(np.linalg.norm(np.asarray(P, np.float64)[:3, 3] - np.asarray(T, np.float64)[:3, 3])) for P, T in zip(poses, truth)]


def new_volume(hashed=False):
    import sdf_cloud_restatement as SC
    import tsdf_cloud_color_restatement as CC
    return CC.add_color(SC.HVolume(**OPTS) if hashed else SC.Volume(DIMS, **OPTS))


def restatement_tracks():
    """(the photometric loop's (poses, records, infos, status, n_colored), the geometric loop's, truth), both on the CPU, dense."""
    import sdf_cloud_color_restatement as R
    import tsdf_cloud_color_restatement as CC
    scans, cols, truth = fixture()
    eye = np.eye(4, dtype=f32)
    colored = R.track(new_volume(), scans, cols, eye, weight=COLOR_OPTIONS["weight"], color_huber=COLOR_OPTIONS["huber"], **OPTIONS)
    geometric = CC.track(new_volume(), scans, cols, eye, **OPTIONS)
    return colored, geometric, truth


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    colored, geometric, truth = restatement_tracks()
    ec, eg = translation_errors(colored[0], truth), translation_errors(geometric[0], truth)
    out = dict(colored_worst_translation_m=max(ec), colored_last_translation_m=ec[-1], geometric_worst_translation_m=max(eg),
               geometric_last_translation_m=eg[-1], lateral_travel_m=TRAVEL, scans=N_SCANS, points_per_scan=GRID[0] * GRID[1],
               n_iterations=OPTIONS["n_iterations"], weight=COLOR_OPTIONS["weight"], colored_statuses=sorted(set(r["status"] for r in colored[1])),
               colored_iterations=[r["iterations"] for r in colored[1]], geometric_iterations=[r["iterations"] for r in geometric[1]])
    print(json.dumps(out))
    print("photometric loop per scan:", " ".join("%.4f" % e for e in ec))
    print("geometric loop per scan:", " ".join("%.4f" % e for e in eg))
    assert 2 * max(ec) < TRAVEL / 2 < eg[-1], "the fixture does not separate the two trackers"
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
