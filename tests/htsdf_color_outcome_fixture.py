"""The outcome fixture of direct SDF tracking with the photometric term on the HASHED coloured volume (tests/test_gpu_htsdf_color.py,
DESIGN.md section 6zb): the textured wall of tests/tsdf_color_outcome_fixture.py -- 12 frames of 160 x 120, the camera sliding 1 cm per
frame along a flat wall whose geometry leaves the lateral pose free -- tracked at stride 2 with 20 iterations, the default stops, weight
0.1 and the colour Huber off, on a hashed volume with that fixture's origin, voxel size and truncation.  Run as a script (CPU only) it
tracks the frames twice with the numpy restatements, once coloured (htsdf_color_restatement.track) and once with htsdf_restatement alone,
asserts that the fixture separates the two and writes tests/golden/htsdf_color_outcome.json: the reference the device's bound is twice
of.  The hashed model observes no free space outside the band, so the figures need not be the dense fixture's: they come from this run."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "htsdf_color_outcome.json")
OPTIONS = dict(stride=2, n_iterations=20)
COLOR_OPTIONS = dict(weight=0.1, huber=0.0)


def hashed_model(color=True):
    """tum.track's model dict: the textured wall's volume without its extent, hashed (coloured or not)."""
    import tsdf_color_outcome_fixture as CF
    m = {k: v for k, v in CF.VOLUME.items() if k != "dims"}
    return dict(m, hashed=True, color=True) if color else dict(m, hashed=True)


def restatement_tracks():
    """(poses, records and block counts of the coloured loop, the same of the geometric loop, gt), both on the CPU."""
    import htsdf_color_restatement as HCR
    import htsdf_restatement as HR
    import tsdf_restatement as TS
    import tsdf_color_outcome_fixture as CF
    K, depth, rgbx, gt = CF.fixture()
    cam = TS.Camera(K, CF.W, CF.H)
    eye = np.eye(4, dtype=np.float32)
    opts = {k: v for k, v in CF.VOLUME.items() if k != "dims"}
    colored = HCR.track(HCR.add_color(HR.HVolume(**opts)), depth, rgbx, cam, eye, weight=COLOR_OPTIONS["weight"], color_huber=COLOR_OPTIONS["huber"], **OPTIONS)
    geometric = HR.track(HR.HVolume(**opts), depth, cam, eye, **OPTIONS)
    return colored, geometric, gt


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import tsdf_color_outcome_fixture as CF
    (poses_c, recs_c, nb_c), (poses_g, recs_g, nb_g), gt = restatement_tracks()
    ec, eg = CF.translation_errors(poses_c, gt), CF.translation_errors(poses_g, gt)
    travel = CF.STEP_M * (CF.N_FRAMES - 1)
    out = dict(colored_worst_translation_m=max(ec), colored_last_translation_m=ec[-1], geometric_worst_translation_m=max(eg),
               geometric_last_translation_m=eg[-1], lateral_travel_m=travel, frames=CF.N_FRAMES, width=CF.W, height=CF.H,
               stride=OPTIONS["stride"], n_iterations=OPTIONS["n_iterations"], weight=COLOR_OPTIONS["weight"],
               colored_statuses=sorted(set(r["status"] for r in recs_c)), colored_iterations=[r["iterations"] for r in recs_c],
               geometric_iterations=[r["iterations"] for r in recs_g], colored_n_blocks=nb_c, geometric_n_blocks=nb_g)
    print(json.dumps(out))
    print("coloured loop per frame:", " ".join("%.4f" % e for e in ec))
    print("geometric loop per frame:", " ".join("%.4f" % e for e in eg))
    assert 2 * max(ec) < travel / 2 < eg[-1], "the fixture does not separate the two trackers"
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
