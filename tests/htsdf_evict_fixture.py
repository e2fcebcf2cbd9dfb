"""The fixture of the local (streaming) tracking loop on the hashed TSDF volume (tests/test_htsdf_evict_host.py, tests/test_gpu_htsdf_evict.py,
DESIGN.md section 6za): a camera that slides along a wavy wall for N_OUT steps and back again, at 48 x 36 pixels, with a small max_depth so
that the view's reach is a few blocks and keep_radius = reach + twice the step.  Chosen on the restatement alone.  Run as a script (CPU
only) it tracks the sequence with tests/htsdf_evict_restatement.py, locally and unbounded, and writes what the device has to meet to
tests/golden/htsdf_evict_outcome.json: per frame the evicted, inserted and resident counts, the peak, the total, and how far the nearest
block centre stays from the sphere (the counts are those of a device run as long as its poses differ from these by less)."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "htsdf_evict_outcome.json")
W, H = 48, 36
N_OUT = 20
STEP = 0.25
VOLUME = dict(origin=(0.0125, -0.0375, 0.6125), voxel_size=0.05, truncation=0.2, max_weight=64.0, min_depth=0.2, max_depth=1.3)
OPTIONS = dict(stride=1, n_iterations=15)
f32 = np.float32


def wall(x, y):
    return 1.0 + 0.07 * np.sin(2.6 * x) + 0.05 * np.cos(3.1 * y + 0.4 * x) + 0.04 * np.sin(7.0 * x + 1.0)


def positions():
    out = [k * STEP for k in range(N_OUT + 1)]
    return out + out[-2::-1]


def frames():
    """(K, depth (n, H, W) float32, camera-to-world poses): identity rotation, the camera at (x_k, 0, 0) looking along +z at the wall."""
    from icp_amd.synth import tum_K
    K = tum_K(W)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    a = (u - float(K[0, 2])) / float(K[0, 0]); b = (v - float(K[1, 2])) / float(K[1, 1])
    depth, poses = [], []
    for x0 in positions():
        z = np.ones_like(a)
        for _ in range(60):                            # the ray's depth is a fixed point of z = wall(x0 + a z, b z): a contraction here
            z = wall(x0 + a * z, b * z)
        depth.append(z.astype(f32))
        T = np.eye(4, dtype=f32); T[0, 3] = f32(x0)
        poses.append(T)
    return K, np.stack(depth), poses


def keep_radius(cam, vol):
    import htsdf_evict_restatement as ER
    return float(f32(ER.view_reach(cam, vol) + 2.0 * STEP))


def model():
    """tum.track's model dict."""
    import htsdf_restatement as HR
    import tsdf_restatement as TS
    from icp_amd.synth import tum_K
    m = dict(VOLUME, hashed=True)
    m["keep_radius"] = keep_radius(TS.Camera(tum_K(W), W, H), HR.HVolume(**VOLUME))
    return m


def restatement_runs():
    import htsdf_restatement as HR
    import htsdf_evict_restatement as ER
    import tsdf_restatement as TS
    K, depth, gt = frames()
    cam = TS.Camera(K, W, H)
    eye = np.eye(4, dtype=f32)
    full = HR.HVolume(**VOLUME)
    fposes, frecs, fblocks = HR.track(full, depth, cam, eye, **OPTIONS)
    loc = HR.HVolume(**VOLUME)
    r = keep_radius(cam, loc)
    lposes, lrecs, evs, store = ER.track_local(loc, depth, cam, eye, r, **OPTIONS)
    return dict(full=full, fposes=fposes, frecs=frecs, fblocks=fblocks, loc=loc, lposes=lposes, lrecs=lrecs, evs=evs, store=store, keep_radius=r, gt=gt, cam=cam)


def margin(run):
    """The smallest | |block centre - t_k| - keep_radius | over the frames and over every block of the finished model, in metres."""
    vol = run["full"]
    b = np.array(sorted(vol.blocks), np.int64)
    p = vol.o.astype(np.float64) + ((8 * b) + 3.5) * float(vol.s)
    best = np.inf
    for T in run["lposes"]:
        d = np.linalg.norm(p - T[:3, 3].astype(np.float64), axis=1)
        best = min(best, float(np.abs(d - run["keep_radius"]).min()))
    return best


def outcome(run):
    evs = run["evs"]
    err = [float(np.abs(p[:3, 3] - g[:3, 3]).max()) for p, g in zip(run["lposes"], run["gt"])]
    steps = [float(np.linalg.norm(a[:3, 3].astype(np.float64) - b[:3, 3])) for a, b in zip(run["lposes"][1:], run["lposes"][:-1])]
    return dict(frames=len(evs), width=W, height=H, step=STEP, keep_radius=run["keep_radius"], stride=OPTIONS["stride"], n_iterations=OPTIONS["n_iterations"],
                n_evicted=[e["n_evicted"] for e in evs], n_inserted=[e["n_inserted"] for e in evs], n_resident=[e["n_resident"] for e in evs],
                n_stored=[e["n_stored"] for e in evs], peak_resident=max(e["n_resident"] + e["n_evicted"] for e in evs),
                total_blocks=len(run["full"].blocks), statuses=sorted(set(r["status"] for r in run["lrecs"])),
                worst_translation_error_m=max(err), largest_step_m=max(steps), margin_m=margin(run))


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    out = outcome(restatement_runs())
    print(json.dumps(out))
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
