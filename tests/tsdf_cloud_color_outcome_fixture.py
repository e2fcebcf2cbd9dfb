"""The outcome fixture of coloured laser scans fused into the coloured hashed TSDF volume (tests/test_gpu_tsdf_cloud_color.py, DESIGN.md
section 6zh): the twelve scans of tsdf_cloud_outcome_fixture.scans(), which are not modified, with the colours synth.laser_scan returns
beside them, fused at their true poses by the numpy restatement (tests/tsdf_cloud_color_restatement.py) at that fixture's options.  The
device equals the restatement bit for bit, so the GPU test compares its blocks with model()'s exactly; what makes the model worth
comparing with is asserted here, on the CPU, at the noise-free points of held-out scan 12, each looked up in its nearest voxel:
  at least MIN_COLOURED_SHARE of the points find a coloured voxel, and
  the median over those points of the largest per-channel error is at most MAX_ERROR_RATIO times the same median for a model painted
  with the volume's one mean colour."""
import functools
import numpy as np

import tsdf_cloud_outcome_fixture as CF

f32 = np.float32
MIN_COLOURED_SHARE, MAX_ERROR_RATIO = 0.9, 0.7


@functools.lru_cache(maxsize=None)
def colours():
    """One rgba (n, 4) uint8 array per scan of CF.scans(): the third return of the synth.laser_scan call that made the scan."""
    from icp_amd import synth
    out = []
    for k in range(CF.N_SCANS):
        out.append(np.ascontiguousarray(synth.laser_scan(synth.scan_pose(k), 0xE7A0 + k, n_tilt=CF.N_TILT, n_beam=CF.N_BEAM)[2]))
    return out


@functools.lru_cache(maxsize=None)
def held_out():
    """(the noise-free points of scan HELD_OUT in the world frame, their true colours (n, 3) as float64)."""
    from icp_amd import synth
    pts, _, rgba = synth.laser_scan(synth.scan_pose(CF.HELD_OUT), 0, n_tilt=CF.N_TILT, n_beam=CF.N_BEAM, sigma=0.0)
    return pts, rgba[:, :3].astype(np.float64)


@functools.lru_cache(maxsize=None)
def model():
    """(the restatement's coloured HVolume after the N_SCANS scans, per scan (info, carve stats, n_colored)).  Shared: do not modify."""
    import htsdf_restatement as HR
    import tsdf_cloud_color_restatement as KR
    clouds, poses, _ = CF.scans()
    vol = KR.add_color(HR.HVolume(**CF.options()))
    out = [KR.integrate(vol, c, rgba, T) for c, rgba, T in zip(clouds, colours(), poses)]
    return vol, out


def colour_figures(vol):
    """(share of the held-out points whose nearest voxel is coloured, median over those of the largest per-channel error, the same median
    for a model painted with the mean colour of the volume's coloured voxels), on a 0 .. 255 scale."""
    pts, true = held_out()
    g = np.floor((pts.astype(np.float64) - vol.o.astype(np.float64)) / float(vol.s) + 0.5).astype(np.int64)
    C = np.zeros((len(g), 3), np.float64); W = np.zeros(len(g), np.float64)
    for i, v in enumerate(g):
        b = tuple(int(x) for x in v >> 3)
        if b in vol.colors:
            rgb, wc = vol.colors[b]
            l = v & 7
            C[i] = rgb[l[2], l[1], l[0]]; W[i] = wc[l[2], l[1], l[0]]
    ok = W > 0
    allc = np.concatenate([rgb[wc > 0] for rgb, wc in vol.colors.values()]).astype(np.float64)
    mean = allc.mean(0)
    err = np.abs(C[ok] - true[ok]).max(1)
    base = np.abs(mean[None] - true[ok]).max(1)
    return float(ok.mean()), float(np.median(err)), float(np.median(base))


def assert_colours(vol):
    share, median, baseline = colour_figures(vol)
    print("held-out scan: %.1f %% of %d points find a coloured voxel, median largest channel error %.1f, mean-colour baseline %.1f (ratio %.3f)"
          % (100 * share, len(held_out()[0]), median, baseline, median / baseline))
    assert share >= MIN_COLOURED_SHARE, share
    assert median <= MAX_ERROR_RATIO * baseline, (median, baseline)
    return share, median, baseline


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__)); root = os.path.abspath(os.path.join(here, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    vol, out = model()
    print("%d blocks, last scan %s" % (len(vol.blocks), out[-1]))
    print("updated and not coloured per scan: %s" % [o[0]["n_updated"] - o[2] for o in out])
    assert_colours(vol)
