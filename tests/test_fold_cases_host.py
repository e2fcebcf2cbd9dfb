"""What tests/test_gpu_fold_sizes.py rests on, checked without a device: the inputs of tests/fold_cases.py give the block counts they
claim under the host's own formulas, and in every one of them a block that the fold of k_sdf_solve / k_sdf_solve_color dropped or added
twice could not hide -- every block holds a usable and a valid element (and, with colours, a coloured one), so the exact counts move, and
every block's share of the cost sum (index 27) exceeds the bound n 2^-52 sum |term| that the device test grants that sum.  These are
conditions on the inputs: one that fails needs other holes, not another factor."""
import os
import re

import numpy as np
import pytest

import fold_cases as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def source(name):
    with open(os.path.join(ROOT, "icp-variants_amd", "csrc", name)) as f:
        return f.read()


def test_poses_are_the_neighbours():
    import test_gpu_sdf
    import test_gpu_vgicp
    assert F.SDF_NEAR == test_gpu_sdf.NEAR and F.VG_NEAR == test_gpu_vgicp.NEAR and F.VG_EPS == test_gpu_vgicp.EPS


def test_block_counts_under_the_hosts_own_formulas():
    """sdf_plan (host_sdf.hpp) and vgicp_plan (host_vgicp.hpp) as they are written, evaluated on the shapes of fold_cases: the table of
    SDF_CASES and VG_CASES is keyed by the result.  The colour kind takes sdf_plan's grid: host_sdf.hpp's driver plans for both kinds."""
    plan = source("host_sdf.hpp")
    assert "f.ws = (cam.width + opt.stride - 1) / opt.stride; f.hs = (cam.height + opt.stride - 1) / opt.stride;" in plan
    assert "pl->grid = dim3((f.ws + 15) / 16, (f.hs + 15) / 16);" in plan and "pl->n_blocks = (int)(pl->grid.x * pl->grid.y);" in plan
    # the colour kind has no plan of its own: every coloured call goes through the shared driver, which plans with sdf_plan for either kind
    color = source("host_sdf_color.hpp")
    assert "if ((rc = sdf_plan<K>(c, cam, opt, pl))) return rc;" in plan and "if ((rc = sdf_plan<K>(c, cam, opt, &pl))) return rc;" in plan
    assert "pl->grid" not in color and "n_blocks" not in color and "sdf_plan" not in color
    assert all(call in color for call in ("sdf_system<SdfColor>(", "sdf_align<SdfColor>(", "sdf_track<SdfColor>(", "sdf_time<SdfColor>("))
    for blocks, (w, h, stride) in F.SDF_CASES.items():
        ws, hs = (w + stride - 1) // stride, (h + stride - 1) // stride
        assert ((ws + 15) // 16) * ((hs + 15) // 16) == blocks == F.sdf_blocks(w, h, stride), (blocks, w, h, stride)
    assert F.sdf_blocks(1280, 16, 1) == 80 and F.SDF_CASES[16] == (1280, 16, 5)            # the stride's case: not the frame's 80 blocks
    per_lane = int(re.search(r"constexpr int VG_POINTS_PER_LANE = (\d+);", source("dev_vgicp.hpp")).group(1))
    assert "pl->n_blocks = (s.n + 256 * VG_POINTS_PER_LANE - 1) / (256 * VG_POINTS_PER_LANE);" in source("host_vgicp.hpp")
    assert per_lane * 256 == F.VG_BLOCK
    for blocks, n in F.VG_CASES.items():
        assert (n + 256 * per_lane - 1) // (256 * per_lane) == blocks, (blocks, n)
    # the edges of the fold: 64 lanes, four blocks per lane and round trip (sums), eight (counts)
    fold = source("dev_sdf.hpp")
    assert "b0 += 4 * WAVE" in fold and "b0 += 8 * WAVE" in fold and "b0 += 4 * WAVE" in source("dev_sdf_color.hpp") and "b0 += 8 * WAVE" in source("dev_sdf_color.hpp")
    for edge in (64, 256, 512):
        assert edge in F.SDF_CASES and edge + 1 in F.SDF_CASES and edge in F.VG_CASES and edge + 1 in F.VG_CASES
    assert len(F.CASES) == len(F.SDF_CASES) + len(F.COLOR_BLOCKS) + len(F.VG_CASES)
    assert 1200 in F.SDF_CASES and F.SDF_CASES[1200] == (640, 480, 1) and set(F.COLOR_BLOCKS) <= set(F.SDF_CASES)


@pytest.mark.parametrize("blocks", sorted(F.SDF_CASES))
def test_sdf_premises(blocks):
    c = F.sdf_case(blocks)
    w, h, stride = F.SDF_CASES[blocks]
    sampled = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
    assert c["depth"].shape == (h, w) and np.isfinite(c["cast"]).all()                     # the volume is observed everywhere: no frame has a hole of its own
    d = c["depth"][::stride, ::stride]
    assert (d == F.MINF).any() and np.isnan(d).any() and (d == 2.5).any() and (d > c["cast"][::stride, ::stride]).sum() > (d == 2.5).sum()
    p = F.premises(("sdf", blocks))
    margin = F.check_premises(p, blocks, sampled)
    if blocks in F.OUTLIER_BLOCKS:                                                         # the Huber bound changes weights, in every block
        assert (p["share"][0.05] < p["share"][0.0]).all()
    print("SDF %4d blocks (%d x %d, stride %d): n_depth %d, n_valid %d of %d; per block at least %d usable, %d valid; smallest share of sum 27 / bound = %.3g"
          % (blocks, w, h, stride, p["counts"][0], p["counts"][1], sampled, p["usable"].min(), p["valid"].min(), margin))
    assert set(p["share"]) == set(F.hubers(blocks))
    if blocks in F.COLOR_BLOCKS:
        p = F.premises(("sdf_color", blocks))
        margin = F.check_premises(p, blocks, sampled, color=True)
        print("     coloured: n_depth %d, n_valid %d, n_color %d; per block at least %d coloured; smallest share of sum 27 / bound = %.3g"
              % (p["counts"] + (p["colored"].min(), margin)))


@pytest.mark.parametrize("blocks", sorted(F.VG_CASES))
def test_vgicp_premises(blocks):
    pts, nrm = F.vg_source(blocks)
    n = F.VG_CASES[blocks]
    assert len(pts) == n and np.isnan(pts[::97]).all(1).sum() >= (n - 1) // 97 and (nrm[5::89] == 0).all(1).sum() >= (n - 6) // 89
    p = F.premises(("vgicp", blocks))
    margin = F.check_premises(p, blocks, n)
    assert p["last_valid"] and set(p["share"]) == set(F.min_points(blocks))
    if n % F.VG_BLOCK == 1:                                                                # the last point is alone in its block, and counts
        assert p["usable"][-1] == 1 and all(v[-1] == 1 for v in p["valid"].values())
    print("VGICP %3d blocks (%d points): counts %s; per block at least %s valid; smallest share of sum 27 / bound = %.3g"
          % (blocks, n, p["counts"], {k: int(v.min()) for k, v in p["valid"].items()}, margin))
    g = F.vg_target()[2]
    assert g["n_points"] == F.VG_TARGET_POINTS and g["voxel_size"] == np.float32(F.VG_VOXEL)


def test_check_premises_refuses_what_it_should():
    """An empty block, a block without a valid element, a share below the bound and a wrong block count each fail."""
    p = F.premises(("sdf", 6))
    F.check_premises(p, 6, 1200)
    for broken in (dict(p, usable=p["usable"] * np.array([1, 1, 0, 1, 1, 1])), dict(p, valid=p["valid"] * np.array([1, 1, 1, 1, 0, 1])),
                   dict(p, share={0.0: p["share"][0.0] * np.array([1, 1e-14, 1, 1, 1, 1])}), dict(p, n_blocks=5), dict(p, counts=(1200, p["counts"][1])),
                   dict(p, counts=(p["counts"][0], p["counts"][0]))):
        with pytest.raises(AssertionError):
            F.check_premises(broken, 6, 1200)
