"""The fold of k_sdf_solve and k_sdf_solve_color over more than a handful of blocks.  Direct SDF tracking, its photometric variant and
voxelized GICP end an iteration alike: every block of the accumulate kernel writes a column of partials[28 or 29][n_blocks] and of
counts[2 or 3][n_blocks], and one block folds the columns -- per lane the blocks lane, lane + 64, lane + 128, lane + 192 in one round trip,
then 256 further (the sums); eight blocks per round trip, then 512 further (the counts).  tests/test_gpu_sdf.py, test_gpu_sdf_color.py and
test_gpu_vgicp.py reach 20 blocks; here the block counts of tests/fold_cases.py sit on both sides of 64, 256 and 512 and at the workload's
1200 (640 x 480 at stride 1), against the restatements, with the bounds those tests use, unchanged.  tests/test_fold_cases_host.py shows
without a device that in each of these inputs one block dropped or added twice moves the counts and moves sum 27 by more than its bound.

Measured (MI355X), worst |sum - restatement| / bound: 1.4e-3 at 6 and 16 blocks, at most 7e-5 from 64 blocks on (SDF 7e-5, coloured 3e-5,
VGICP 4.1e-5; 7.6e-6 at 1200 blocks); every step's pose is the restatement's to the bit; every call on the shared buffer gives a fresh
context's bits."""
import functools

import numpy as np
import pytest

import fold_cases as F
import sdf_color_restatement as SC
import sdf_restatement as SR
import support as S
import vgicp_restatement as VR
from support import same_bits

pytestmark = pytest.mark.gpu
STEPS = 3


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def sdf_ctx(factory, color):
    """A fresh context holding fold_cases' volume (with its colour array when color)."""
    vol = F.sdf_volume(color)
    ctx = factory()
    ctx.tsdf_create(color=color, **F.VOLUME)
    ctx.tsdf_upload(vol.tsdf, vol.weight)
    if color:
        ctx.tsdf_color_upload(vol.rgb, vol.wc)
    return ctx


def vg_ctx(factory, ctx=None):
    ctx = factory() if ctx is None else ctx
    ctx.set_gicp_options(F.VG_EPS, 0)
    ctx.set_target(*F.vg_target()[:2], None)
    return ctx


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    """One context for the comparisons against the restatement: the coloured volume and the VGICP target."""
    return vg_ctx(gpu_ctx_factory, sdf_ctx(gpu_ctx_factory, True))


def camera(c):
    from icp_amd import binding
    return binding.depth_camera(c["K"], c["width"], c["height"])


# the device calls, as the one-buffer test repeats them
def sdf_call(ctx, blocks, huber=0.0):
    c = F.sdf_case(blocks)
    return ctx.tsdf_sdf_system(c["depth"], camera(c), F.sdf_pose(), stride=c["stride"], huber=huber)


def color_call(ctx, blocks):
    c = F.sdf_case(blocks)
    return ctx.tsdf_sdf_system(c["depth"], camera(c), F.sdf_pose(), rgbx=c["rgbx"], stride=c["stride"], color_weight=F.COLOR_WEIGHT)


def vg_call(ctx, blocks, mp=1):
    ctx.set_source(*F.vg_source(blocks), None)
    return ctx.vgicp_system(F.vg_pose(), voxel_size=F.VG_VOXEL, min_points=mp)


# the restatement's side, computed once
@functools.lru_cache(maxsize=None)
def sdf_reference(blocks, huber):
    c = F.sdf_case(blocks)
    return SR.system(F.sdf_volume(), c["depth"], F.rcam_of(c), F.sdf_pose(), stride=c["stride"], huber=huber)


@functools.lru_cache(maxsize=None)
def vg_reference(blocks, mp):
    return VR.system(F.vg_target()[2], *F.vg_source(blocks), F.vg_pose(), F.VG_EPS, mp)


def compare(what, blocks, got, again, ref, n_terms):
    """Counts exactly; every sum within n 2^-52 sum |term| of the restatement's; a second call the same bits."""
    (sums, counts), (sums2, counts2), (rcounts, rsums, rabs) = got, again, ref
    bound = n_terms * 2.0 ** -52 * rabs
    err = np.abs(sums - rsums)
    print("%s, %d blocks: counts %s, worst |sum - restatement| / bound = %.3g" % (what, blocks, tuple(counts), (err / np.maximum(bound, 1e-300)).max()))
    assert sums.shape == rsums.shape and tuple(counts) == tuple(rcounts), (what, blocks, counts, rcounts)
    assert (bound > 0).all() and (err <= bound).all(), (what, blocks, err, bound)
    assert np.array_equal(u64(sums), u64(sums2)) and tuple(counts2) == tuple(counts), (what, blocks)


@pytest.mark.parametrize("blocks", sorted(F.SDF_CASES))
def test_sdf_sums(ctx, blocks):
    """icp_tsdf_sdf_system against SR.system on every frame of fold_cases.SDF_CASES: the Huber bound 0, and 0.05 too at 257 and 1200 blocks."""
    for huber in F.hubers(blocks):
        ref = sdf_reference(blocks, huber)
        assert F.SDF_CASES[blocks][0] * F.SDF_CASES[blocks][1] > ref[0][0] > ref[0][1] > 0
        compare("SDF sums %s huber %g" % (F.SDF_CASES[blocks], huber), blocks, sdf_call(ctx, blocks, huber), sdf_call(ctx, blocks, huber), ref, ref[0][1])
    if blocks in F.OUTLIER_BLOCKS:
        assert sdf_reference(blocks, 0.05)[1][27] < 0.9 * sdf_reference(blocks, 0.0)[1][27]        # the Huber bound changes weights there


@pytest.mark.parametrize("blocks", F.COLOR_BLOCKS)
def test_colored_sums(ctx, blocks):
    """icp_tsdf_sdf_system_color against SC.system: three counts, 29 sums -- the 29th, which only wave 0 of the fold owns, like the rest --
    within (n_valid + n_color) 2^-52 sum(|geometric term| + |photometric term|), tests/test_gpu_sdf_color.py's bound."""
    c = F.sdf_case(blocks)
    ref = SC.system(F.sdf_volume(True), c["depth"], c["rgbx"], F.rcam_of(c), F.sdf_pose(), stride=c["stride"], weight=F.COLOR_WEIGHT)
    assert ref[0][0] > ref[0][1] > ref[0][2] > 0 and 0 < ref[1][28] < ref[1][27] and ref[1].shape == (29,)
    compare("coloured sums %s" % (F.SDF_CASES[blocks],), blocks, color_call(ctx, blocks), color_call(ctx, blocks), ref, ref[0][1] + ref[0][2])


@pytest.mark.parametrize("blocks", sorted(F.VG_CASES))
def test_vgicp_sums(ctx, blocks):
    """icp_vgicp_system against VR.system on every source of fold_cases.VG_CASES: min_points 1, and 3 too at 257 blocks."""
    for mp in F.min_points(blocks):
        ref = vg_reference(blocks, mp)
        assert F.VG_CASES[blocks] > ref[0][0] > ref[0][1] > 0
        compare("VGICP sums %d points min_points %d" % (F.VG_CASES[blocks], mp), blocks, vg_call(ctx, blocks, mp), vg_call(ctx, blocks, mp), ref, ref[0][1])
    if len(F.min_points(blocks)) > 1:
        assert vg_reference(blocks, 3)[0][1] < vg_reference(blocks, 1)[0][1]


def follow(what, blocks, start, rec, rc, trace, system):
    """Every iteration's pose within S.POSE_TOL of the restatement's step from the DEVICE's previous pose, n_valid exactly, the cost within
    the summation bound; the record's counts are the trace's."""
    assert rc == 0 and rec["status"] == 0 and rec["iterations"] == STEPS and len(trace) == STEPS
    prev = start
    n_depth = None
    for i, t in enumerate(trace):
        counts, sums, sabs = system(prev)
        want, _ = SR.step(sums, counts, prev)
        diff = float(np.abs(t["pose"] - want).max())
        bound = counts[1] * 2.0 ** -52 * sabs[27]
        print("%s, %d blocks, step %d: n_depth %d, n_valid %d, cost %.6g, |cost - restatement| / bound = %.3g, |pose - restatement| = %.3g"
              % (what, blocks, i, counts[0], t["n_valid"], t["cost"], abs(t["cost"] - sums[27]) / bound, diff))
        assert t["status"] == 0 and t["n_valid"] == counts[1], (what, i, t["n_valid"], counts)
        assert diff <= S.POSE_TOL, (what, i, diff)
        assert abs(t["cost"] - sums[27]) <= bound, (what, i)
        n_depth = counts[0] if n_depth is None else n_depth
        prev = t["pose"]
    assert same_bits(rec["pose"], trace[-1]["pose"])
    assert (rec["n_depth"], rec["n_valid_first"], rec["n_valid_last"]) == (n_depth, trace[0]["n_valid"], trace[-1]["n_valid"])
    assert u64(rec["cost_first"]) == u64(trace[0]["cost"]) and u64(rec["cost_last"]) == u64(trace[-1]["cost"])


@pytest.mark.parametrize("blocks", [257, 1200])
def test_sdf_steps(ctx, blocks):
    """icp_tsdf_align_depth, 3 iterations, the stops off, traced: the fold with step = 1 and the pose solve on sums of this size."""
    c = F.sdf_case(blocks)
    start = F.sdf_pose()
    pose, rec, rc, trace = ctx.tsdf_align_depth(c["depth"], camera(c), start, trace=True, stride=c["stride"], n_iterations=STEPS, stop_rotation=0.0, stop_translation=0.0)
    follow("SDF steps", blocks, start, rec, rc, trace, lambda p: SR.system(F.sdf_volume(), c["depth"], F.rcam_of(c), p, stride=c["stride"]))
    assert same_bits(pose, rec["pose"])


def test_vgicp_steps(ctx):
    """icp_vgicp_align at 257 blocks, 3 iterations, the stops off, traced."""
    blocks = 257
    src, nrm = F.vg_source(blocks)
    ctx.set_source(src, nrm, None)
    start = F.vg_pose()
    pose, rec, rc, trace = ctx.vgicp_align(start, trace=True, voxel_size=F.VG_VOXEL, n_iterations=STEPS, stop_rotation=0.0, stop_translation=0.0)
    follow("VGICP steps", blocks, start, rec, rc, trace, lambda p: VR.system(F.vg_target()[2], src, nrm, p, F.VG_EPS))
    assert same_bits(pose, rec["pose"])


def test_one_buffer_many_sizes(gpu_ctx_factory):
    """The sums and the counts share one allocation (sdf_partials) whose split depends on n_blocks and whose size only grows.  On ONE context,
    in this order: the 6-block SDF system, the 1200-block one, the 257-block coloured one (29 rows, 3 count rows), the 513-block VGICP one,
    the 6-block SDF system again -- each bit for bit what a fresh context gives for that call alone.  A stale column or a stale offset
    would show here and nowhere else."""
    calls = [("SDF", 6, sdf_call), ("SDF", 1200, sdf_call), ("coloured", 257, color_call), ("VGICP", 513, vg_call), ("SDF", 6, sdf_call)]
    alone = {}
    for what, blocks, call in calls:
        if (what, blocks) not in alone:
            fresh = vg_ctx(gpu_ctx_factory) if what == "VGICP" else sdf_ctx(gpu_ctx_factory, what == "coloured")
            alone[(what, blocks)] = call(fresh, blocks)
    one = vg_ctx(gpu_ctx_factory, sdf_ctx(gpu_ctx_factory, True))
    for what, blocks, call in calls:
        sums, counts = call(one, blocks)
        want, wcounts = alone[(what, blocks)]
        print("one buffer: %s, %d blocks: counts %s, %d of %d sums bit-equal to a fresh context's" % (what, blocks, tuple(counts), (u64(sums) == u64(want)).sum(), len(want)))
        assert tuple(counts) == tuple(wcounts) and np.array_equal(u64(sums), u64(want)), (what, blocks)
    assert alone[("SDF", 1200)][1] == sdf_reference(1200, 0.0)[0] and alone[("SDF", 6)][1] == sdf_reference(6, 0.0)[0]
