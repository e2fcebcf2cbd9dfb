"""icp_tsdf_integrate_cloud on the device at the edges of its shapes, ranges and accumulators: the cases of
tests/tsdf_cloud_cases.py (tests/test_tsdf_cloud_cases_host.py shows without a device that each one reaches its edge) against the numpy
restatement of the contract, bit for bit and field by field, with no tolerance.

  DENSE_SHAPES    non-cubic boxes around k_tsdf_fold_cloud's 64 x 4 x 16 tile, axes of length 1, two poses
  DENSE_FACES     samples on the floorf(x + 0.5f) tie at every face of the box, an edge, a corner, sdf == -truncation
  RANGE_STRADDLE  n_samples > 0 and n_outside > 0 in one call at the hashed volume's +- 2^23 voxels
  PILE_UP         N = 2^17 + 1 on six addresses, S beyond 32 bits and below zero; both orders of the points
  SATURATION      max_weight 1.0 and 2.5 over four fuses
  LANES           the touch's rule about the lane to the left, at block capacity 64 and 1; both orders of the points
  BAND            M = 1 and M = 20
  the scratch     one context through dense, dense of the same voxel count, hashed that grows, dense with a depth frame in between"""
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_restatement as HR
import tsdf_cloud_cases as TC
import tsdf_cloud_restatement as CR
import tsdf_restatement as TS
from support import same_bits, tsdf_blocks_equal_restatement as assert_equals_restatement, fuse_cloud as fuse

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    """One context for every case: each volume replaces the one before, dense and hashed in turn, and the accumulators follow."""
    return gpu_ctx_factory()


def create(ctx, opts, dims, capacity):
    if dims is None:
        ctx.tsdf_create_hashed(block_capacity=capacity, **opts)
    else:
        ctx.tsdf_create(dims=dims, **opts)


def device_state(ctx, dims):
    """What the volume holds: (coords, tsdf, weight) of the blocks, or (tsdf, weight) of the box."""
    return ctx.tsdf_blocks()[1:] if dims is None else ctx.tsdf_volume()


def run_case(ctx, table, name, reverse=False, which="source"):
    """The case's steps fused on the device into a fresh volume: every info equal to the restatement's, field by field.  reverse: the
    points of every step in the opposite order.  -> the device's state"""
    reason, steps = TC.TABLES[table][name]
    want, vol = TC.reference(table, name)
    create(ctx, *[steps[0][j] for j in (0, 1, 5)])
    for k, (_, dims, pts, pose, origin, _) in enumerate(steps):
        pts = pts[::-1].copy() if reverse else pts
        (ctx.set_source if which == "source" else ctx.set_target)(pts)
        info = ctx.tsdf_integrate_cloud(which, pose=pose, sensor_origin=origin)
        print("%s %s step %d%s: %s" % (table, name, k, " reversed" if reverse else "", info))
        for field in CR.INFO:
            assert info[field] == want[k][field], (name, k, field, info, want[k])
        assert sorted(info) == sorted(CR.INFO)
    dims = steps[0][1]
    if dims is None:
        assert_equals_restatement(ctx, vol, name)
    else:
        T, W = ctx.tsdf_volume()
        assert same_bits(T, vol.tsdf) and same_bits(W, vol.weight), name
    return device_state(ctx, dims)


def assert_same_state(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if x.dtype != np.float32 else same_bits(x, y), what


@pytest.mark.parametrize("name", list(TC.DENSE_SHAPES))
def test_dense_shapes(ctx, name):
    T, W = run_case(ctx, "DENSE_SHAPES", name, which="target" if name == TC.AS_TARGET else "source")
    assert W.max() == 2 and W.shape == TC.DENSE_SHAPES[name][1][0][1][::-1]


def test_an_axis_of_length_one_is_refused(ctx):
    """icp_tsdf_options asks for every extent >= 2: no box is thinner than DENSE_SHAPES' thinnest.  The refusal leaves the volume, and what
    the next cloud makes of it, as they were."""
    from icp_amd import binding
    opts, dims, pts, pose, _, _ = TC.DENSE_SHAPES["40x33x2"][1][0]
    ctx.tsdf_create(dims=dims, **opts)
    for bad in TC.REFUSED:
        with pytest.raises(binding.IcpError, match="dimension"):
            ctx.tsdf_create(dims=bad, **opts)
    ctx.set_source(pts)
    assert ctx.tsdf_integrate_cloud("source", pose=pose) == TC.reference("DENSE_SHAPES", "40x33x2")[0][0]


@pytest.mark.parametrize("name", list(TC.DENSE_FACES))
def test_dense_faces(ctx, name):
    run_case(ctx, "DENSE_FACES", name)


@pytest.mark.parametrize("name", list(TC.RANGE_STRADDLE))
def test_range_straddle(ctx, name):
    run_case(ctx, "RANGE_STRADDLE", name)
    info = ctx.tsdf_blocks()[0]
    assert info["n_blocks"] >= 2 and info["n_out_of_range"] > 0


@pytest.mark.parametrize("name", list(TC.PILE_UP))
def test_pile_up(ctx, name):
    forward = run_case(ctx, "PILE_UP", name)
    assert_same_state(run_case(ctx, "PILE_UP", name, reverse=True), forward, name)


@pytest.mark.parametrize("name", list(TC.SATURATION))
def test_saturation(ctx, name):
    state = run_case(ctx, "SATURATION", name)
    assert state[-1].max() == TC.SAT_WEIGHTS[TC.SATURATION[name][1][0][0]["max_weight"]][-1]


@pytest.mark.parametrize("name", list(TC.LANES))
def test_lanes(ctx, name):
    forward = run_case(ctx, "LANES", name)
    assert_same_state(run_case(ctx, "LANES", name, reverse=True), forward, name)
    if name.endswith("capacity_1"):
        assert ctx.tsdf_blocks()[0]["n_grown"] >= 1


@pytest.mark.parametrize("name", list(TC.BAND))
def test_band(ctx, name):
    run_case(ctx, "BAND", name)


def test_the_scratch_follows_the_volume(gpu_ctx_factory):
    """One context, the volume re-created again and again, a fuse compared with a restatement carried along behind every step: a dense box,
    one of the same voxel count with x and z exchanged, a hashed volume of one block that grows between two calls, a dense box again, and
    a depth frame between two clouds on it."""
    ctx = gpu_ctx_factory()
    wall = TC.cloud(3000, seed=91)

    def dense_equal(dv, what):
        T, W = ctx.tsdf_volume()
        assert same_bits(T, dv.tsdf) and same_bits(W, dv.weight), what

    for dims in ((8, 4, 2), (2, 4, 8)):
        opts = dict(TC.OPTS, origin=(-0.05 * dims[0], -0.05 * dims[1], 2.0 - 0.05 * dims[2]))
        ctx.tsdf_create(dims=dims, **opts)
        dv = CR.DVolume(dims, **opts)
        for pose in (TC.EYE, TC.TILTED):
            info = fuse(ctx, dv, wall, pose)
            assert info["n_updated"] > 0 and info["n_outside"] > 0
            dense_equal(dv, dims)
        assert dv.weight.max() == 2
    ctx.tsdf_create_hashed(block_capacity=1, **TC.OPTS)
    hv = HR.HVolume(**TC.OPTS)
    assert fuse(ctx, hv, TC.cloud(1, seed=92), TC.TILTED)["n_blocks"] >= 1
    small = assert_equals_restatement(ctx, hv, "one point")
    assert fuse(ctx, hv, TC.cloud(1000, seed=93), TC.TILTED)["n_blocks"] > 32
    large = assert_equals_restatement(ctx, hv, "the pool has grown")
    assert large["capacity"] > small["capacity"] and large["n_grown"] > small["n_grown"]
    fuse(ctx, hv, wall, TC.EYE)
    assert_equals_restatement(ctx, hv, "after the growth")
    # dense again, now BOX's 48^3 (max_depth 2.4 cuts some of the rays), with a depth frame between two clouds
    cam, rcam = HC.camera()
    ctx.tsdf_create(dims=HC.BOX_DIMS, **HC.BOX)
    dv = CR.DVolume(HC.BOX_DIMS, **HC.BOX)
    near = (TC.cloud(2000, seed=94) * f32(0.7)).astype(f32)
    i0 = fuse(ctx, dv, near, HC.TILTED)
    assert 0 < i0["n_rays"] < i0["n_points"] and i0["n_updated"] > 0
    dense_equal(dv, "cloud")
    tv = TS.Volume(HC.BOX_DIMS, **HC.BOX)
    tv.tsdf, tv.weight = dv.tsdf, dv.weight
    n = TS.integrate(tv, HC.crafted_frame(), rcam, HC.TILTED)
    assert ctx.tsdf_integrate(HC.crafted_frame(), cam, HC.TILTED) == n > 0
    dv.tsdf, dv.weight = tv.tsdf, tv.weight
    dense_equal(dv, "frame after cloud")
    fuse(ctx, dv, near[::-1].copy(), HC.POSES[2])
    dense_equal(dv, "cloud after frame after cloud")
    assert dv.weight.max() == 3
