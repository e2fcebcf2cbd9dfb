"""Laser scans into the TSDF volume on the device (icp_tsdf_integrate_cloud) against the numpy restatement of the
contract (tests/tsdf_cloud_restatement.py), bit for bit: crafted clouds around every branch of the walk, the hashed volume against the
dense one, the order of the points and repeated calls, the composition with depth frames, evict and insert and a coloured volume, the
outcome on twelve synthetic scans with the mesh behind it, and the refusals."""
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_restatement as HR
import tsdf_cloud_outcome_fixture as CF
import tsdf_cloud_restatement as CR
from support import same_bits, pose_of, tsdf_blocks_equal_restatement as assert_equals_restatement, fuse_cloud as fuse
from tsdf_cloud_cases import cloud, OPTS, DYADIC

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE = 1, 3, 4
ODD = dict(OPTS, truncation=0.22)                   # 2 truncation / s = 4.4: the last sample is the fminf clamp
TILTED = pose_of((0.12, -0.2, 0.07), (0.1, -0.05, 0.02))
EYE = np.eye(4, dtype=f32)


def far_pose():
    T = TILTED.copy(); T[0, 3] = f32(2.0e6)
    return T


E = (0.05, -0.02, 0.1)
CASES = {
    # name: (options, cloud, pose, sensor origin, block capacity)
    "single": (OPTS, cloud(1), TILTED, None, 64),
    "n63": (OPTS, cloud(63), TILTED, None, 64),
    "n64": (OPTS, cloud(64), TILTED, None, 64),
    "n65": (OPTS, cloud(65), TILTED, None, 64),
    "n257": (OPTS, cloud(257), TILTED, None, 64),
    "n3000": (OPTS, cloud(3000), TILTED, None, 1 << 10),
    # +x from a voxel centre, everything dyadic: r = 8.5 voxels, truncation 3 voxels, so every sample lands on a .5 tie of floorf(. + 0.5f)
    "ties": (DYADIC, np.array([[2.125, 0, 0], [0, 1.625, 0], [0, 0, -1.375]], f32), EYE, None, 64),
    # the surface at the world origin, the ray along the diagonal: blocks -1 and 0 on all three axes
    "across_zero": (dict(OPTS, origin=(0.0, 0.0, 0.0)), np.array([[0.3, 0.3, 0.3], [0.31, 0.28, 0.33]], f32), pose_of((0, 0, 0), (-0.3, -0.3, -0.3)), None, 64),
    "nearer_than_truncation": (OPTS, np.array([[0.05, 0.0, 0.2], [0.0, 0.1, 0.0], [1e-3, 0, 0]], f32), TILTED, None, 64),
    "clamped_last_sample": (ODD, cloud(200, seed=6), TILTED, None, 64),
    "at_the_sensor_centre": (OPTS, np.array([E, [0.3, 0.2, 1.5], E], f32), TILTED, E, 64),
    "nan_and_inf": (OPTS, np.concatenate([np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], f32), cloud(70, seed=8)]), TILTED, None, 64),
    "beyond_max_depth": (OPTS, np.array([[0, 0, 6.5], [0, 0, 5.5], [4.0, 4.0, 4.0], [0, 6.0, 0]], f32), EYE, None, 64),
    "sensor_origin_tilted": (OPTS, cloud(300, seed=5), TILTED, E, 64),
    "beyond_the_range": (OPTS, cloud(100, seed=7), far_pose(), None, 64),
    "growth_from_one_block": (OPTS, cloud(1000, seed=11), TILTED, None, 1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_restatement(gpu_ctx_factory, name):
    """Block coordinates, tsdf, weight and every field of the info, bit for bit."""
    opts, pts, pose, origin, capacity = CASES[name]
    ctx = gpu_ctx_factory()
    ctx.tsdf_create_hashed(block_capacity=capacity, **opts)
    hv = HR.HVolume(**opts)
    info = fuse(ctx, hv, pts, pose, origin)
    binfo = assert_equals_restatement(ctx, hv, name)
    if name == "beyond_the_range":
        assert info["n_blocks"] == 0 and info["n_updated"] == 0 and info["n_samples"] == 0 and info["n_outside"] > 500 and info["n_rays"] == 100
        assert binfo["n_out_of_range"] == info["n_outside"]
    else:
        assert info["n_updated"] > 0 and info["n_outside"] == 0 and info["n_blocks"] > 0
    if name == "growth_from_one_block":
        assert binfo["n_grown"] >= 5 and binfo["capacity"] >= info["n_blocks"] > 32
    if name == "ties":
        assert info["n_rays"] == 3 and info["n_samples"] == 3 * 7          # M = 6, every sample a voxel of its own
    if name == "across_zero":
        b = np.array(sorted(hv.blocks))
        assert (b.min(0) == -1).all() and (b.max(0) == 0).all()
    if name == "nearer_than_truncation":
        assert info["n_samples"] < 3 * 7                                    # some t_m <= 0
    if name == "at_the_sensor_centre":
        assert info["n_points"] == 3 and info["n_rays"] == 1
    if name == "nan_and_inf":
        assert info["n_points"] == 74 and info["n_rays"] == 70
    if name == "beyond_max_depth":
        assert info["n_rays"] == 2                                          # 5.5 and exactly 6.0; 6.5 and 6.93 are not usable


def test_hashed_equals_dense(gpu_ctx_factory):
    """After tsdf_allocate_blocks over a box, three scans fused into the hashed volume and into a dense one with the same origin are equal
    voxel for voxel; the dense call equals the dense restatement, and n_outside is what leaves the box."""
    from icp_amd import binding
    opts = dict(OPTS, origin=(-1.8, -1.8, -0.5))
    dims = (48, 48, 48)
    h, d = gpu_ctx_factory(), gpu_ctx_factory()
    h.tsdf_create_hashed(block_capacity=64, **opts)
    box = HC.box_coords((0, 0, 0), (6, 6, 6))
    h.tsdf_allocate_blocks(box)
    d.tsdf_create(dims=dims, **opts)
    hv = HR.HVolume(**opts); hv.allocate(box); dv = CR.DVolume(dims, **opts)
    poses = [EYE, TILTED, pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05))]
    dense_infos = []
    for k, pose in enumerate(poses):
        pts = cloud(1500, seed=20 + k)
        ih, idn = fuse(h, hv, pts, pose), fuse(d, dv, pts, pose)
        dense_infos.append(idn)
        assert ih["n_outside"] == 0 < idn["n_outside"] and idn["n_blocks"] == 0 and 0 < idn["n_updated"] < ih["n_updated"]
    _, coords, t, w = h.tsdf_blocks()
    T, Wt = binding.tsdf_blocks_to_dense(coords, t, w, (0, 0, 0), dims)
    Td, Wd = d.tsdf_volume()
    assert same_bits(T, Td) and same_bits(Wt, Wd) and Wd.max() == 3
    assert same_bits(Td, dv.tsdf) and same_bits(Wd, dv.weight)
    assert_equals_restatement(h, hv, "hashed")
    # eth.fuse_scans on a dense box is the same three calls
    from icp_amd import eth
    infos = eth.fuse_scans(d, [cloud(1500, seed=20 + k) for k in range(3)], poses, voxel_size=opts["voxel_size"], truncation=opts["truncation"], origin=opts["origin"],
                           max_range=opts["max_depth"], hashed=False, dims=dims)
    Te, We = d.tsdf_volume()
    assert same_bits(Te, Td) and same_bits(We, Wd) and infos == dense_infos


def test_order_and_repetition(gpu_ctx_factory):
    """The same cloud reversed and shuffled gives identical blocks; a second integrate equals the restatement's second fold; and a depth
    frame integrated after a cloud, then a cloud again, still equals the restatement -- the accumulators were left zero."""
    ctx = gpu_ctx_factory()
    pts = cloud(3000, seed=31)
    perm = np.random.default_rng(5).permutation(len(pts))
    got = []
    for p in (pts, pts[::-1].copy(), pts[perm]):
        ctx.tsdf_create_hashed(block_capacity=1 << 10, **OPTS)
        ctx.set_source(p)
        infos = [ctx.tsdf_integrate_cloud("source", pose=TILTED) for _ in range(2)]
        got.append((infos, ctx.tsdf_blocks()[1:]))
    for infos, blocks in got[1:]:
        assert infos == got[0][0]
        assert all(same_bits(a, b) for a, b in zip(blocks, got[0][1])) and np.array_equal(blocks[0], got[0][1][0])
    hv = HR.HVolume(**OPTS)
    want = [CR.integrate(hv, pts, TILTED) for _ in range(2)]
    assert got[0][0] == want and want[1]["n_blocks"] == want[0]["n_blocks"]
    assert_equals_restatement(ctx, hv, "second fold")
    assert got[0][1][2].max() == 2
    # depth frames and clouds in turn, on STRADDLE's volume (max_depth 2.4 cuts some of the cloud's rays)
    cam, rcam = HC.camera()
    ctx.tsdf_create_hashed(**HC.STRADDLE)
    hv = HR.HVolume(**HC.STRADDLE)
    near = (cloud(2000, seed=32) * f32(0.7)).astype(f32)
    i0 = fuse(ctx, hv, near, HC.TILTED)
    assert 0 < i0["n_rays"] < i0["n_points"]
    assert ctx.tsdf_integrate(HC.crafted_frame(), cam, HC.TILTED) == HR.integrate(hv, HC.crafted_frame(), rcam, HC.TILTED)
    assert_equals_restatement(ctx, hv, "frame after cloud")
    fuse(ctx, hv, near[::-1].copy(), HC.POSES[2])
    assert ctx.tsdf_integrate(HC.frames()[1], cam, EYE) == HR.integrate(hv, HC.frames()[1], rcam, EYE)
    fuse(ctx, hv, near, EYE)
    assert_equals_restatement(ctx, hv, "cloud after frame after cloud")
    # the target works as the source does
    ctx.set_target(near)
    info = ctx.tsdf_integrate_cloud("target", pose=HC.TILTED)
    assert info == CR.integrate(hv, near, HC.TILTED)
    assert_equals_restatement(ctx, hv, "target")


def test_after_evict_and_insert(gpu_ctx_factory):
    """A cloud fused after an evict and an insert (the pool compacted, then refilled) equals the same integrate on a fresh volume
    uploaded with the same blocks, and the restatement."""
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    first, second = cloud(2000, seed=41), cloud(2000, seed=42)
    a.tsdf_create_hashed(block_capacity=16, **OPTS)
    hv = HR.HVolume(**OPTS)
    fuse(a, hv, first, TILTED)
    centre = (0.0, 0.0, 2.0)
    einfo, ec, et, ew = a.tsdf_evict_blocks(centre, 1.5)
    print("evict: %s" % einfo)
    assert 0 < einfo["n_evicted"] < len(hv.blocks)
    a.tsdf_insert_blocks(ec, et, ew)
    _, coords, t, w = a.tsdf_blocks()
    b.tsdf_create_hashed(block_capacity=1 << 10, **OPTS)
    b.tsdf_upload_blocks(coords, t, w)
    ia = fuse(a, hv, second, pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05)))
    b.set_source(second)
    ib = b.tsdf_integrate_cloud("source", pose=pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05)))
    assert ia == ib
    ba, bb = a.tsdf_blocks()[1:], b.tsdf_blocks()[1:]
    assert np.array_equal(ba[0], bb[0]) and same_bits(ba[1], bb[1]) and same_bits(ba[2], bb[2]) and ba[2].max() == 2
    assert_equals_restatement(a, hv, "after evict and insert")


def test_colours_stay_as_they_are(gpu_ctx_factory):
    """On a coloured hashed volume the call writes geometry only: the colours of the blocks that existed are bit for bit unchanged, the
    blocks the cloud adds are uncoloured."""
    ctx = gpu_ctx_factory()
    cam, _ = HC.camera()
    ctx.tsdf_create_hashed(color=True, **HC.STRADDLE)
    rgbx = np.random.default_rng(3).integers(0, 256, (HC.H, HC.W, 4), dtype=np.uint8)
    n, nc = ctx.tsdf_integrate(HC.crafted_frame(), cam, HC.TILTED, rgbx=rgbx)
    assert nc > 0
    _, c0, t0, w0, rgb0, cw0 = ctx.tsdf_blocks(colors=True)
    near = (cloud(2000, seed=32) * f32(0.7)).astype(f32)
    ctx.set_source(near)
    info = ctx.tsdf_integrate_cloud("source", pose=HC.POSES[2])
    _, c1, t1, w1, rgb1, cw1 = ctx.tsdf_blocks(colors=True)
    assert info["n_updated"] > 0 and len(c1) > len(c0) and not same_bits(w1.sum(), w0.sum())
    key = lambda c: (c[:, 2].astype(np.int64) << 42) + (c[:, 1].astype(np.int64) << 21) + c[:, 0]
    at = np.searchsorted(key(c1), key(c0))
    assert np.array_equal(c1[at], c0)
    assert same_bits(rgb1[at], rgb0) and same_bits(cw1[at], cw0) and cw0.max() > 0
    new = np.ones(len(c1), bool); new[at] = False
    assert not rgb1[new].any() and not cw1[new].any()


def test_outcome_mesh_and_reconstruct(gpu_ctx_factory, tmp_path):
    """Twelve synthetic scans fused at their true poses with eth.fuse_scans: the blocks equal the fixture's restatement exactly (which is
    a surface: asserted on the CPU there), tsdf_mesh_hashed returns a mesh, and eth.reconstruct writes a PLY that reads back identically."""
    from icp_amd import eth, meshio
    clouds, poses, normals = CF.scans()
    vol, want = CF.model()
    CF.assert_surface(vol)
    ctx = gpu_ctx_factory()
    infos = eth.fuse_scans(ctx, clouds, poses, voxel_size=CF.VOXEL, truncation=CF.TRUNCATION, origin=CF.ORIGIN, max_range=CF.MAX_RANGE, block_capacity=256)
    assert infos == want
    assert_equals_restatement(ctx, vol, "outcome")
    F, _, valid = ctx.tsdf_sample(CF.held_out_points())
    rF, _, rvalid = HR.sample(vol, CF.held_out_points())
    assert np.array_equal(valid, rvalid) and same_bits(F, rF)
    v, nr, t = ctx.tsdf_mesh_hashed()
    print("mesh: %d vertices, %d triangles from %d blocks" % (len(v), len(t), infos[-1]["n_blocks"]))
    assert len(v) > 1000 and len(t) > 1000 and np.isfinite(v).all() and int(t.max()) < len(v)
    # the whole chain: tracked against the voxel map, fused at the tracked poses, meshed, written
    ctx.set_gicp_options(1e-3, 0)
    path = str(tmp_path / "room.ply")
    tposes, recs, status, mesh = eth.reconstruct(ctx, list(zip(clouds, normals)), poses[0], tsdf_voxel_size=CF.VOXEL, truncation=CF.TRUNCATION, mesh_path=path,
                                                 voxel_size=0.25, hashed=True, n_iterations=30, min_valid=64)
    assert len(tposes) == CF.N_SCANS and len(recs) == CF.N_SCANS - 1 and len(mesh[0]) > 1000 and len(mesh[2]) > 1000
    back = meshio.load_ply_mesh(path)
    assert all(same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(mesh, back))
    print("reconstruct: status %d, %d vertices, %d triangles" % (status, len(mesh[0]), len(mesh[2])))


def test_refusals_leave_the_volume_as_it_was(gpu_ctx_factory):
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    lib = ctx.lib
    p = binding.pose_to_c(TILTED)
    call = lambda which, pose, e=None: lib.icp_tsdf_integrate_cloud(ctx.h, which, binding._ptr(pose), binding._ptr(e), None)
    msg = lambda: lib.icp_last_error(ctx.h).decode()
    ctx.set_source(cloud(50))
    assert call(1, p) == ERR_INVALID_ARG and "icp_tsdf_integrate_cloud" in msg() and "no volume" in msg()
    fresh = gpu_ctx_factory()
    fresh.tsdf_create_hashed(block_capacity=8, **OPTS)
    assert lib.icp_tsdf_integrate_cloud(fresh.h, 1, binding._ptr(p), None, None) == ERR_NO_SOURCE
    assert lib.icp_tsdf_integrate_cloud(fresh.h, 0, binding._ptr(p), None, None) == ERR_NO_TARGET
    assert "icp_tsdf_integrate_cloud" in lib.icp_last_error(fresh.h).decode() and fresh.tsdf_blocks()[0]["n_blocks"] == 0
    for hashed in (True, False):
        if hashed:
            ctx.tsdf_create_hashed(**OPTS)
        else:
            ctx.tsdf_create(dims=(40, 40, 40), **dict(OPTS, origin=(-1.8, -1.8, 0.0)))
        assert ctx.tsdf_integrate_cloud("source", pose=TILTED)["n_updated"] > 0
        state = lambda: ctx.tsdf_blocks() if hashed else ctx.tsdf_volume()
        before = state()
        bad = p.copy(); bad[13] = np.nan
        inf = p.copy(); inf[0] = np.inf
        assert call(1, bad) == ERR_INVALID_ARG and "pose" in msg() and call(1, inf) == ERR_INVALID_ARG
        assert call(2, p) == ERR_INVALID_ARG and call(-1, p) == ERR_INVALID_ARG and "which" in msg()
        assert call(1, None) == ERR_INVALID_ARG
        assert call(1, p, np.array([0, np.nan, 0], f32)) == ERR_INVALID_ARG and "sensor origin" in msg()
        assert call(0, p) == ERR_NO_TARGET and "icp_tsdf_integrate_cloud" in msg()
        after = state()
        if hashed:
            assert before[0] == after[0] and np.array_equal(before[1], after[1]) and same_bits(before[2], after[2]) and same_bits(before[3], after[3])
        else:
            assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    # a hashed volume that may not grow: refused, the blocks it had are all still there and nothing is written
    assert lib.icp_debug_htsdf_max_blocks(fresh.h, 3) == 0
    fresh.set_source(cloud(1, seed=2))
    assert 0 < fresh.tsdf_integrate_cloud("source", pose=TILTED)["n_blocks"] <= 8
    before = fresh.tsdf_blocks()
    fresh.set_source(cloud(500))
    assert lib.icp_tsdf_integrate_cloud(fresh.h, 1, binding._ptr(p), None, None) == ERR_INVALID_ARG
    assert "icp_tsdf_integrate_cloud" in lib.icp_last_error(fresh.h).decode() and "blocks" in lib.icp_last_error(fresh.h).decode()
    after = fresh.tsdf_blocks()
    assert before[0]["n_blocks"] == after[0]["n_blocks"] and np.array_equal(before[1], after[1]) and same_bits(before[2], after[2]) and same_bits(before[3], after[3])
    assert lib.icp_debug_htsdf_max_blocks(fresh.h, 22) == 0
    assert fresh.tsdf_integrate_cloud("source", pose=TILTED)["n_blocks"] > 8
