"""icp_tsdf_mesh on the device against the numpy restatement of its contract (tests/tsdf_mesh_restatement.py), bit for bit: uploaded analytic
volumes, a fused volume with every kind of voxel, the calling contract, and the mesh of the model through tum.reconstruct_room."""
import ctypes as C
import os
import numpy as np
import pytest

import tsdf_restatement as TS
import tsdf_mesh_restatement as TM
from icp_amd.synth import tum_K
from support import bits, upload

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG = 1


def check_against_restatement(ctx, vol, min_weight, what):
    """The device's mesh of the resident volume == the restatement's of `vol`: counts, vertex and normal bits, triangle arrays."""
    v, n, t = ctx.tsdf_mesh(min_weight)
    rv, rn, rt = TM.mesh(vol, min_weight)
    print("%s: V %d, T %d (restatement %d, %d)" % (what, len(v), len(t), len(rv), len(rt)))
    assert (len(v), len(t)) == (len(rv), len(rt)), what
    assert t.dtype == np.uint32 and np.array_equal(t, rt), what
    assert np.array_equal(bits(v), bits(rv)), what
    assert np.array_equal(bits(n), bits(rn)), what
    return v, n, t


SMALL = dict(dims=(37, 21, 29), s=0.05, origin=(-0.9, -0.5, -0.7))      # no multiple of a 64-voxel run, of nx or of a 1024-voxel block
CENTRE = (0.013, -0.021, 0.034)


@pytest.mark.parametrize("shape", ["sphere", "torus", "sphere_with_holes"])
def test_uploaded_volume_bit_for_bit(gpu_ctx_factory, shape):
    """37 x 21 x 29 = 22533 voxels: 353 runs of 64 (the last one partial), 23 blocks of 1024 voxels, rows of 37 that no run lines up with."""
    fn = TM.torus(CENTRE, 0.3, 0.12) if shape == "torus" else TM.sphere(CENTRE, 0.4)
    vol = TM.analytic_volume(fn, **SMALL)
    if shape == "sphere_with_holes":
        rng = np.random.default_rng(11)
        vol.weight[:, 9, :] = 0                                  # a slab of unobserved voxels
        vol.weight[rng.random(vol.weight.shape) < 0.02] = 0      # scattered ones
        vol.tsdf[rng.random(vol.tsdf.shape) < 0.01] = np.nan     # non-finite values of every kind
        vol.tsdf[5, 10, 12] = np.inf; vol.tsdf[20, 8, 30] = -np.inf
        vol.tsdf[14, 3:8, 4:30] = 0.0                            # exact zeros next to the surface
    ctx = gpu_ctx_factory()
    upload(ctx, vol)
    v, n, t = check_against_restatement(ctx, vol, 0.0, shape)
    assert len(t) > 1000
    if shape != "sphere_with_holes":
        uc, twice = TM.edge_counts(t)
        assert (uc == 2).all() and twice == 0 and len(v) - len(uc) + len(t) == (0 if shape == "torus" else 2)
    else:
        assert np.isfinite(v).all() and np.isfinite(n).all()


def test_many_blocks_bit_for_bit(gpu_ctx_factory):
    """70 x 66 x 230 = 1 062 600 voxels.  A block covers 1024 voxels (TM_BLOCK_VOXELS), so the count tables have 1038 entries: more than the
    1024 the scan takes at a time, and its carry runs.  (The 70 x 66 x 61 volume of 256-voxel blocks, with one axis scaled.)"""
    dims = (70, 66, 230)
    assert (dims[0] * dims[1] * dims[2] + 1023) // 1024 == 1038
    vol = TM.analytic_volume(TM.sphere((0.0113, -0.0207, 0.031), 0.6), dims=dims, s=0.02, origin=(-0.69, -0.65, -2.29))
    vol.tsdf[:, :, :] = np.where(vol.tsdf > 0.08, f32(1.0), vol.tsdf)     # (a truncated field far from the surface, as a fused volume has)
    far = TM.analytic_volume(TM.sphere((0.05, 0.02, 2.2), 0.35), dims=dims, s=0.02, origin=(-0.69, -0.65, -2.29))
    vol.tsdf = np.minimum(vol.tsdf, far.tsdf).astype(f32)                 # a second sphere cut by the last layers: blocks 1024.., behind the carry
    vol.weight[100:103] = 0
    ctx = gpu_ctx_factory()
    upload(ctx, vol)
    v, n, t = check_against_restatement(ctx, vol, 0.0, "1038 blocks")
    own_block = (np.floor((v[:, 2] - vol.o[2]) / vol.s).astype(np.int64) * 66 * 70) // 1024
    assert own_block.min() < 1024 < own_block.max()                      # vertices on both sides of the scan's chunk boundary


def fused_volume(ctx):
    """The volume and frames of test_gpu_tsdf.py::test_integrate_matches_restatement_bit_for_bit: a crafted start (arbitrary values, weights in
    {0, 1, 1.5}, NaNs with a payload), a depth frame with holes, NaN, inf and a step, two poses, max_weight 2.  Fused on the device and in
    the restatement; returns the restatement's volume."""
    from icp_amd import binding, synth
    W, H = 40, 30
    K = tum_K(W)
    cam, rcam = binding.depth_camera(K, W, H), TS.Camera(K, W, H)
    opts = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=2.0, min_depth=0.3, max_depth=2.4)
    ctx.tsdf_create(**opts)
    vol = TS.Volume(**opts)
    rng = np.random.default_rng(3)
    shape = (29, 21, 37)
    t0 = rng.uniform(-1, 1, shape).astype(f32); w0 = rng.choice(np.array([0, 1, 1.5], f32), shape)
    marked = np.zeros(shape, bool); marked[:3] = True
    t0.view(np.uint32)[marked] = 0x7FC12345; w0.view(np.uint32)[marked] = 0xFFC54321
    ctx.tsdf_upload(t0, w0)
    vol.tsdf, vol.weight = t0.copy(), w0.copy()

    def wavy(base):
        u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        return (base + 0.3 * np.sin(u * 0.3) + 0.2 * np.cos(v * 0.4) + 0.5 * (u > 0.7 * W)).astype(f32)
    d1 = wavy(1.5)
    d1[0, :6] = [MINF, np.nan, np.inf, 0.0, -1.0, 2.5]
    d1[10:14, 20:24] = MINF
    d2 = wavy(1.4); d2[5, 5] = np.nan
    poses = [np.eye(4, dtype=f32), synth.make_pose((0.1, -0.25, 0.05), (0.3, -0.1, 0.2)).astype(f32)]
    for depth, pose in [(d1, poses[0]), (d2, poses[1]), (d1, poses[0]), (d1, poses[0])]:
        assert ctx.tsdf_integrate(depth, cam, pose) == TS.integrate(vol, depth, rcam, pose)
    return vol


def test_fused_volume_bit_for_bit(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    vol = fused_volume(ctx)
    t_before, w_before = ctx.tsdf_volume()
    assert np.array_equal(bits(t_before), bits(vol.tsdf)) and np.array_equal(bits(w_before), bits(vol.weight))
    counts = []
    for mw in (0.0, 1.5):
        v, n, t = check_against_restatement(ctx, vol, mw, "fused volume, min_weight %g" % mw)
        assert len(v) > 0 and len(t) > 0
        counts.append((len(v), len(t)))
        v2, n2, t2 = ctx.tsdf_mesh(mw)                                   # a second call: identical arrays
        assert np.array_equal(bits(v), bits(v2)) and np.array_equal(bits(n), bits(n2)) and np.array_equal(t, t2)
        t_after, w_after = ctx.tsdf_volume()
        assert np.array_equal(bits(t_after), bits(t_before)) and np.array_equal(bits(w_after), bits(w_before))
    assert counts[0][0] != counts[1][0] and counts[0][1] != counts[1][1]


def raw_mesh(ctx, min_weight, max_v, max_t, v, n, t):
    nv, nt = C.c_int32(-7), C.c_int32(-7)
    from icp_amd import binding
    rc = ctx.lib.icp_tsdf_mesh(ctx.h, C.c_float(min_weight), C.c_int32(max_v), C.c_int32(max_t), binding._ptr(v), binding._ptr(n), binding._ptr(t), C.byref(nv), C.byref(nt))
    return rc, nv.value, nt.value


def test_calling_contract(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    msg = lambda: ctx.lib.icp_last_error(ctx.h).decode()
    # no volume
    rc, nv, nt = raw_mesh(ctx, 0.0, 0, 0, None, None, None)
    assert rc == ERR_INVALID_ARG and "no volume" in msg() and (nv, nt) == (0, 0)
    vol = TM.analytic_volume(TM.sphere(CENTRE, 0.4), **SMALL)
    upload(ctx, vol)
    rv, rn, rt = TM.mesh(vol)
    V, T = len(rv), len(rt)
    # a bad min_weight
    for bad in (float("nan"), -1.0, float("inf")):
        rc, nv, nt = raw_mesh(ctx, bad, 0, 0, None, None, None)
        assert rc == ERR_INVALID_ARG and "min_weight" in msg()
    # count only
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None) == (0, V, T)
    # a capacity one too small on either side: the counts, a message with both, untouched arrays
    for max_v, max_t in ((V - 1, T), (V, T - 1)):
        v = np.full((V, 3), 7.5, f32); n = np.full((V, 3), 7.5, f32); t = np.full((T, 3), 0xABCDEF01, np.uint32)
        assert raw_mesh(ctx, 0.0, max_v, max_t, v, n, t) == (ERR_INVALID_ARG, V, T)
        assert str(V) in msg() and str(T) in msg()
        assert (v == 7.5).all() and (n == 7.5).all() and (t == 0xABCDEF01).all()
    # exact capacities, with and without normals
    v = np.full((V, 3), 7.5, f32); n = np.full((V, 3), 7.5, f32); t = np.zeros((T, 3), np.uint32)
    assert raw_mesh(ctx, 0.0, V, T, v, n, t) == (0, V, T)
    assert np.array_equal(bits(v), bits(rv)) and np.array_equal(bits(n), bits(rn)) and np.array_equal(t, rt)
    v2 = np.zeros((V + 5, 3), f32); t2 = np.zeros((T + 5, 3), np.uint32)
    assert raw_mesh(ctx, 0.0, V + 5, T + 5, v2, None, t2) == (0, V, T)
    assert np.array_equal(bits(v2[:V]), bits(rv)) and np.array_equal(t2[:T], rt) and not v2[V:].any() and not t2[T:].any()
    # vertices and triangles go together
    assert raw_mesh(ctx, 0.0, V, T, v, n, None)[0] == ERR_INVALID_ARG and raw_mesh(ctx, 0.0, V, T, None, None, t)[0] == ERR_INVALID_ARG
    # nothing observed: an empty mesh
    ctx.tsdf_reset()
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None) == (0, 0, 0)
    assert raw_mesh(ctx, 0.0, V, T, v, n, t) == (0, 0, 0)
    ev, en, et = ctx.tsdf_mesh()
    assert ev.shape == (0, 3) and en.shape == (0, 3) and et.shape == (0, 3)
    # the volume released: refused again
    ctx.tsdf_release()
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None)[0] == ERR_INVALID_ARG


def test_context_left_alone(gpu_ctx_factory):
    """icp_run on a resident pair gives identical records before and after icp_tsdf_mesh; params and the convergence measure do not change."""
    from icp_amd import binding, synth
    W, H = 160, 120
    K = tum_K(W)
    T = [synth.camera_pose(k) for k in range(2)]
    depth = [synth.depth_frame(Tk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05)[0][:, 2].reshape(H, W).copy() for k, Tk in enumerate(T)]
    cam = binding.depth_camera(K, W, H)
    ctx = gpu_ctx_factory()
    p = ctx.params; p.metric = 1; p.knn_backend = 1; p.n_iterations = 10; p.max_distance = 0.1
    ctx.push_params()
    ctx.set_target_depth(depth[0], None, cam, binding.depth_options(False, 1))
    ctx.set_source_depth(depth[1], None, cam, binding.depth_options(False, 4))
    src = np.ones((64, 3), f32)
    ctx.set_convergence_reference(src, src)
    ctx.tsdf_create(dims=(71, 35, 89), origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
    ctx.tsdf_integrate(depth[0], cam, np.eye(4, dtype=f32))
    before = binding.IcpParams(); ctx.lib.icp_get_params(ctx.h, C.byref(before))
    pose_a, recs_a, _ = ctx.run(np.eye(4))
    rmse_a = ctx.rmse(pose_a)
    v, n, t = ctx.tsdf_mesh()
    assert len(t) > 100
    after = binding.IcpParams(); ctx.lib.icp_get_params(ctx.h, C.byref(after))
    assert bytes(before) == bytes(after)
    pose_b, recs_b, _ = ctx.run(np.eye(4))
    assert np.array_equal(pose_a.view(np.uint32), pose_b.view(np.uint32)) and len(recs_a) == len(recs_b) > 0
    for a, b in zip(recs_a, recs_b):
        assert set(a) == set(b)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    assert f32(ctx.rmse(pose_b)) == f32(rmse_a)


def test_model_mesh_through_reconstruct_room(tmp_path, gpu_ctx_factory):
    pytest.importorskip("PIL")
    from icp_amd import binding, meshio, tum
    W, H = 80, 60
    K = tum_K(W)
    d = str(tmp_path / "seq")
    tum.write_synthetic_sequence(d, 3, width=W, height=H, K=K)
    seq = tum.load_sequence(d, frame_step=1, K=K)
    assert seq["frames"] == [0, 1, 2] and seq["width"] == W
    model = dict(dims=(71, 35, 89), origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)

    def params():
        p = binding.default_params(); p.metric = 1; p.knn_backend = 1
        return p
    out = str(tmp_path / "out")
    ctx = gpu_ctx_factory()
    poses, recs, rc, paths = tum.reconstruct_room(ctx, seq, params(), out_dir=out, model=model, model_mesh="model.ply")
    assert sorted(os.listdir(out)) == ["mesh_0.off", "mesh_1.off", "mesh_2.off", "model.ply"] and len(paths) == 3
    v, n, t = meshio.load_ply_mesh(os.path.join(out, "model.ply"))
    dv, dn, dt = ctx.tsdf_mesh()
    assert len(dt) > 100
    assert np.array_equal(bits(v), bits(dv)) and np.array_equal(bits(n), bits(dn)) and np.array_equal(t, dt)
    # without model_mesh: the directory listing of before, and the same tracking
    out2 = str(tmp_path / "out2")
    poses2, recs2, rc2, paths2 = tum.reconstruct_room(gpu_ctx_factory(), seq, params(), out_dir=out2, model=model)
    assert sorted(os.listdir(out2)) == ["mesh_0.off", "mesh_1.off", "mesh_2.off"] and rc2 == rc
    for a, b in zip(poses, poses2):
        assert np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))
    # a file name without a model or without out_dir writes nothing
    out3 = str(tmp_path / "out3")
    tum.reconstruct_room(gpu_ctx_factory(), seq, params(), out_dir=out3, model_mesh="model.ply")
    assert sorted(os.listdir(out3)) == ["mesh_0.off", "mesh_1.off", "mesh_2.off"]
