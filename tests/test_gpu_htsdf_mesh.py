"""icp_tsdf_mesh_hashed on the device: against the numpy restatement of its contract (tests/htsdf_mesh_restatement.py) bit for bit, order
included; against icp_tsdf_mesh on the dense volume over the blocks' bounding box as a multiset of triangles; independence of where the
blocks sit in the pool; the calling contract; the volume left as it was; the mesh of a hashed model through tum.reconstruct_room."""
import ctypes as C
import os
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_mesh_cases as MC
import htsdf_mesh_restatement as HM
from icp_amd.synth import tum_K
from support import bits, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG = 1


def hashed_ctx(factory, case, opts=MC.OPTS, **kw):
    ctx = factory()
    ctx.tsdf_create_hashed(**opts, **kw)
    ctx.tsdf_upload_blocks(*case)
    return ctx


def fused_ctx(factory, opts, **kw):
    ctx = factory()
    ctx.tsdf_create_hashed(**opts, **kw)
    cam, _ = HC.camera()
    for d, P in zip(HC.frames(), HC.POSES):
        ctx.tsdf_integrate(d, cam, P)
    return ctx


def assert_same_mesh(got, want, what):
    assert (len(got[0]), len(got[2])) == (len(want[0]), len(want[2])), what
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2]), what
    assert np.array_equal(bits(got[0]), bits(want[0])), what
    assert np.array_equal(bits(got[1]), bits(want[1])), what


def check_against_restatement(ctx, opts, min_weight, what):
    """The device's mesh of the resident hashed volume == the restatement's of its blocks, order included."""
    _, coords, t, w = ctx.tsdf_blocks()
    got = ctx.tsdf_mesh_hashed(min_weight)
    want = HM.mesh(coords, t, w, opts["origin"], opts["voxel_size"], min_weight)
    print("%s: %d blocks, V %d, T %d (restatement %d, %d)" % (what, len(coords), len(got[0]), len(got[2]), len(want[0]), len(want[2])))
    assert_same_mesh(got, want, what)
    return got, (coords, t, w)


def dense_device_mesh(factory, blocks, opts, min_weight):
    """icp_tsdf_mesh of a second context's dense volume over the bounding box of the blocks."""
    d_opts, T, W = MC.dense_of(*blocks, opts)
    ctx = factory()
    ctx.tsdf_create(**d_opts)
    ctx.tsdf_upload(T, W)
    return ctx.tsdf_mesh(min_weight)


UPLOADED = [("A", MC.case_a, 0.0, False), ("B", MC.case_b, 0.0, True), ("C without (0,0,0)", lambda: MC.case_c((0, 0, 0)), 0.0, True),
            ("C without (-1,-1,-1)", lambda: MC.case_c((-1, -1, -1)), 0.0, True), ("D", MC.case_d, 0.0, True), ("D at min_weight 1.5", MC.case_d, 1.5, True),
            ("E", MC.case_e, 0.0, True), ("F", MC.case_f, 0.0, False)]


@pytest.mark.parametrize("name,make,mw,dense", UPLOADED, ids=[c[0] for c in UPLOADED])
def test_uploaded_blocks_bit_for_bit(gpu_ctx_factory, name, make, mw, dense):
    """Cases A to F: the restatement bit for bit, order included; B to E also icp_tsdf_mesh on the dense box, as a multiset of triangles."""
    ctx = hashed_ctx(gpu_ctx_factory, make())
    got, blocks = check_against_restatement(ctx, MC.OPTS, mw, name)
    assert len(got[2]) > 0
    if name == "F":
        assert np.isfinite(got[0]).all() and (np.abs(got[0]) > 1000).any()      # positions from the signed global coordinate
    if dense:
        want = dense_device_mesh(gpu_ctx_factory, blocks, MC.OPTS, mw)
        assert (len(got[0]), len(got[2])) == (len(want[0]), len(want[2]))
        assert np.array_equal(HM.triangle_rows(*got), HM.triangle_rows(*want))


@pytest.mark.parametrize("which", ["NEG", "STRADDLE"])
def test_fused_volume_bit_for_bit(gpu_ctx_factory, which):
    """Case H: three frames fused on the device.  NEG is dyadic and is also compared with the dense path; STRADDLE with the restatement only."""
    opts = getattr(HC, which)
    ctx = fused_ctx(gpu_ctx_factory, opts)
    got, blocks = check_against_restatement(ctx, opts, 0.0, "H(%s)" % which)
    assert len(got[2]) > 1000
    if which == "NEG":
        want = dense_device_mesh(gpu_ctx_factory, blocks, opts, 0.0)
        assert (len(got[0]), len(got[2])) == (len(want[0]), len(want[2]))
        assert np.array_equal(HM.triangle_rows(*got), HM.triangle_rows(*want))


@pytest.mark.parametrize("name,make", [("B", MC.case_b), ("E", MC.case_e)])
def test_pool_order_does_not_show(gpu_ctx_factory, name, make):
    """Case G: the blocks uploaded in key order, in reverse order, and into a volume of one block that grows on the way: identical arrays."""
    coords, t, w = make()
    ref = hashed_ctx(gpu_ctx_factory, (coords, t, w)).tsdf_mesh_hashed()
    assert len(ref[2]) > 0
    rev = hashed_ctx(gpu_ctx_factory, (coords[::-1], t[::-1], w[::-1]))
    assert_same_mesh(rev.tsdf_mesh_hashed(), ref, "reversed")
    grown = factory_grown(gpu_ctx_factory, coords, t, w)
    assert grown.tsdf_blocks()[0]["n_grown"] > 0
    assert_same_mesh(grown.tsdf_mesh_hashed(), ref, "grown")


def factory_grown(factory, coords, t, w):
    """block_capacity=1; half the blocks allocated in a shuffled order first (the pool grows several times), then everything uploaded."""
    ctx = factory()
    ctx.tsdf_create_hashed(block_capacity=1, **MC.OPTS)
    perm = np.random.default_rng(5).permutation(len(coords))
    ctx.tsdf_allocate_blocks(coords[perm[:len(perm) // 2 + 1]])
    ctx.tsdf_upload_blocks(coords[perm], t[perm], w[perm])
    return ctx


def raw_mesh(ctx, min_weight, max_v, max_t, v, n, t, counts=True):
    from icp_amd import binding
    nv, nt = C.c_int32(-5), C.c_int32(-5)
    rc = ctx.lib.icp_tsdf_mesh_hashed(ctx.h, C.c_float(min_weight), C.c_int32(max_v), C.c_int32(max_t), binding._ptr(v), binding._ptr(n), binding._ptr(t),
                                      C.byref(nv) if counts else None, C.byref(nt) if counts else None)
    return rc, nv.value, nt.value


def test_calling_contract(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    msg = lambda: ctx.lib.icp_last_error(ctx.h).decode()
    # no volume
    rc, nv, nt = raw_mesh(ctx, 0.0, 0, 0, None, None, None)
    assert rc == ERR_INVALID_ARG and "no volume" in msg() and (nv, nt) == (0, 0)
    # a dense volume: refused, named, untouched
    ctx.tsdf_create(dims=(16, 16, 16), origin=(0, 0, 0), voxel_size=0.125, truncation=0.5)
    before = ctx.tsdf_volume()
    rc, nv, nt = raw_mesh(ctx, 0.0, 0, 0, None, None, None)
    assert rc == ERR_INVALID_ARG and "dense" in msg() and (nv, nt) == (0, 0)
    after = ctx.tsdf_volume()
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    # an empty hashed volume
    ctx.tsdf_create_hashed(**MC.OPTS)
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None) == (0, 0, 0)
    ev, en, et = ctx.tsdf_mesh_hashed()
    assert ev.shape == (0, 3) and en.shape == (0, 3) and et.shape == (0, 3)
    # blocks without a sign change
    coords = HC.box_coords((-1, 0, 0), (2, 1, 1))
    ctx.tsdf_upload_blocks(coords, np.ones((2, 8, 8, 8), f32), np.ones((2, 8, 8, 8), f32))
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None) == (0, 0, 0)
    one = np.zeros((1, 3), f32); tri = np.zeros((1, 3), np.uint32)
    assert raw_mesh(ctx, 0.0, 1, 1, one, one.copy(), tri) == (0, 0, 0)
    # case B
    ctx.tsdf_upload_blocks(*MC.case_b())
    rv, rn, rt = HM.mesh(*MC.case_b(), MC.OPTS["origin"], MC.OPTS["voxel_size"])
    V, T = len(rv), len(rt)
    for bad in (float("nan"), -1.0, float("inf")):
        rc, nv, nt = raw_mesh(ctx, bad, 0, 0, None, None, None)
        assert rc == ERR_INVALID_ARG and "min_weight" in msg()
    # null count pointers
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None, counts=False)[0] == ERR_INVALID_ARG and "count" in msg()
    # count only
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None) == (0, V, T)
    # a capacity one too small on either side: the counts, a message with the four numbers, untouched arrays
    for max_v, max_t in ((V - 1, T), (V, T - 1)):
        v = np.full((V, 3), 7.5, f32); n = np.full((V, 3), 7.5, f32); t = np.full((T, 3), 0xABCDEF01, np.uint32)
        assert raw_mesh(ctx, 0.0, max_v, max_t, v, n, t) == (ERR_INVALID_ARG, V, T)
        assert all(str(x) in msg() for x in (V, T, max_v, max_t)), msg()
        assert (v == 7.5).all() and (n == 7.5).all() and (t == 0xABCDEF01).all()
    # exact capacities, with and without normals
    v = np.full((V, 3), 7.5, f32); n = np.full((V, 3), 7.5, f32); t = np.zeros((T, 3), np.uint32)
    assert raw_mesh(ctx, 0.0, V, T, v, n, t) == (0, V, T)
    assert np.array_equal(bits(v), bits(rv)) and np.array_equal(bits(n), bits(rn)) and np.array_equal(t, rt)
    v2 = np.zeros((V + 5, 3), f32); t2 = np.zeros((T + 5, 3), np.uint32)
    assert raw_mesh(ctx, 0.0, V + 5, T + 5, v2, None, t2) == (0, V, T)
    assert np.array_equal(bits(v2[:V]), bits(rv)) and np.array_equal(t2[:T], rt) and not v2[V:].any() and not t2[T:].any()
    pv, pn, pt = ctx.tsdf_mesh_hashed(normals=False)
    assert pn is None and np.array_equal(bits(pv), bits(rv)) and np.array_equal(pt, rt)
    # vertices and triangles go together
    assert raw_mesh(ctx, 0.0, V, T, v, n, None)[0] == ERR_INVALID_ARG and raw_mesh(ctx, 0.0, V, T, None, None, t)[0] == ERR_INVALID_ARG
    # icp_tsdf_mesh keeps refusing the hashed volume
    nv, nt = C.c_int32(0), C.c_int32(0)
    assert ctx.lib.icp_tsdf_mesh(ctx.h, C.c_float(0), 0, 0, None, None, None, C.byref(nv), C.byref(nt)) == ERR_INVALID_ARG and "hashed" in msg()
    # the volume released: refused again
    ctx.tsdf_release()
    assert raw_mesh(ctx, 0.0, 0, 0, None, None, None)[0] == ERR_INVALID_ARG and "no volume" in msg()


def test_volume_left_as_it_was(gpu_ctx_factory):
    """tsdf_blocks() is bit-identical before and after a mesh call; a further integrate and a tracked frame on the meshed context give what
    a context that never meshed gives; and the mesh after that integrate (the pool has grown) equals the restatement: the scratch follows."""
    from icp_amd import binding
    cam, _ = HC.camera()
    frames = HC.frames()
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        c.tsdf_create_hashed(block_capacity=64, **HC.NEG)
        for k in (0, 1):
            c.tsdf_integrate(frames[k], cam, HC.POSES[k])
    before = a.tsdf_blocks()
    first = a.tsdf_mesh_hashed()
    assert len(first[2]) > 100
    after = a.tsdf_blocks()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and same_bits(before[2], after[2]) and same_bits(before[3], after[3])
    o = a.tsdf_hashed_options
    assert tuple(o.origin) == tuple(f32(x) for x in HC.NEG["origin"]) and o.voxel_size == f32(HC.NEG["voxel_size"])
    # the same integrate on both
    assert a.tsdf_integrate(frames[2], cam, HC.POSES[2]) == b.tsdf_integrate(frames[2], cam, HC.POSES[2])
    ba, bb = a.tsdf_blocks(), b.tsdf_blocks()
    print("blocks %d -> %d, capacity %d -> %d, growths %d -> %d" % (before[0]["n_blocks"], ba[0]["n_blocks"], before[0]["capacity"], ba[0]["capacity"],
                                                                     before[0]["n_grown"], ba[0]["n_grown"]))
    assert ba[0]["n_blocks"] > before[0]["capacity"] and ba[0]["n_grown"] > before[0]["n_grown"]      # the pool has grown past what the scratch was sized for
    assert ba[0]["n_blocks"] == bb[0]["n_blocks"]
    assert np.array_equal(ba[1], bb[1]) and same_bits(ba[2], bb[2]) and same_bits(ba[3], bb[3])
    check_against_restatement(a, HC.NEG, 0.0, "after a further integrate")
    # the same tracked frames on both
    d = np.stack([frames[2], frames[1]])
    pa, ra, rca = a.track_depth_sdf(d, cam, pose=HC.POSES[2], stride=1, n_iterations=6)
    pb, rb, rcb = b.track_depth_sdf(d, cam, pose=HC.POSES[2], stride=1, n_iterations=6)
    assert rca == rcb and same_bits(pa, pb) and len(ra) == len(rb) == 1
    for key in ra[0]:
        assert np.array_equal(np.asarray(ra[0][key]), np.asarray(rb[0][key]), equal_nan=True), key
    ba, bb = a.tsdf_blocks(), b.tsdf_blocks()
    assert np.array_equal(ba[1], bb[1]) and same_bits(ba[2], bb[2]) and same_bits(ba[3], bb[3])


def test_context_left_alone(gpu_ctx_factory):
    """icp_run on a resident pair gives identical records before and after icp_tsdf_mesh_hashed; the params do not change."""
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
    ctx.tsdf_create_hashed(origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
    ctx.tsdf_integrate(depth[0], cam, np.eye(4, dtype=f32))
    before = binding.IcpParams(); ctx.lib.icp_get_params(ctx.h, C.byref(before))
    pose_a, recs_a, _ = ctx.run(np.eye(4))
    rmse_a = ctx.rmse(pose_a)
    v, n, t = ctx.tsdf_mesh_hashed()
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
    from icp_amd import meshio, tum
    W, H = 80, 60
    K = tum_K(W)
    d = str(tmp_path / "seq")
    tum.write_synthetic_sequence(d, 3, width=W, height=H, K=K)
    seq = tum.load_sequence(d, frame_step=1, K=K)
    model = dict(hashed=True, origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
    out = str(tmp_path / "out")
    ctx = gpu_ctx_factory()
    poses, recs, rc, paths = tum.reconstruct_room(ctx, seq, out_dir=out, model=model, sdf=dict(stride=1, n_iterations=10), model_mesh="m.ply", densify=False)
    assert sorted(os.listdir(out)) == ["m.ply", "mesh_0.off", "mesh_1.off", "mesh_2.off"] and len(paths) == 3
    v, n, t = meshio.load_ply_mesh(os.path.join(out, "m.ply"))
    info = ctx.tsdf_blocks()[0]                                   # still a hashed volume
    dv, dn, dt = ctx.tsdf_mesh_hashed()
    assert info["n_blocks"] > 10 and len(dt) > 100
    assert np.array_equal(bits(v), bits(dv)) and np.array_equal(bits(n), bits(dn)) and np.array_equal(t, dt)
    with pytest.raises(ValueError):
        tum.reconstruct_room(ctx, seq, out_dir=out, model=dict(dims=(8, 8, 8), origin=(0, 0, 0)), model_mesh="m.ply", densify=False)
