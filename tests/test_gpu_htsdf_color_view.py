"""The coloured views of the hashed TSDF volume on the device (icp_tsdf_raycast_color_hashed, icp_set_target_tsdf_color_hashed,
icp_track_depth_model_color_hashed, icp_tsdf_mesh_color_hashed): against the numpy restatement of their contract
(tests/htsdf_color_view_restatement.py) bit for bit on every case and camera size; against the dense coloured calls on the densified
volume; independence of where the blocks sit in the pool; the edge cases; the coloured target against the host route; the loop against a
composition of public calls, also while the pool grows; the mesh; the volume and the context left as they were; the refusals; the path
through tum; and the outcome on the textured wall."""
import ctypes as C
import functools
import json
import os
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_color_view_cases as VC
import htsdf_color_view_outcome_fixture as VOF
import htsdf_color_view_restatement as VR
import htsdf_raycast_cases as RC
import support as S
import tsdf_color_outcome_fixture as CF
import tsdf_restatement as TS
import tsdf_shape_cases as SC
from icp_amd.synth import camera_sequence
from support import bits, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE = 1, 3, 4
MODES = dict(colour_weighting=dict(weighting=3), colour_icp=dict(color_icp=1), colored_metric=dict(metric=4))      # test_gpu_tsdf_color.py's
configure = functools.partial(S.configure, n_iterations=35, max_distance=0.1, seed=0)
ROOM = dict(origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
NAMES = [c[0] for c in VC.all_cases()]


def color_ctx(factory, case, capacity=1 << 12, order=None):
    """A context whose coloured hashed volume holds the case's blocks and colours (uploaded in the given order)."""
    name, opts, c, t, w, rgb, wc, _ = case
    ctx = factory()
    ctx.tsdf_create_hashed(block_capacity=capacity, color=True, **{k: v for k, v in opts.items() if k != "dims"})
    o = np.arange(len(c)) if order is None else order
    ctx.tsdf_upload_blocks(c[o], t[o], w[o], rgb[o], wc[o])
    return ctx


def same_blocks(a, b):
    """Context.tsdf_blocks(colors=True) twice: the info, the coordinates and the four arrays bit for bit."""
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and all(same_bits(x, y) for x, y in zip(a[2:], b[2:]))


def assert_same_cast(got, want, what):
    """(depth, vertices, normals, rgba, hits, coloured hits) twice: NaN-safe bit comparison of the four arrays, both counts equal; holes
    consistent, and rgba == 0 exactly where there is no coloured hit."""
    assert got[4] == want[4] and got[5] == want[5], (what, got[4:6], want[4:6])
    for a, b, which in zip(got[:3], want[:3], ("depth", "vertices", "normals")):
        assert a.shape == b.shape and same_bits(a, b), (what, which, int((bits(a) != bits(b)).sum()))
    assert got[3].shape == want[3].shape and np.array_equal(got[3], want[3]), (what, "rgba", int((got[3] != want[3]).any(1).sum()))
    d = got[0].reshape(-1)
    assert int((d != MINF).sum()) == got[4] and ((got[1] == MINF).all(1) == (d == MINF)).all() and ((got[2] == MINF).all(1) == (d == MINF)).all(), what
    colored = got[3][:, 3] == 255
    assert int(colored.sum()) == got[5] and ((got[3] == 0).all(1) == ~colored).all() and not (colored & (d == MINF)).any(), what


@pytest.mark.parametrize("ci", range(len(NAMES)), ids=NAMES)
def test_device_equals_restatement(gpu_ctx_factory, ci):
    """Every case at every camera size (1 x 1, 7 x 5, 16 x 16, 17 x 33, 64 x 48) and every pose: the four arrays and both counts."""
    case = VC.all_cases()[ci]
    ctx = color_ctx(gpu_ctx_factory, case)
    total = colored = 0
    for si, (w, h) in enumerate(VC.SIZES):
        cam = RC.camera(w, h)[0]
        for pi, P in enumerate(case[7]):
            got = ctx.tsdf_raycast_color_hashed(cam, P)
            assert_same_cast(got, VC.restated(ci, si, pi), (case[0], w, h, pi))
            total += got[4]; colored += got[5]
    print("%s: %d hits, %d coloured over %d casts" % (case[0], total, colored, len(VC.SIZES) * len(case[7])))
    assert total >= colored > 100


@pytest.mark.parametrize("ci", range(len(VC.dense_equality_cases())), ids=[c[0] for c in VC.dense_equality_cases()])
def test_device_equals_the_dense_coloured_raycast(gpu_ctx_factory, ci):
    """P, and A - D and G moved to non-negative coordinates: icp_tsdf_raycast_color_hashed against icp_tsdf_raycast_color on the coloured
    volume densified from voxel (0, 0, 0) with the same origin (tsdf_upload + tsdf_color_upload), bit for bit, all four arrays, both counts."""
    case = VC.dense_equality_cases()[ci]
    d_opts, T, W, RGB, WC = VC.dense_lo0(case)
    hashed, dense = color_ctx(gpu_ctx_factory, case), gpu_ctx_factory()
    dense.tsdf_create(color=True, **d_opts)
    dense.tsdf_upload(T, W); dense.tsdf_color_upload(RGB, WC)
    total = 0
    for cw, ch in VC.SIZES:
        cam = RC.camera(cw, ch)[0]
        for pi, P in enumerate(case[7]):
            got, want = hashed.tsdf_raycast_color_hashed(cam, P), dense.tsdf_raycast_color(cam, P)
            assert_same_cast(got, want, (case[0], cw, ch, pi))
            total += got[5]
    assert total > 100


def test_pool_order_does_not_matter(gpu_ctx_factory):
    """P's blocks uploaded in key order and reversed, and P fused on the device from the colour frames into a pool that starts with ONE
    block and grows: identical arrays from the coloured cast and from tsdf_mesh_hashed(colors=True), equal to the restatement's."""
    cam, _ = HC.camera()
    case = VC.all_cases()[0]
    assert case[0] == "P"
    n = len(case[2])
    ctxs = [color_ctx(gpu_ctx_factory, case), color_ctx(gpu_ctx_factory, case, order=np.arange(n)[::-1].copy())]
    g = gpu_ctx_factory()
    g.tsdf_create_hashed(block_capacity=1, color=True, **HC.BOX)
    for d, c, P in zip(HC.frames(), VC.color_frames(), HC.POSES):
        g.tsdf_integrate(d, cam, P, rgbx=c)
    ctxs.append(g)
    info = g.tsdf_blocks()[0]
    assert info["n_grown"] > 3 and info["n_blocks"] == n
    for pi, P in enumerate(case[7]):
        want = VC.restated(0, len(VC.SIZES) - 1, pi)
        for k, ctx in enumerate(ctxs):
            assert_same_cast(ctx.tsdf_raycast_color_hashed(cam, P), want, ("pool order", k, pi))
    want = VC.restated_mesh(0, 0.0)
    for k, ctx in enumerate(ctxs):
        got = ctx.tsdf_mesh_hashed(colors=True)
        assert len(got[2]) > 1000 and all(np.array_equal(S.raw_bits(x), S.raw_bits(y)) for x, y in zip(got, want[:4])), k


def test_edge_cases_and_null_outputs(gpu_ctx_factory):
    """An empty volume and a pose looking away: all holes, no hit, ICP_ERR_NO_TARGET.  A coloured hashed volume fused WITHOUT colour frames:
    hits > 0, coloured hits 0, and the coloured target refuses with "nothing that has a colour".  Any output may be NULL."""
    from icp_amd import binding
    case = VC.all_cases()[0]
    cam = RC.camera(17, 33)[0]
    empty = gpu_ctx_factory()
    empty.tsdf_create_hashed(color=True, **HC.BOX)
    away = RC.pose((0.0, np.pi, 0.0), (0.0, 0.0, -1.0))
    ctx = color_ctx(gpu_ctx_factory, case)
    for what, c, P in (("empty", empty, case[7][0]), ("away", ctx, away)):
        d, v, n, rgba, hits, ncol = c.tsdf_raycast_color_hashed(cam, P)
        assert hits == 0 and ncol == 0 and (d == MINF).all() and (v == MINF).all() and (n == MINF).all() and (rgba == 0).all(), what
        assert c.set_target_tsdf_hashed(cam, P, check=False, color=True) == (0, ERR_NO_TARGET), what
        assert "nothing that has a colour" in c.lib.icp_last_error(c.h).decode()
    plain = gpu_ctx_factory()
    plain.tsdf_create_hashed(color=True, **HC.BOX)
    cam64, _ = HC.camera()
    for d, P in zip(HC.frames(), HC.POSES):
        plain.tsdf_integrate(d, cam64, P)
    d, v, n, rgba, hits, ncol = plain.tsdf_raycast_color_hashed(cam, case[7][0])
    assert hits == VC.restated(0, VC.SIZES.index((17, 33)), 0)[4] > 100 and ncol == 0 and (rgba == 0).all() and int((d != MINF).sum()) == hits
    assert plain.set_target_tsdf_hashed(cam, case[7][0], check=False, color=True) == (0, ERR_NO_TARGET)
    msg = plain.lib.icp_last_error(plain.h).decode()
    assert "nothing that has a colour" in msg and "icp_set_target_tsdf_color_hashed" in msg
    assert plain.set_target_tsdf_hashed(cam, case[7][0]) == hits                      # the geometry is still there
    # outputs one at a time
    P = case[7][0]
    full = ctx.tsdf_raycast_color_hashed(cam, P)
    npx = cam.width * cam.height
    p = binding.pose_to_c(P); hits = C.c_int32(0); ncol = C.c_int32(0)
    assert ctx.lib.icp_tsdf_raycast_color_hashed(ctx.h, C.byref(cam), binding._ptr(p), None, None, None, None, C.byref(hits), C.byref(ncol)) == 0
    assert hits.value == full[4] > 0 and ncol.value == full[5] > 0
    for k, (shape, dt) in enumerate((((npx,), f32), ((npx, 3), f32), ((npx, 3), f32), ((npx, 4), np.uint8))):
        buf = np.full(shape, 7, dt)
        args = [None, None, None, None]; args[k] = binding._ptr(buf)
        assert ctx.lib.icp_tsdf_raycast_color_hashed(ctx.h, C.byref(cam), binding._ptr(p), *args, None, None) == 0
        assert np.array_equal(S.raw_bits(buf.reshape(full[k].shape)), S.raw_bits(full[k])), k


@pytest.mark.parametrize("backend", [0, 1], ids=["brute", "lbvh"])
@pytest.mark.parametrize("mode", list(MODES))
def test_coloured_target_matches_the_host_route(gpu_ctx_factory, mode, backend):
    """icp_set_target_tsdf_color_hashed, then icp_correspond / icp_run, against icp_set_target with the host arrays of the coloured cast
    whose uncoloured hits were turned into holes: case G at 64 x 48, under colour weighting, colour ICP and the colored metric."""
    ci = NAMES.index("G")
    case = VC.all_cases()[ci]
    w, h = 64, 48
    cam = RC.camera(w, h)[0]
    a, b = color_ctx(gpu_ctx_factory, case), color_ctx(gpu_ctx_factory, case)
    for c in (a, b):
        S.configure(c, knn_backend=backend, n_iterations=10, max_distance=0.1, seed=0, **MODES[mode])
    target_pose = case[7][1]
    source_pose = target_pose @ S.pose_of((0.01, 0.02, 0.0), (-0.03, 0.02, 0.03))
    _, sv, sn, sc, _, _ = b.tsdf_raycast_color_hashed(cam, source_pose)
    keep = sc[:, 3] == 255
    sp, sn, sc = np.ascontiguousarray(sv[keep]), np.ascontiguousarray(sn[keep]), np.ascontiguousarray(sc[keep])
    n_a = a.set_target_tsdf_hashed(cam, target_pose, color=True)
    d, v, nr, rgba, hits, ncol = b.tsdf_raycast_color_hashed(cam, target_pose)
    drop = (rgba[:, 3] == 0) & (v[:, 2] != MINF)
    want = VC.restated(ci, VC.SIZES.index((w, h)), 1)
    print("coloured target (%s, backend %d): %d hits, %d coloured, %d dropped" % (mode, backend, hits, ncol, drop.sum()))
    assert n_a == ncol == want[5] and hits == want[4] and drop.sum() == hits - ncol > 50
    v = v.copy(); nr = nr.copy(); v[drop] = MINF; nr[drop] = MINF
    b.set_target(v, nr, rgba)
    for c in (a, b):
        c.set_source(sp, sn, sc)
    eye = np.eye(4, dtype=f32)
    ma, sa, na = a.correspond(eye); mb, sb, nb = b.correspond(eye)
    assert na == nb > 50 and np.array_equal(ma["idx"], mb["idx"]) and same_bits(ma["weight"], mb["weight"]) and (ma["idx"] < w * h).all()
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
    pa, ra, rca = a.run(eye, check=False); pb, rb, rcb = b.run(eye, check=False)
    assert rca == rcb and same_bits(pa, pb) and len(ra) == len(rb) > 0
    S.assert_same_run(ra, rb)


def python_loop(ctx, K, depth, rgbx, gt, cam, so):
    """icp_track_depth_model_color_hashed as a composition of public calls (the volume exists)."""
    W, H = cam.width, cam.height
    eye = np.eye(4, dtype=f32)
    pose = eye.copy()
    ctx.tsdf_integrate(depth[0], cam, pose, rgbx=rgbx[0])
    recs = []
    for k in range(1, len(depth)):
        r = dict(n_src=0, iterations=0, status=0, initial_rmse=-1.0, final_rmse=-1.0)
        _, trc = ctx.set_target_tsdf_hashed(cam, pose, check=False, color=True)
        r["n_src"], src_rc = ctx.set_source_depth(depth[k], rgbx[k], cam, so, check=False)
        if trc or src_rc:
            r["status"] = trc or src_rc
        else:
            xyz, _, _, valid = ctx.backproject_depth(depth[k], None, K, max_distance=so.max_distance)
            idx = np.arange(0, W * H, so.downsample_factor)
            sp = xyz[idx][valid[idx]]
            ctx.set_convergence_reference(sp, ctx.transform_points(sp, TS.gt_in_camera(pose, gt[k - 1])))
            r["initial_rmse"] = ctx.rmse(eye)
            dT, its, rc = ctx.run(eye, check=False)
            r["iterations"], r["status"] = len(its), rc
            r["final_rmse"] = ctx.rmse(dT)
            if rc == 0:
                pose = TS.compose_pose(pose, dT)
                ctx.tsdf_integrate(depth[k], cam, pose, rgbx=rgbx[k])
        r["pose"] = pose.copy()
        recs.append(r)
    return pose, recs


@pytest.mark.parametrize("mode,capacity", [(m, 16) for m in MODES] + [("colored_metric", 1)], ids=["%s, 16 blocks" % m for m in MODES] + ["colored_metric, 1 block"])
def test_track_depth_model_color_hashed_matches_composition_of_public_calls(gpu_ctx_factory, mode, capacity):
    """5 frames of 40 x 30 of the synthetic room with their colour frames, frame 2 all MINF, on a coloured hashed volume that starts with 16
    blocks, and with ONE, so that both pools grow inside the loop: records, poses and the blocks with their colours bit for bit; the
    empty frame carried and skipped with its status; the colour weight counts the frames fused."""
    from icp_amd import binding
    W, H = 40, 30
    K, depth, rgbx, gt = camera_sequence(5, W, H)
    depth[2][:] = MINF
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 1, SC.TRACK_MAX_DISTANCE, fix_color_index=True)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        configure(c, max_distance=0.3, **MODES[mode])
        c.tsdf_create_hashed(block_capacity=capacity, color=True, **ROOM)
    pose, recs, rc = a.track_depth_model_hashed(depth, cam, so, gt=gt, rgbx_frames=rgbx)
    ref_pose, ref = python_loop(b, K, depth, rgbx, gt, cam, so)
    print("track_depth_model_color_hashed (%s, capacity %d): statuses %s, iterations %s, n_src %s"
          % (mode, capacity, [r["status"] for r in recs], [r["iterations"] for r in recs], [r["n_src"] for r in recs]))
    assert len(recs) == 4 and rc == next((r["status"] for r in ref if r["status"]), 0) == ERR_NO_SOURCE
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert (r["n_src"], r["iterations"], r["status"]) == (h["n_src"], h["iterations"], h["status"]), k
        assert same_bits(r["pose"], h["pose"]), k
        assert bits(f32(r["initial_rmse"])) == bits(f32(h["initial_rmse"])) and bits(f32(r["final_rmse"])) == bits(f32(h["final_rmse"])), k
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    assert recs[0]["status"] == 0 and recs[1]["status"] == ERR_NO_SOURCE and same_bits(recs[1]["pose"], recs[0]["pose"]) and recs[1]["n_src"] == 0
    ab, bb = a.tsdf_blocks(colors=True), b.tsdf_blocks(colors=True)
    assert same_blocks(ab, bb)
    fused = 1 + sum(r["status"] == 0 for r in recs)
    assert ab[3].max() == fused and ab[5].max() == fused and ab[0]["n_grown"] == bb[0]["n_grown"] > 0 and ab[0]["n_unplaced"] == 0
    assert recs[0]["final_rmse"] < recs[0]["initial_rmse"] and recs[1]["initial_rmse"] == -1


DYADIC = ("NEG", "A", "B", "C without (0, 0, 0)", "D", "G")      # o + (float)lo s is exact: the dense box holds the same positions


@pytest.mark.parametrize("name", VC.MESH_CASES)
def test_mesh_colours(gpu_ctx_factory, name):
    """Every mesh case at two min_weights: all four arrays equal the restatement bit for bit, the first three equal tsdf_mesh_hashed();
    as a set of rows they equal tsdf_mesh(colors=True) on the dense coloured volume over the blocks' bounding box (where that box holds the
    same positions).  The counting call, colors_out NULL, and arrays too small: counts returned, nothing written."""
    from icp_amd import binding
    ci = NAMES.index(name)
    case = VC.all_cases()[ci]
    ctx = color_ctx(gpu_ctx_factory, case)
    dense = None
    if name in DYADIC:
        d_opts, T, W, RGB, WC = VC.dense_of(case)
        dense = gpu_ctx_factory()
        dense.tsdf_create(color=True, **d_opts)
        dense.tsdf_upload(T, W); dense.tsdf_color_upload(RGB, WC)
    for mw in VC.MIN_WEIGHTS:
        want = VC.restated_mesh(ci, mw)
        got = ctx.tsdf_mesh_hashed(min_weight=mw, colors=True)
        plain = ctx.tsdf_mesh_hashed(min_weight=mw)
        print("%s at min_weight %g: V %d, T %d, coloured vertices %d" % (name, mw, len(got[0]), len(got[2]), int((got[3][:, 3] == 255).sum())))
        for k, (x, y) in enumerate(zip(got, want[:4])):
            assert x.shape == y.shape and np.array_equal(S.raw_bits(x), S.raw_bits(y)), (name, mw, k)
        assert all(np.array_equal(S.raw_bits(x), S.raw_bits(y)) for x, y in zip(got[:3], plain))
        if dense is not None:
            dv, dn, dt, dc = dense.tsdf_mesh(min_weight=mw, colors=True)
            assert np.array_equal(VR.colored_triangle_rows(got[0], got[1], got[3], got[2]), VR.colored_triangle_rows(dv, dn, dc, dt)), (name, mw)
    v, n, t, col = ctx.tsdf_mesh_hashed(colors=True)
    nv, nt = C.c_int32(0), C.c_int32(0)
    P, B = binding._ptr, C.byref
    fn = ctx.lib.icp_tsdf_mesh_color_hashed
    assert fn(ctx.h, C.c_float(0), 0, 0, None, None, None, None, B(nv), B(nt)) == 0 and (nv.value, nt.value) == (len(v), len(t)) and len(t) > 100
    v2 = np.full_like(v, 7); t2 = np.full_like(t, 7)
    assert fn(ctx.h, C.c_float(0), len(v), len(t), P(v2), None, None, P(t2), B(nv), B(nt)) == 0                     # normals_out and colors_out NULL
    assert same_bits(v2, v) and np.array_equal(t2, t)
    v2[:] = 7; t2[:] = 7; c2 = np.full_like(col, 7)
    nv.value = nt.value = 0
    assert fn(ctx.h, C.c_float(0), len(v) - 1, len(t), P(v2), None, P(c2), P(t2), B(nv), B(nt)) == ERR_INVALID_ARG
    assert (nv.value, nt.value) == (len(v), len(t)) and (v2 == 7).all() and (t2 == 7).all() and (c2 == 7).all()
    assert "icp_tsdf_mesh_color_hashed" in ctx.lib.icp_last_error(ctx.h).decode()


def test_the_new_calls_leave_volume_and_context_as_they_were(gpu_ctx_factory):
    """Context a makes the three calls that are no loop between every step, context b never does: the blocks and their colours stay
    bit-identical, a further coloured integrate, an icp_tsdf_align_depth with color_weight > 0 equal b's, and an icp_run before and after
    the ray-cast and the mesh is unchanged (the target call replaces the target: that is what it is for)."""
    from icp_amd import binding
    cam, _ = HC.camera()
    case = VC.all_cases()[0]
    a, b = color_ctx(gpu_ctx_factory, case), color_ctx(gpu_ctx_factory, case)
    K, depth, rgbx, gt = camera_sequence(2, 80, 60)
    cam2 = binding.depth_camera(K, 80, 60)
    for c in (a, b):
        S.configure(c, n_iterations=10, max_distance=0.1, seed=0)
        c.set_target_depth(depth[0], None, cam2, binding.depth_options(False, 1))
        c.set_source_depth(depth[1], None, cam2, binding.depth_options(False, 4))
    before = a.tsdf_blocks(colors=True)
    prm_before = binding.IcpParams(); a.lib.icp_get_params(a.h, C.byref(prm_before))
    pose_0, recs_0, _ = a.run(np.eye(4))
    for P in case[7]:
        assert a.tsdf_raycast_color_hashed(cam, P)[5] > 100
    assert len(a.tsdf_mesh_hashed(colors=True)[3]) > 1000
    assert same_blocks(a.tsdf_blocks(colors=True), before)
    prm_after = binding.IcpParams(); a.lib.icp_get_params(a.h, C.byref(prm_after))
    assert bytes(prm_before) == bytes(prm_after)
    pose_1, recs_1, _ = a.run(np.eye(4))
    assert same_bits(pose_0, pose_1) and len(recs_0) == len(recs_1) > 0
    S.assert_same_run(recs_0, recs_1)
    assert a.set_target_tsdf_hashed(cam, case[7][0], color=True) > 100
    assert same_blocks(a.tsdf_blocks(colors=True), before)
    # what follows equals a context that never made the calls
    d, c = HC.frames()[1], VC.color_frames()[1]
    assert a.tsdf_integrate(d, cam, HC.POSES[1], rgbx=c) == b.tsdf_integrate(d, cam, HC.POSES[1], rgbx=c)
    a.tsdf_raycast_color_hashed(cam, case[7][1]); a.tsdf_mesh_hashed(colors=True)
    (pa, ra, rca), (pb, rb, rcb) = (x.tsdf_align_depth(HC.frames()[2], cam, HC.POSES[2], rgbx=VC.color_frames()[2], color_weight=0.1, stride=1, n_iterations=6) for x in (a, b))
    assert rca == rcb == 0 and same_bits(pa, pb) and ra["n_valid_last"] == rb["n_valid_last"] > 500
    a.set_target_tsdf_hashed(cam, case[7][0], color=True)
    assert same_blocks(a.tsdf_blocks(colors=True), b.tsdf_blocks(colors=True))


def test_refusals(gpu_ctx_factory):
    """The four new calls without a volume, on a dense volume and on a hashed volume without colours: ICP_ERR_INVALID_ARG with a message
    that names the call, nothing touched.  The loop's refusals (GICP, null colour frames, fix_color_index 0, another projective camera)
    leave the blocks bit-identical; the loop accepts the colour modes.  The geometry-only hashed calls stay legal on the coloured volume
    and leave the colours alone; the dense-named coloured calls keep refusing it."""
    from icp_amd import binding
    W, H = 40, 30
    K, depth, rgbx, gt = camera_sequence(3, W, H)
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 1, SC.TRACK_MAX_DISTANCE, fix_color_index=True)
    so_shifted = binding.depth_options(False, 1, SC.TRACK_MAX_DISTANCE)
    ctx = gpu_ctx_factory()
    configure(ctx)
    lib, h = ctx.lib, ctx.h
    eye = np.eye(4, dtype=f32)
    p = binding.pose_to_c(eye); n = C.c_int32(5); m = C.c_int32(5); out = (binding.IcpTrackFrame * 2)()
    d = np.ascontiguousarray(depth, f32); cols = np.ascontiguousarray(rgbx, np.uint8)
    buf = np.full(W * H * 3, 7, f32)
    P, B = binding._ptr, C.byref
    msg = lambda: lib.icp_last_error(h).decode()
    track = lambda s=so, r=cols: lib.icp_track_depth_model_color_hashed(h, P(d), P(r), C.c_int32(3), B(cam), B(s), None, P(p), out)
    new = {
        "icp_tsdf_raycast_color_hashed": lambda: lib.icp_tsdf_raycast_color_hashed(h, B(cam), P(p), P(buf), None, None, None, B(n), B(m)),
        "icp_set_target_tsdf_color_hashed": lambda: lib.icp_set_target_tsdf_color_hashed(h, B(cam), P(p), B(n)),
        "icp_track_depth_model_color_hashed": track,
        "icp_tsdf_mesh_color_hashed": lambda: lib.icp_tsdf_mesh_color_hashed(h, C.c_float(0), 0, 0, None, None, None, None, B(n), B(m)),
    }
    for name, call in new.items():
        assert call() == ERR_INVALID_ARG and "no volume" in msg() and name in msg(), (name, msg())
    ctx.tsdf_create(color=True, dims=(71, 35, 89), **ROOM)
    ctx.tsdf_integrate(depth[0], cam, eye, rgbx=rgbx[0])
    t0, w0 = ctx.tsdf_volume()
    for name, call in new.items():
        assert call() == ERR_INVALID_ARG and "dense" in msg() and name in msg(), (name, msg())
    t1, w1 = ctx.tsdf_volume()
    assert same_bits(t0, t1) and same_bits(w0, w1) and (buf == 7).all() and same_bits(binding.pose_from_c(p), eye)
    ctx.tsdf_create_hashed(**ROOM)
    ctx.tsdf_integrate(depth[0], cam, eye)
    plain = ctx.tsdf_blocks()
    for name, call in new.items():
        assert call() == ERR_INVALID_ARG and "no colours" in msg() and name in msg(), (name, msg())
    after = ctx.tsdf_blocks()
    assert after[0] == plain[0] and np.array_equal(after[1], plain[1]) and same_bits(after[2], plain[2]) and same_bits(after[3], plain[3]) and (buf == 7).all()
    # the coloured hashed volume: the loop's refusals
    ctx.tsdf_create_hashed(color=True, **ROOM)
    ctx.tsdf_integrate(depth[0], cam, eye, rgbx=rgbx[0])
    before = ctx.tsdf_blocks(colors=True)
    configure(ctx, metric=3)
    assert track() == ERR_INVALID_ARG and "GICP" in msg() and "icp_track_depth_model_color_hashed" in msg()
    configure(ctx)
    assert lib.icp_track_depth_model_color_hashed(h, P(d), None, C.c_int32(3), B(cam), B(so), None, P(p), out) == ERR_INVALID_ARG and "colour frames" in msg()
    assert track(so_shifted) == ERR_INVALID_ARG and "fix_color_index" in msg() and "icp_track_depth_model_color_hashed" in msg()
    configure(ctx, matching=1, knn_backend=0, K=K * np.array([[1.01], [1], [1]], f32), width=W, height=H)
    assert track() == ERR_INVALID_ARG and "camera" in msg()
    moved = binding.depth_camera(K, W, H, S.pose_of((0, 0, 0), (0.1, 0, 0)))
    assert lib.icp_tsdf_raycast_color_hashed(h, B(moved), P(p), P(buf), None, None, None, B(n), B(m)) == ERR_INVALID_ARG and "extrinsics" in msg()
    assert lib.icp_tsdf_mesh_color_hashed(h, C.c_float(-1), 0, 0, None, None, None, None, B(n), B(m)) == ERR_INVALID_ARG and "min_weight" in msg()
    configure(ctx)
    assert same_blocks(ctx.tsdf_blocks(colors=True), before) and same_bits(binding.pose_from_c(p), eye) and (buf == 7).all()
    # the dense-named coloured calls keep refusing the coloured hashed volume
    old = {
        "icp_tsdf_raycast_color": lambda: lib.icp_tsdf_raycast_color(h, B(cam), P(p), P(buf), None, None, None, B(n), B(m)),
        "icp_set_target_tsdf_color": lambda: lib.icp_set_target_tsdf_color(h, B(cam), P(p), B(n)),
        "icp_track_depth_model_color": lambda: lib.icp_track_depth_model_color(h, P(d), P(cols), C.c_int32(3), B(cam), B(so), None, P(p), out),
        "icp_tsdf_mesh_color": lambda: lib.icp_tsdf_mesh_color(h, C.c_float(0), 0, 0, None, None, None, None, B(n), B(m)),
    }
    for name, call in old.items():
        assert call() == ERR_INVALID_ARG and "hashed volume" in msg() and name in msg(), name
    # the geometry-only hashed calls stay legal and leave the colours alone
    assert ctx.tsdf_raycast_hashed(cam, eye)[3] > 100 and ctx.set_target_tsdf_hashed(cam, eye) > 100 and len(ctx.tsdf_mesh_hashed()[2]) > 100
    assert same_blocks(ctx.tsdf_blocks(colors=True), before)
    # and the loop runs under every colour mode
    for kw in MODES.values():
        configure(ctx, **kw)
        ctx.tsdf_reset()
        assert track() in (0, 8), (kw, msg())
    configure(ctx)


def test_through_tum(tmp_path, gpu_ctx_factory):
    """tum.track(model=dict(hashed=True, color=True, raycast="color", ...)) equals Context.track_depth_model_hashed(..., rgbx_frames=...)
    with the options it chooses (fix_color_index set); tum.reconstruct_room(..., densify=False, model_mesh=...) writes a PLY whose colours
    are tsdf_mesh_hashed(colors=True)'s and whose geometry is the uncoloured call's; a model without colours writes no colour property."""
    from icp_amd import binding, meshio, tum
    W, H = 80, 60
    K, depth, rgbx, gt = camera_sequence(4, W, H)
    seq = dict(depth=depth, rgbx=rgbx, gt=gt, K=K, width=W, height=H, frames=list(range(4)))
    model = dict(hashed=True, color=True, raycast="color", block_capacity=64, **ROOM)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        configure(c, **MODES["colour_weighting"])
    poses, recs, rc = tum.track(a, seq, model=model)
    b.params = tum.reconstruct_room_params(b.params, K, W, H); b.push_params()
    b.tsdf_create_hashed(block_capacity=64, color=True, **ROOM)
    cam = binding.depth_camera(K, W, H)
    o = tum.reconstruct_room_options(b.params)[1]
    so = binding.depth_options(bool(o.keep_original_size), int(o.downsample_factor), float(o.max_distance), fix_color_index=True)
    _, ref, rcb = b.track_depth_model_hashed(depth, cam, so, gt=gt, rgbx_frames=rgbx)
    print("tum.track on the coloured hashed ray-cast: statuses %s, iterations %s" % ([r["status"] for r in recs], [r["iterations"] for r in recs]))
    assert rc == rcb and len(recs) == len(ref) == 3 and len(poses) == 4
    for x, y in zip(recs, ref):
        assert (x["n_src"], x["iterations"], x["status"]) == (y["n_src"], y["iterations"], y["status"]) and same_bits(x["pose"], y["pose"])
    assert recs[0]["status"] == 0 and a.tsdf_blocks(colors=True)[5].max() >= 2
    out = str(tmp_path / "out")
    c = gpu_ctx_factory()
    configure(c, **MODES["colour_weighting"])
    _, recs_c, _, paths = tum.reconstruct_room(c, seq, out_dir=out, model=model, model_mesh="m.ply", densify=False)
    assert sorted(os.listdir(out)) == ["m.ply", "mesh_0.off", "mesh_1.off", "mesh_2.off", "mesh_3.off"] and len(paths) == 4
    v, n, t, col = meshio.load_ply_mesh(os.path.join(out, "m.ply"), colors=True)
    dv, dn, dt, dcol = c.tsdf_mesh_hashed(colors=True)
    pv, pn, pt = c.tsdf_mesh_hashed()
    assert len(dt) > 100 and np.array_equal(col, dcol) and np.array_equal(bits(v), bits(pv)) and np.array_equal(bits(n), bits(pn)) and np.array_equal(t, pt)
    assert (col[:, 3] == 255).sum() > 0.5 * len(col) and len(np.unique(col[:, :3], axis=0)) > 3
    for x, y in zip(recs_c, recs):
        assert x["status"] == y["status"] and same_bits(x["pose"], y["pose"])
    # a model without colours writes what it wrote before
    configure(c)
    tum.reconstruct_room(c, seq, out_dir=out, model=dict(hashed=True, raycast=True, block_capacity=64, **ROOM), model_mesh="plain.ply", densify=False)
    assert meshio.load_ply_mesh(os.path.join(out, "plain.ply"), colors=True)[3] is None


def test_outcome_on_the_textured_wall(gpu_ctx_factory):
    """The textured wall of tests/tsdf_color_outcome_fixture.py (12 frames of 160 x 120, 1 cm of lateral travel per frame, 0.11 m in all)
    through tum.track on a HASHED model: the coloured ray-cast loop under the colored metric, and the geometric ray-cast loop under
    point-to-plane.  Figures (translation error [m]):
      restatement loops on the CPU (tests/golden/htsdf_color_view_outcome.json, written by tests/htsdf_color_view_outcome_fixture.py):
        coloured worst frame 0.0021, geometric ends 0.1098 off (it stays where it started), 75 blocks
      device (MI355X): coloured worst frame 0.0021 (last 0.0019, status 0, 75 blocks), geometric ends 0.1098 off; printed below next to the bound
    The coloured loop's worst frame must stay below TWICE the CPU golden's (the project's standing margin for a device loop against its
    restatement); the geometric loop must end more than half the 0.11 m of travel from the truth."""
    from icp_amd import binding, tum
    with open(VOF.GOLDEN) as f:
        ref = json.load(f)
    K, depth, rgbx, gt = CF.fixture()
    seq = dict(depth=depth, rgbx=rgbx, gt=gt, K=K, width=CF.W, height=CF.H)
    ctx = gpu_ctx_factory()
    ctx.set_colored_options(CF.LAMBDA, CF.GRADIENT_K)
    opts = (binding.depth_options(False, 1), binding.depth_options(False, CF.SOURCE_FACTOR))

    def run(metric, model):
        configure(ctx, metric=metric)
        _, recs, rc = tum.track(ctx, seq, with_gt=False, model=model, options=opts)
        return CF.translation_errors([np.eye(4)] + [r["pose"] for r in recs], gt), recs, rc
    ec, recs_c, rc_c = run(4, VOF.hashed_model(True))
    n_blocks = ctx.tsdf_blocks()[0]["n_blocks"]
    eg, recs_g, rc_g = run(1, VOF.hashed_model(False))
    travel = CF.STEP_M * (CF.N_FRAMES - 1)
    print("restatement: coloured worst %.4f m, geometric ends %.4f m off, %d blocks; device: coloured worst %.4f m (bound %.4f, last %.4f, status %d, %d blocks), "
          "geometric ends %.4f m off (statuses %s); travel %.2f m"
          % (ref["colored_worst_translation_m"], ref["geometric_last_translation_m"], ref["n_blocks"], max(ec), 2 * ref["colored_worst_translation_m"], ec[-1], rc_c, n_blocks,
             eg[-1], sorted(set(r["status"] for r in recs_g)), travel))
    assert ref["lateral_travel_m"] == travel and 2 * ref["colored_worst_translation_m"] < travel / 2 < ref["geometric_last_translation_m"]
    assert rc_c == 0 and all(r["status"] == 0 for r in recs_c)
    assert max(ec) < 2 * ref["colored_worst_translation_m"]
    assert eg[-1] > travel / 2
