"""The TSDF kernels at the shapes their tiles make special (tests/tsdf_shape_cases.py lists them and says which tile each is about;
tests/test_tsdf_shape_cases_host.py shows without a device that every input reaches the code it is meant for).  Every comparison is bit
for bit: against the restatements (tsdf_restatement, tsdf_color_restatement, tsdf_mesh_restatement), and against the device itself where
a result must not depend on the tile -- a volume against the slice of a larger one, a frame against the crop of a larger one, the model
target on a context whose planes hold another target's points against the host route on a fresh context.

  integrate, plain and coloured     the nine volumes from (2, 2, 2) to exactly 2 x 2 x 2 tiles; slices of the largest
  ray-cast, plain and coloured      nine frames from one pixel to 40 x 30, three poses; crops of the largest
  the model target                  frames of 1200, 289 and 495 pixels (16, 31, 17 padded entries), both k-NN back ends, with and without
                                    colours, after a 4096-point target made of copies of the source; the tracking loop likewise
  mesh and coloured mesh            the nine volumes; all 256 corner-sign cases of a cell in three layouts

Measured (MI355X): every deviation 0."""
import numpy as np
import pytest

import support as S
import tsdf_shape_cases as SC
import tsdf_mesh_restatement as TM
from support import bits, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)


def camera(size=(SC.W, SC.H)):
    from icp_amd import binding
    return binding.depth_camera(SC.camera_matrix(), *size)


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    """One context for the integrate and mesh tests: every volume replaces the one before, the scratch buffers stay."""
    return gpu_ctx_factory()


# ---- 1. integrate

def run_integrate(ctx, case, color):
    """The case's start uploaded and its steps integrated: [(updated, coloured or None, tsdf, weight, rgb or None, wc or None)] after every step."""
    ctx.tsdf_create(color=color, **case["opts"])
    t0, w0, c0, wc0 = case["start"]
    ctx.tsdf_upload(t0, w0)
    if color:
        ctx.tsdf_color_upload(c0, wc0)
    out = []
    for depth, rgbx, pose in case["steps"]:
        if color:
            n, ncol = ctx.tsdf_integrate(depth, camera(), pose, rgbx=rgbx)
        else:
            n, ncol = ctx.tsdf_integrate(depth, camera(), pose), None
        out.append((n, ncol) + ctx.tsdf_volume() + (ctx.tsdf_color_volume() if color else (None, None)))
    return out


@pytest.mark.parametrize("color", [False, True], ids=["plain", "coloured"])
@pytest.mark.parametrize("dims", SC.VOLUMES, ids=str)
def test_integrate_matches_restatement(ctx, dims, color):
    """Two frames at two poses and the first once more with max_weight = 2, from a crafted start: the counts and every bit of tsdf, weight
    (and colour, Wc) after every call; the NaN payloads where nothing is written keep their bits."""
    case = SC.integrate_case(dims)
    got, ref = run_integrate(ctx, case, color), SC.integrate_reference(dims)
    for k, (g, r) in enumerate(zip(got, ref)):
        print("integrate %s step %d: %d written%s (restatement %d, %d)" % (dims, k, g[0], "" if not color else ", %d coloured" % g[1], r[0], r[1]))
        assert g[0] == r[0] and (not color or g[1] == r[1]), (dims, k)
        assert same_bits(g[2], r[2]) and same_bits(g[3], r[3]), (dims, k)
        if color:
            assert same_bits(g[4], r[4]) and same_bits(g[5], r[5]), (dims, k)
    m = case["marked"]
    assert (bits(got[-1][2])[m] == 0x7FC12345).all() and (bits(got[-1][3])[m] == 0xFFC54321).all()
    if color:
        assert (bits(got[-1][4])[m] == 0x7FC0BEEF).all() and (bits(got[-1][5])[m] == 0xFFC0FACE).all()


@pytest.mark.parametrize("color", [False, True], ids=["plain", "coloured"])
def test_integrate_slices(ctx, color):
    """A voxel's update depends on that voxel alone: the volumes (64, 4, 16), (65, 5, 17) and (2, 2, 2) at the origin and voxel size of
    (128, 8, 32), started from the slice of its start, equal the slice [:nz, :ny, :nx] of the DEVICE's (128, 8, 32) after every call."""
    big = run_integrate(ctx, SC.integrate_case(SC.BIG), color)
    for dims in SC.SLICES:
        nx, ny, nz = dims
        got = run_integrate(ctx, SC.integrate_case(dims, SC.BIG), color)
        for k, (g, b) in enumerate(zip(got, big)):
            assert g[0] > 0, (dims, k)
            for x, y in zip(g[2:], b[2:]):
                assert x is None or same_bits(x, y[:nz, :ny, :nx]), (dims, k)
            inside = SC.integrate_reference(dims, SC.BIG)[k]
            assert g[0] == inside[0] and (not color or g[1] == inside[1]), (dims, k)


# ---- 2. ray-cast

@pytest.fixture(scope="module")
def ray(gpu_ctx_factory):
    """(context, the device's 40 x 30 outputs per pose): RAY_OPTS fused on the device from the two frames, with their colours; the
    downloaded arrays are the restatement's, so the references of tsdf_shape_cases hold for the device's volume; then the slabs of Wc = 0."""
    c = gpu_ctx_factory()
    c.tsdf_create(color=True, **SC.RAY_OPTS)
    for depth, rgbx, pose in SC.ray_frames():
        c.tsdf_integrate(depth, camera(), pose, rgbx=rgbx)
    vol = SC.ray_volume()
    t, w = c.tsdf_volume(); rgb, wc = c.tsdf_color_volume()
    assert same_bits(t, vol.tsdf) and same_bits(w, vol.weight) and same_bits(rgb, vol.rgb) and same_bits(wc, vol.fused_wc)
    c.tsdf_color_upload(vol.rgb, vol.wc)
    full = {name: (c.tsdf_raycast(camera(), pose), c.tsdf_raycast_color(camera(), pose)) for name, pose in SC.RAY_POSES.items()}
    return c, full


@pytest.mark.parametrize("size", SC.RAY_SIZES, ids=str)
def test_raycast_matches_restatement_and_crop(ray, size):
    """Depth, vertices, normals and the hit count of icp_tsdf_raycast, and with them the packed colours and the coloured count of
    icp_tsdf_raycast_color, against the restatement from every pose; and against [:h, :w] of the device's own 40 x 30 output, the hit
    count against the hits in that rectangle ((64, 1) reaches beyond the frame: its first 40 pixels are held against row 0)."""
    c, full = ray
    w, h = size
    for name, pose in SC.RAY_POSES.items():
        rd, rv, rn, rrgba, rhits, rncol, _ = SC.ray_reference(size, name)
        d, v, n, hits = c.tsdf_raycast(camera(size), pose)
        cd, cv, cn, rgba, chits, ncol = c.tsdf_raycast_color(camera(size), pose)
        print("ray-cast %s %s: %d hits, %d coloured (restatement %d, %d)" % (size, name, hits, ncol, rhits, rncol))
        assert (hits, chits, ncol) == (rhits, rhits, rncol), (size, name)
        for got in ((d, v, n), (cd, cv, cn)):
            assert same_bits(got[0], rd) and same_bits(got[1], rv) and same_bits(got[2], rn), (size, name)
        assert np.array_equal(rgba, rrgba), (size, name)
        (fd, fv, fn, fhits), (gd, gv, gn, frgba, ghits, gncol) = full[name]
        if w <= SC.W and h <= SC.H:
            for x, y in zip((d, v, n), SC.crop(size, fd, fv, fn)):
                assert same_bits(x, y), (size, name)
            for x, y in zip((cd, cv, cn, rgba), SC.crop(size, gd, gv, gn, frgba)):
                assert np.array_equal(S.raw_bits(x), S.raw_bits(y)), (size, name)
            assert hits == int((fd[:h, :w] != MINF).sum()) and ncol == int((frgba.reshape(SC.H, SC.W, 4)[:h, :w, 3] != 0).sum()), (size, name)
        else:
            assert same_bits(d[:SC.H, :SC.W], fd[:h, :w]) and same_bits(cd[:SC.H, :SC.W], gd[:h, :w]), (size, name)
            assert np.array_equal(rgba.reshape(h, w, 4)[:SC.H, :SC.W], frgba.reshape(SC.H, SC.W, 4)[:h, :w]), (size, name)
        if size == (1, 1):
            assert ("hit" if hits else "hole") == SC.ONE_PIXEL[name]


# ---- 3. the model target with padding, on a context with stale planes

def model_ctx(factory, color, backend, opts, vol=None):
    c = factory()
    S.configure(c, knn_backend=backend, color_icp=int(color), **SC.TARGET_PARAMS)
    c.tsdf_create(color=color, **opts)
    if vol is not None:
        c.tsdf_upload(vol.tsdf, vol.weight)
        if color:
            c.tsdf_color_upload(vol.rgb, vol.wc)
    return c


TARGET_CASES = [(size, color, backend) for size in SC.TARGET_FRAMES for color in (False, True) for backend in (0, 1)]
target_ids = ["%dx%d-%s-%s" % (s[0], s[1], "coloured" if c else "plain", "lbvh" if b else "brute") for s, c, b in TARGET_CASES]


@pytest.mark.parametrize("size,color,backend", TARGET_CASES, ids=target_ids)
def test_model_target_padding_on_stale_planes(gpu_ctx_factory, size, color, backend):
    """Context a held a 4096-point target made of copies of the source as it lies after each of the two poses, so its planes beyond W H
    hold zero-distance matches; then icp_set_target_tsdf[_color].  Context b is fresh and takes the host route (icp_tsdf_raycast[_color],
    uncoloured hits masked to holes, icp_set_target).  icp_correspond at both poses: equal idx, weight bits and sums, no idx >= W H;
    icp_run: the same pose bits and status."""
    w, h = size
    n = w * h
    vol = SC.ray_volume()
    a, b = (model_ctx(gpu_ctx_factory, color, backend, SC.RAY_OPTS, vol) for _ in range(2))
    sp, sn, sc = SC.target_source(size, color)
    poses = (SC.EYE, SC.SOURCE_POSE)
    stale = SC.stale_cloud([(a.transform_points(sp, p), a.transform_normals(sn, p), sc) for p in poses])
    assert len(stale[0]) >= SC.padded(n)
    a.set_target(stale[0], stale[1], stale[2] if color else None)
    hits = a.set_target_tsdf(camera(size), SC.EYE, color=color)
    if color:
        d, v, nr, rgba, all_hits, ncol = b.tsdf_raycast_color(camera(size), SC.EYE)
        drop = (rgba[:, 3] == 0) & (v[:, 2] != MINF)
        v = v.copy(); nr = nr.copy(); v[drop] = MINF; nr[drop] = MINF
        b.set_target(v, nr, rgba)
        assert hits == ncol and drop.sum() == all_hits - ncol
    else:
        d, v, nr, all_hits = b.tsdf_raycast(camera(size), SC.EYE)
        b.set_target(v, nr)
        assert hits == all_hits
    assert hits == SC.target_reference(size, color)[3] and 0 < hits < n
    for c in (a, b):
        c.set_source(sp, sn, sc if color else None)
    for pose in poses:
        ma, sa, na = a.correspond(pose); mb, sb, nb = b.correspond(pose)
        print("target %s coloured %d backend %d: %d hits, %d matched of %d, largest idx %d" % (size, color, backend, hits, na, len(sp), ma["idx"].max()))
        assert (ma["idx"] < n).all(), (size, int(ma["idx"].max()))
        assert na == nb and np.array_equal(ma["idx"], mb["idx"]) and same_bits(ma["weight"], mb["weight"])
        assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
    assert na > 50
    pa, ra, rca = a.run(SC.EYE, check=False); pb, rb, rcb = b.run(SC.EYE, check=False)
    assert rca == rcb and same_bits(pa, pb) and len(ra) == len(rb) > 0
    S.assert_same_run(ra, rb)


@pytest.mark.parametrize("size,color,backend", TARGET_CASES, ids=target_ids)
def test_track_depth_model_on_stale_planes(gpu_ctx_factory, size, color, backend):
    """icp_track_depth_model[_color] over three frames of this size on a context whose target planes hold 4096 copies of the sources the
    loop will see at its first iterations (frames 1 and 2 back-projected: the loop starts every frame from the identity), against the
    same call on a fresh context, record for record, and the fused volumes bit for bit.  The plane buffers are larger than they need be."""
    from icp_amd import binding
    w, h = size
    K, depth, rgbx, gt = SC.track_frames(size)
    cam = binding.depth_camera(K, w, h)
    so = binding.depth_options(False, 1, max_distance=SC.TRACK_MAX_DISTANCE, fix_color_index=color)
    a, b = (model_ctx(gpu_ctx_factory, color, backend, SC.ROOM_OPTS) for _ in range(2))
    moved = []
    for k in (1, 2):
        xyz, nrm, rgba, valid = a.backproject_depth(depth[k], rgbx[k], K, max_distance=SC.TRACK_MAX_DISTANCE, fix_color_index=True)
        ok = valid & np.isfinite(nrm).all(1)
        assert ok.sum() > 100
        moved.append((xyz[ok], nrm[ok], rgba[ok]))
    stale = SC.stale_cloud(moved)
    a.set_target(stale[0], stale[1], stale[2] if color else None)
    frames = rgbx if color else None
    (pa, ra, rca), (pb, rb, rcb) = a.track_depth_model(depth, cam, so, gt=gt, rgbx_frames=frames), b.track_depth_model(depth, cam, so, gt=gt, rgbx_frames=frames)
    print("track %s coloured %d backend %d: statuses %s, iterations %s, n_src %s" % (size, color, backend, [r["status"] for r in rb], [r["iterations"] for r in rb], [r["n_src"] for r in rb]))
    assert rca == rcb and same_bits(pa, pb) and len(ra) == len(rb) == 2
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert (x["n_src"], x["iterations"], x["status"]) == (y["n_src"], y["iterations"], y["status"]), k
        assert same_bits(x["pose"], y["pose"]), k
        assert bits(f32(x["initial_rmse"])) == bits(f32(y["initial_rmse"])) and bits(f32(x["final_rmse"])) == bits(f32(y["final_rmse"])), k
    for x, y in zip(a.tsdf_volume() + (a.tsdf_color_volume() if color else ()), b.tsdf_volume() + (b.tsdf_color_volume() if color else ())):
        assert same_bits(x, y)
    assert rb[0]["n_src"] > 100 and rb[0]["iterations"] > 0 and rb[0]["status"] == 0        # a frame was aligned against the model


# ---- 4. and 5. mesh

def check_mesh(ctx, vol, ref, what):
    """icp_tsdf_mesh and icp_tsdf_mesh_color of `vol` against the restatement's (vertices, normals, triangles, colours): the counts, every
    bit, every index below V, no directed edge twice."""
    S.upload(ctx, vol, color=True)
    rv, rn, rt, rcol = ref
    v, n, t = ctx.tsdf_mesh()
    cv, cn, ct, col = ctx.tsdf_mesh(colors=True)
    print("mesh %s: V %d, T %d (restatement %d, %d)" % (what, len(v), len(t), len(rv), len(rt)))
    assert (len(v), len(t)) == (len(cv), len(ct)) == (len(rv), len(rt)) and len(t) > 0, what
    for got in ((v, n, t), (cv, cn, ct)):
        assert got[2].dtype == np.uint32 and np.array_equal(got[2], rt), what
        assert same_bits(got[0], rv) and same_bits(got[1], rn), what
    assert np.array_equal(col, rcol), what
    assert int(t.max()) < len(v) and TM.edge_counts(t)[1] == 0, what


@pytest.mark.parametrize("dims", SC.VOLUMES, ids=str)
def test_mesh_matches_restatement(ctx, dims):
    check_mesh(ctx, SC.mesh_volume(dims), SC.mesh_reference("shape", dims), str(dims))


@pytest.mark.parametrize("layout", list(SC.LAYOUTS))
def test_all_256_cell_cases(ctx, layout):
    """Every corner-sign case of a cell, one cell each, exact zeros of both signs among the corners: rows of 47 voxels, rows that are one
    run each, and the cells turned into the y-z plane of a volume with rows of 2."""
    check_mesh(ctx, SC.case_volume(layout), SC.mesh_reference("cases", layout), layout)
