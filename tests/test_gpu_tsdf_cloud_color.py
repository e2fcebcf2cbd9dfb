"""The colours of laser scans fused into the coloured TSDF volume on the device (icp_tsdf_integrate_cloud_color, icp_track_scans_sdf_color;
DESIGN.md section 6zh) against the numpy restatement of the contract (tests/tsdf_cloud_color_restatement.py), BIT FOR BIT: colours, colour
weights and n_colored of every case of tests/tsdf_cloud_color_cases.py on both storages, with geometry, info and carve stats those of
icp_tsdf_integrate_cloud on a twin context; the same with carving on; an uncoloured fuse on a coloured volume; the tracking loop; the
refusals; and the outcome: twelve coloured scans into a model, a coloured mesh and a PLY."""
import ctypes
import time

import numpy as np
import pytest

import htsdf_restatement as HR
import sdf_cloud_cases as SK
import sdf_cloud_outcome_fixture as SOF
import sdf_cloud_restatement as SC
import support as S
import tsdf_cloud_color_cases as K
import tsdf_cloud_color_outcome_fixture as OF
import tsdf_cloud_color_restatement as KR
import tsdf_cloud_outcome_fixture as CF
import tsdf_cloud_restatement as CR
from support import same_bits
from tsdf_cloud_cases import cloud, OPTS, TILTED, EYE

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, ERR_INVALID_ARG, ERR_COLOR_MISMATCH = 0, 1, 7
OFF = dict(distance=0.0, min_range=0.0)


def create(ctx, c, color):
    if c["dims"] is None:
        ctx.tsdf_create_hashed(block_capacity=c["capacity"], color=color, **c["opts"])
    else:
        ctx.tsdf_create(dims=c["dims"], color=color, **c["opts"])


def run(ctx, c, carve=OFF, color=True):
    """The case on the device: a coloured volume and the coloured fuse, or (color=False) the twin -- a volume without colours and
    icp_tsdf_integrate_cloud.  -> per fuse step (info, carve stats, n_colored or None)"""
    create(ctx, c, color)
    ctx.set_tsdf_carve(**carve)
    out = []
    for st in c["steps"]:
        if st[0] == "evict":
            assert ctx.tsdf_evict_blocks(st[1], st[2], hold=False)[0]["n_evicted"] > 0
            continue
        _, pts, rgba, pose, origin = st
        if color:
            ctx.set_source(pts, None, rgba)
            info = ctx.tsdf_integrate_cloud("source", pose=pose, sensor_origin=origin, color=True)
            nc = info.pop("n_colored")
        else:
            ctx.set_source(pts)
            info, nc = ctx.tsdf_integrate_cloud("source", pose=pose, sensor_origin=origin), None
        st_ = ctx.tsdf_carve_stats()
        out.append((info, dict(n_steps=st_["n_steps"], n_carved=st_["n_carved"]), nc))
    ctx.set_tsdf_carve(0.0)
    return out


def geometry(ctx, c):
    return ctx.tsdf_blocks()[1:] if c["dims"] is None else ctx.tsdf_volume()


def colours(ctx, c):
    return ctx.tsdf_blocks(colors=True)[4:] if c["dims"] is None else ctx.tsdf_color_volume()


def same_state(a, b):
    return len(a) == len(b) and all(same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a, b))


def geometry_equals(ctx, vol, what):
    if isinstance(vol, HR.HVolume):
        S.tsdf_blocks_equal_restatement(ctx, vol, what)
    else:
        T, W = ctx.tsdf_volume()
        assert same_bits(T, vol.tsdf) and same_bits(W, vol.weight), what


@pytest.mark.parametrize("name", list(K.CASES))
def test_device_equals_restatement(gpu_ctx_factory, name):
    """Every case: colours, colour weights and n_colored equal the restatement's bit for bit; geometry, info and carve stats equal the
    restatement's and those of icp_tsdf_integrate_cloud on a twin context without colours."""
    c = K.CASES[name]
    want, vol = K.reference(name)
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    got = run(ctx, c)
    print("%s: %s" % (name, [(o[0]["n_updated"], o[2]) for o in got]))
    assert got == want, (name, got, want)
    geometry_equals(ctx, vol, name)
    assert same_state(colours(ctx, c), KR.colors_of(vol)), name
    plain = run(twin, c, color=False)
    assert [o[:2] for o in plain] == [o[:2] for o in got] and same_state(geometry(ctx, c), geometry(twin, c)), name
    if c["dims"] is None:
        assert ctx.tsdf_blocks()[0] == twin.tsdf_blocks()[0]


@pytest.mark.parametrize("name", K.CARVED)
def test_with_carving_on(gpu_ctx_factory, name):
    """distance 0.5 and inf: geometry, info and carve stats equal the uncoloured carved fuse on a twin context, colours and n_colored equal
    the UNCARVED coloured fuse's."""
    c = K.CASES[name]
    want, vol = K.reference(name)
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for carve in K.CARVES:
        got, plain = run(ctx, c, carve), run(twin, c, carve, color=False)
        assert [o[:2] for o in got] == [o[:2] for o in plain] and same_state(geometry(ctx, c), geometry(twin, c)), (name, carve)
        assert [o[2] for o in got] == [o[2] for o in want] and same_state(colours(ctx, c), KR.colors_of(vol)), (name, carve)
        assert all(o[1]["n_steps"] > 0 for o in got)


@pytest.mark.parametrize("kind", ["hashed", "dense"])
def test_an_uncoloured_fuse_leaves_the_colours(gpu_ctx_factory, kind):
    """icp_tsdf_integrate_cloud on a coloured volume behind a coloured fuse: geometry moves on, the colours of what existed keep their
    bits, new blocks are uncoloured."""
    c = K.CASES["n257/" + kind]
    ctx = gpu_ctx_factory()
    run(ctx, c)
    before = colours(ctx, c); coords0 = ctx.tsdf_blocks()[1] if kind == "hashed" else None
    ctx.set_source(cloud(400, seed=77))
    assert ctx.tsdf_integrate_cloud("source", pose=EYE)["n_updated"] > 0
    after = colours(ctx, c)
    if kind == "dense":
        assert same_state(before, after) and before[1].max() == 1
        return
    coords1 = ctx.tsdf_blocks()[1]
    key = lambda cc: (cc[:, 2].astype(np.int64) << 42) + (cc[:, 1].astype(np.int64) << 21) + cc[:, 0]
    at = np.searchsorted(key(coords1), key(coords0))
    assert np.array_equal(coords1[at], coords0) and same_bits(after[0][at], before[0]) and same_bits(after[1][at], before[1]) and before[1].max() == 1
    new = np.ones(len(coords1), bool); new[at] = False
    assert new.any() and not after[0][new].any() and not after[1][new].any()


def same_records(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


@pytest.mark.parametrize("storage", ["dense", "hashed"])
def test_the_loop(gpu_ctx_factory, storage):
    """track_scans_sdf(colors=...) on four small scans: poses, records and infos are bit-identical to the uncoloured loop on a twin
    context; the colours equal the restatement's coloured fuses at those poses; eth.track_tsdf(colors=...) is the same call."""
    from icp_amd import eth
    scans, cols, _ = K.track_scans()
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    case = dict(opts=SK.OPTS, dims=SK.DIMS if storage == "dense" else None, capacity=64)
    create(ctx, case, True); create(twin, case, False)
    poses, recs, infos, status, ncs = ctx.track_scans_sdf(scans, SK.TRACK_POSES[0], colors=cols, n_iterations=10)
    tposes, trecs, tinfos, tstatus = twin.track_scans_sdf(scans, SK.TRACK_POSES[0], n_iterations=10)
    assert status == tstatus == OK and all(same_bits(a, b) for a, b in zip(poses, tposes)) and same_records(recs, trecs) and infos == tinfos
    assert same_state(geometry(ctx, case), geometry(twin, case))
    vol = K.new_volume(case)
    want = [KR.integrate(vol, s, col, T) for s, col, T in zip(scans, cols, poses)]
    print("%s loop: n_colored %s of n_updated %s" % (storage, ncs, [i["n_updated"] for i in infos]))
    assert [w[0] for w in want] == infos and [w[2] for w in want] == ncs and all(n > 0 for n in ncs)
    geometry_equals(ctx, vol, storage + " loop")
    assert same_state(colours(ctx, case), KR.colors_of(vol))
    kw = dict(voxel_size=SK.OPTS["voxel_size"], truncation=SK.OPTS["truncation"], origin=SK.OPTS["origin"], max_range=SK.OPTS["max_depth"], block_capacity=64)
    kw.update(dict(hashed=True) if storage == "hashed" else dict(hashed=False, dims=SK.DIMS))
    again = eth.track_tsdf(twin, scans, SK.TRACK_POSES[0], colors=cols, n_iterations=10, **kw)
    assert len(again) == 5 and again[4] == ncs and all(same_bits(a, b) for a, b in zip(again[0], poses))
    assert same_state(colours(twin, case), colours(ctx, case))
    # a scan that fails is skipped: n_colored 0, zeroed info
    far = [scans[0], (scans[1] + f32(50.0)).astype(f32)]
    create(ctx, case, True)
    out = ctx.track_scans_sdf(far, SK.TRACK_POSES[0], colors=cols[:2], n_iterations=10)
    assert out[3] != OK and out[4][0] == ncs[0] and out[4][1] == 0 and out[2][1]["n_updated"] == 0


def test_refusals_leave_the_bits(gpu_ctx_factory):
    """A volume without colours, a cloud without colours, the loop's null colours: refused with a message that names the call, geometry
    and colours as they were."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    lib = ctx.lib
    p = binding.pose_to_c(TILTED)
    msg = lambda: lib.icp_last_error(ctx.h).decode()
    info = binding.IcpTsdfCloudInfo(); nc = ctypes.c_int32(-1)
    call = lambda which=1: lib.icp_tsdf_integrate_cloud_color(ctx.h, which, binding._ptr(p), None, ctypes.byref(info), ctypes.byref(nc))
    scan = np.ascontiguousarray(cloud(50)); rgba = K.colours(50, 3)
    xp = (ctypes.c_void_p * 1)(binding._ptr(scan)); cp = (ctypes.c_void_p * 1)(binding._ptr(rgba)); none = (ctypes.c_void_p * 1)(None); cn = (ctypes.c_int32 * 1)(50)
    o = binding.sdf_options()
    loop = lambda cols: lib.icp_track_scans_sdf_color(ctx.h, xp, cols, cn, 1, ctypes.byref(o), binding._ptr(p.copy()), None, None, None)
    for kind in ("hashed", "dense"):
        c = K.CASES["n257/" + kind]
        # no colours in the volume
        create(ctx, c, False)
        ctx.set_source(scan, None, rgba)
        assert ctx.tsdf_integrate_cloud("source", pose=TILTED)["n_updated"] > 0
        before = geometry(ctx, c)
        assert call() == ERR_INVALID_ARG and "icp_tsdf_integrate_cloud_color" in msg() and "no colours" in msg() and nc.value == 0 and info.n_points == 0
        assert loop(cp) == ERR_INVALID_ARG and "icp_track_scans_sdf_color" in msg()
        assert same_state(before, geometry(ctx, c))
        # colours in the volume
        run(ctx, c)
        gb, cb = geometry(ctx, c), colours(ctx, c)
        ctx.set_source(scan)                           # a cloud without colours
        assert call() == ERR_COLOR_MISMATCH and "icp_tsdf_integrate_cloud_color" in msg()
        assert call(0) == 3 and call(2) == ERR_INVALID_ARG          # the call's own checks come first: no target; which
        bad = p.copy(); bad[13] = np.nan
        assert lib.icp_tsdf_integrate_cloud_color(ctx.h, 1, binding._ptr(bad), None, None, None) == ERR_INVALID_ARG and "finite" in msg()
        assert loop(None) == ERR_INVALID_ARG and "icp_track_scans_sdf_color" in msg() and loop(none) == ERR_INVALID_ARG and "null colours" in msg()
        with pytest.raises(binding.IcpError):
            ctx.tsdf_integrate_cloud("source", pose=TILTED, color=True)
        assert same_state(gb, geometry(ctx, c)) and same_state(cb, colours(ctx, c))
        # and the call goes through once the cloud has colours, NULL outputs allowed
        ctx.set_source(scan, None, rgba)
        assert lib.icp_tsdf_integrate_cloud_color(ctx.h, 1, binding._ptr(p), None, None, None) == OK
        assert not same_state(cb, colours(ctx, c))


def test_more_than_2_24_points_is_refused(gpu_ctx_factory):
    """A resident cloud of 2^24 + 1 coloured points (about 270 MB of upload): refused before any device work, the volume's bits unchanged;
    the time of the whole test is printed."""
    from icp_amd import binding
    t0 = time.time()
    ctx = gpu_ctx_factory()
    c = K.CASES["one_point/dense"]
    run(ctx, c)
    gb, cb = geometry(ctx, c), colours(ctx, c)
    n = (1 << 24) + 1
    pts = np.zeros((n, 3), f32); pts[:, 0] = 2.0
    ctx.set_source(pts, None, np.zeros((n, 4), np.uint8))
    p = binding.pose_to_c(EYE)
    nc = ctypes.c_int32(-1)
    assert ctx.lib.icp_tsdf_integrate_cloud_color(ctx.h, 1, binding._ptr(p), None, None, ctypes.byref(nc)) == ERR_INVALID_ARG
    m = ctx.lib.icp_last_error(ctx.h).decode()
    assert "icp_tsdf_integrate_cloud_color" in m and "2^24" in m and nc.value == 0
    assert same_state(gb, geometry(ctx, c)) and same_state(cb, colours(ctx, c))
    ctx.set_source(pts[:8], None, np.zeros((8, 4), np.uint8))      # (the large planes leave the context)
    print("2^24 + 1 points: refused; the test took %.2f s" % (time.time() - t0))


def test_outcome_model_mesh_and_ply(gpu_ctx_factory, tmp_path):
    """The twelve coloured scans: eth.fuse_scans(colors=...) equals the fixture's model bit for bit (whose conditions are asserted on the
    CPU); eth.reconstruct(colors=...) on both trackers returns a coloured mesh whose PLY reads back with the same colours."""
    from icp_amd import eth, meshio
    clouds, poses, normals = CF.scans()
    cols = OF.colours()
    vol, want = OF.model()
    ctx = gpu_ctx_factory()
    kw = dict(truncation=CF.TRUNCATION, origin=CF.ORIGIN, max_range=CF.MAX_RANGE, block_capacity=256)
    infos = eth.fuse_scans(ctx, clouds, poses, colors=cols, voxel_size=CF.VOXEL, **kw)
    assert [i.pop("n_colored") for i in infos] == [w[2] for w in want] and infos == [w[0] for w in want]
    S.tsdf_blocks_equal_restatement(ctx, vol, "outcome")
    assert same_state(ctx.tsdf_blocks(colors=True)[4:], KR.colors_of(vol))
    ctx.set_gicp_options(1e-3, 0)
    runs = (("sdf", dict(SOF.SDF_OPTIONS)), ("map", dict(voxel_size=0.25, hashed=True, n_iterations=30, min_valid=64)))
    for tracker, opts in runs:
        path = str(tmp_path / ("room_%s.ply" % tracker))
        tposes, recs, status, mesh = eth.reconstruct(ctx, list(zip(clouds, normals)), poses[0], colors=cols, tsdf_voxel_size=CF.VOXEL, mesh_path=path, tracker=tracker,
                                                     **kw, **opts)
        v, n, t, col = mesh
        print("reconstruct(tracker=%r, colors=...): status %d, %d vertices, %d triangles, %d coloured vertices" % (tracker, status, len(v), len(t), int((col[:, 3] == 255).sum())))
        assert len(tposes) == CF.N_SCANS and len(v) > 1000 and len(t) > 1000
        assert col.shape == (len(v), 4) and col.dtype == np.uint8 and (col[:, 3] == 255).any()
        back = meshio.load_ply_mesh(path, colors=True)
        assert same_bits(back[0], v) and np.array_equal(back[2], t) and np.array_equal(back[3], col)
