"""The bilateral depth filter on the device: icp_filter_depth bit for bit against the numpy restatement on every
shape around the kernel's tile, the resident path against the host path (filter the frame with icp_filter_depth, hand it to a context
whose filter is off), who reads the filtered frame and who the raw one, and the outcome fixture's figures."""
import ctypes as C
import json
import numpy as np
import pytest

import depth_filter_restatement as DF
import depth_filter_outcome_fixture as XF
import tsdf_outcome_fixture as OF
import support as S
from support import same_bits
from icp_amd import binding
from icp_amd.synth import camera_sequence

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
TW, TH = binding.DEPTH_FILTER_TILE
# (width, height): smaller than the radius; one tile exactly; one tile plus a pixel in each direction; two tiles by two; odd; a real frame
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 2), (TW, TH), (TW + 1, TH), (TW, TH + 1), (TW + 1, TH + 1), (2 * TW, 2 * TH), (37, 29), (320, 240)]
RADII = [1, 2, 3, 4]
ON = dict(radius=3, sigma_space=4.5, sigma_range=0.03)
ROOM = dict(origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
ROOM_DENSE = dict(dims=(71, 35, 89), **ROOM)
RECORD_KEYS = ("n_depth", "n_valid_first", "n_valid_last", "iterations", "status")
W, H, N_FRAMES = 80, 60, 6


def same_image(a, b):
    """Bit for bit, NaNs compared as NaNs."""
    a = np.ascontiguousarray(a, f32); b = np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_record(a, b):
    keys = [k for k in a if k not in ("pose", "pad") and not k.startswith("cost")]
    return set(RECORD_KEYS) <= set(keys) and all(a[k] == b[k] for k in keys) and all(u64(a[k]) == u64(b[k]) for k in a if k.startswith("cost")) \
        and same_bits(a["pose"], b["pose"])


def noisy_plane(w, h, seed, base=1.5, holes=0.05):
    r = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = (base * (1.0 + 0.0013 * u + 0.0007 * v + r.normal(0, 0.002, (h, w)))).astype(f32)
    d[r.random((h, w)) < holes] = MINF
    return d


def seam_spots(w, h):
    """Corners, and the pixels on both sides of the first tile seam in x and in y (where the image has them)."""
    xs = sorted({0, w - 1} | {x for x in (TW - 1, TW) if x < w})
    ys = sorted({0, h - 1} | {y for y in (TH - 1, TH) if y < h})
    return [(x, y) for y in ys for x in xs]


# A pair of depths whose t is 256.0f to the bit under the library's inv_bin for CUT_SIGMA (the sixth float above 0.03, found by a search over
# sigma_range and the depth difference; both depths are multiples of 2^-24 in [0.5, 1), so their difference is exact), and one a float below.
CUT_SIGMA, CUT_C, CUT_N = 0.03000001050531864, f32(0.5), f32(0.5900000333786011)


def cut_pair():
    """(sigma_range, c, n at the cut, n one float below it), checked: t(n) == 256.0f exactly, t(n below) < 256.0f."""
    ib = binding.depth_filter_tables(radius=1, sigma_range=CUT_SIGMA)[2]
    t = lambda n: f32(f32(f32(n - CUT_C) * f32(n - CUT_C)) * ib)
    below = np.nextafter(CUT_N, f32(0))
    assert f32(CUT_SIGMA) == CUT_SIGMA and t(CUT_N) == f32(256.0) and t(below) < f32(256.0) and int(t(below)) == 255
    return CUT_SIGMA, CUT_C, CUT_N, below


def contents(w, h, seed):
    """(name, frame, sigma_range) of every content class, for one shape."""
    out = [("noisy plane, 5 % holes", noisy_plane(w, h, seed), 0.03), ("all holes", np.full((h, w), MINF, f32), 0.03)]
    d = noisy_plane(w, h, seed + 1, holes=0.0)
    specials = [f32(np.nan), f32(np.inf), f32(0), f32(-0.75), MINF, f32(-0.0)]
    for k, (x, y) in enumerate(seam_spots(w, h)):          # unusable values as centres, their usable neighbours see them as neighbours
        if k % 2 == 0:
            d[y, x] = specials[(k // 2) % len(specials)]
    out.append(("NaN, +inf, 0, negatives at corners and seams", d, 0.03))
    d = noisy_plane(w, h, seed + 2, holes=0.0)
    for k, (x, y) in enumerate(seam_spots(w, h)):          # the other half of the spots: every seam pixel is once the unusable one
        if k % 2 == 1:
            d[y, x] = specials[(k // 2) % len(specials)]
    out.append(("the same on the other side of the seams", d, 0.03))
    out.append(("depths around 1e-3", noisy_plane(w, h, seed + 3, base=1e-3), 0.03))
    out.append(("depths around 1e3", noisy_plane(w, h, seed + 4, base=1e3), 0.03))
    out.append(("every neighbour cut", noisy_plane(w, h, seed + 5), 1e-6))
    if w * h >= 2:
        sr, c, at, below = cut_pair()
        for name, other in (("t == 256.0f exactly", at), ("t one float below 256", below)):
            d = np.full((h, w), MINF, f32)
            d.flat[0] = c; d.flat[1] = other               # (0, 0) and its right neighbour, or the pixel below it in a 1-wide image
            out.append((name, d, sr))
    return out


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_filter_depth_equals_restatement_bit_for_bit(ctx, shape, radius):
    w, h = shape
    for name, d, sr in contents(w, h, 100 * w + h):
        Sp, R, ib = binding.depth_filter_tables(radius=radius, sigma_range=sr)
        want = DF.filter_depth(d, radius, Sp, R, ib)
        got = ctx.filter_depth(d, radius=radius, sigma_range=sr)
        assert same_image(got, want), (name, shape, radius, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
        assert same_image(ctx.filter_depth(d, radius=0), d), name
    if w * h >= 2:                                           # the cut itself: at t == 256.0f the pair is apart, a float below it is averaged
        sr, c, at, below = cut_pair()
        cut = ctx.filter_depth(contents(w, h, 0)[-2][1], radius=radius, sigma_range=sr)
        near = ctx.filter_depth(contents(w, h, 0)[-1][1], radius=radius, sigma_range=sr)
        assert cut.flat[0] == c and abs(float(cut.flat[1]) - float(at)) < 1e-6               # (R[0] * 0.5 is exact; R[0] * n is rounded once)
        assert c + 1e-4 < near.flat[0] < near.flat[1] < at - 1e-4                               # the neighbour enters with S * R[255], about 0.011


def test_context_options_and_refusals(gpu_ctx_factory):
    c = gpu_ctx_factory()
    o = c.depth_filter_options()
    assert (o.radius, f32(o.sigma_space), f32(o.sigma_range)) == (0, f32(4.5), f32(0.03))
    d = noisy_plane(45, 19, 7)
    assert same_image(c.filter_depth(d), d)                 # off: a copy
    c.set_depth_filter(radius=2, sigma_space=2.0, sigma_range=0.01)
    o = c.depth_filter_options()
    assert (o.radius, f32(o.sigma_space), f32(o.sigma_range)) == (2, f32(2.0), f32(0.01))
    want = DF.filter_depth(d, 2, *binding.depth_filter_tables(o))
    assert same_image(c.filter_depth(d), want)              # NULL options: the context's
    other = c.filter_depth(d, radius=4)                     # options of the call: the context's stay, and its next frame is filtered with them
    assert same_image(other, DF.filter_depth(d, 4, *binding.depth_filter_tables(radius=4))) and not same_image(other, want)
    assert same_image(c.filter_depth(d), want) and c.depth_filter_options().radius == 2
    for bad in (dict(radius=5), dict(radius=-1), dict(sigma_space=0.0), dict(sigma_range=float("nan")), dict(sigma_range=1e-19)):
        with pytest.raises(binding.IcpError) as e:
            c.set_depth_filter(**dict(dict(radius=2), **bad))
        assert e.value.code == 1
        with pytest.raises(binding.IcpError):
            c.filter_depth(d, **dict(dict(radius=2), **bad))
    assert c.depth_filter_options().radius == 2             # a refused call changes nothing
    assert c.lib.icp_set_depth_filter_options(c.h, None) == 0 and c.depth_filter_options().radius == 0      # NULL: the defaults
    out = np.empty_like(d)
    assert c.lib.icp_filter_depth(c.h, None, 45, 19, None, binding._ptr(out)) == 1 and c.lib.icp_filter_depth(c.h, binding._ptr(d), 0, 19, None, binding._ptr(out)) == 1


def get_cloud(c, which):
    """The resident target (0) or source (1): (n, planes (6, n) or (3, n), rgba (n,) or None)."""
    fn = c.lib.icp_debug_get_cloud
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    n, fl = C.c_int32(0), C.c_int32(0)
    assert fn(c.h, which, None, None, 0, C.byref(n), C.byref(fl)) == 0
    planes = np.zeros((6, n.value), f32); rgba = np.zeros(n.value, np.uint32)
    assert fn(c.h, which, binding._ptr(planes), binding._ptr(rgba), n.value, C.byref(n), C.byref(fl)) == 0
    return n.value, planes[:6 if fl.value & 1 else 3], (rgba if fl.value & 2 else None)


def same_cloud(a, b):
    return a[0] == b[0] and same_image(a[1], b[1]) and ((a[2] is None and b[2] is None) or np.array_equal(a[2], b[2]))


def noisy_sequence(n=N_FRAMES):
    K, depth, rgbx, gt = camera_sequence(n, W, H, sigma=0.002)
    return K, depth, rgbx, gt, binding.depth_camera(K, W, H)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("factor", [1, 8])
def test_resident_clouds_equal_host_filtered_frames(gpu_ctx_factory, factor, keep):
    """Filter on + the raw frame == filter off + the frame icp_filter_depth gave: points, normals, colours and kept count of both clouds."""
    K, depth, rgbx, _, cam = noisy_sequence(2)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    a.set_depth_filter(**ON)
    opt = binding.depth_options(keep, factor, 0.1, True)
    for cols in (None, rgbx):
        for k, (set_a, set_b) in enumerate(((a.set_target_depth, b.set_target_depth), (a.set_source_depth, b.set_source_depth))):
            d = depth[k]; c = None if cols is None else cols[k]
            filt = a.filter_depth(d)
            assert not same_image(filt, d)
            na = set_a(d, c, cam, opt); nb = set_b(filt, c, cam, opt)
            ca, cb = get_cloud(a, k), get_cloud(b, k)
            assert na == nb == ca[0] and same_cloud(ca, cb), (factor, keep, k, cols is not None)
            assert (ca[2] is not None) == (cols is not None) and ca[1].shape[0] == 6
            nr = b.set_target_depth(d, c, cam, opt) if k == 0 else b.set_source_depth(d, c, cam, opt)     # the raw frame gives another cloud
            assert not same_cloud(get_cloud(b, k), ca) or nr != na


def make_volume(c, storage, color=False):
    if getattr(c, "has_volume", False):
        c.tsdf_release()
    c.has_volume = True
    if storage == "hashed":
        c.tsdf_create_hashed(block_capacity=64, color=color, **ROOM)
    else:
        c.tsdf_create(color=color, **ROOM_DENSE)


def volume_bits(c, storage, color=False):
    if storage == "hashed":
        got = c.tsdf_blocks(colors=True) if color else c.tsdf_blocks()
        return [np.ascontiguousarray(x).view(np.uint8) for x in got[1:]]
    out = list(c.tsdf_volume()) + (list(c.tsdf_color_volume()) if color else [])
    return [np.ascontiguousarray(x).view(np.uint8) for x in out]


def same_volume(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["dense", "hashed", "dense_color", "hashed_color"])
def test_sdf_calls_read_the_filtered_frame_and_fusion_the_raw_one(gpu_ctx_factory, case):
    """a: filter on, raw frames.  b: filter off, icp_filter_depth's frames where a frame is aligned, raw frames where it is fused.  The sums
    of icp_tsdf_sdf_system, and the pose, record and trace of icp_tsdf_align_depth, are the same; so is the volume after the integrates."""
    storage, color = case.split("_")[0], case.endswith("color")
    K, depth, rgbx, gt, cam = noisy_sequence(3)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    a.set_depth_filter(**ON)
    eye = np.eye(4, dtype=f32)
    ckw = dict(color_weight=0.1) if color else {}
    for c in (a, b):
        make_volume(c, storage, color)
        for k in (0, 1):
            c.tsdf_integrate(depth[k], cam, eye if k == 0 else gt[0], rgbx=rgbx[k] if color else None)
    assert same_volume(volume_bits(a, storage, color), volume_bits(b, storage, color))       # fusion reads raw
    filt = a.filter_depth(depth[2])
    for pose in (eye, gt[1]):
        for stride in (1, 3):
            sa, ca = a.tsdf_sdf_system(depth[2], cam, pose, stride=stride, rgbx=rgbx[2] if color else None, **ckw)
            sb, cb = b.tsdf_sdf_system(filt, cam, pose, stride=stride, rgbx=rgbx[2] if color else None, **ckw)
            sr, cr = b.tsdf_sdf_system(depth[2], cam, pose, stride=stride, rgbx=rgbx[2] if color else None, **ckw)
            assert ca == cb and np.array_equal(u64(sa), u64(sb)) and ca[1] > 50, (case, stride)
            assert not np.array_equal(u64(sa), u64(sr))     # ... and not what the raw frame gives
    pa, ra, rca, ta = a.tsdf_align_depth(depth[2], cam, gt[0], trace=True, n_iterations=8, rgbx=rgbx[2] if color else None, **ckw)
    pb, rb, rcb, tb = b.tsdf_align_depth(filt, cam, gt[0], trace=True, n_iterations=8, rgbx=rgbx[2] if color else None, **ckw)
    assert rca == rcb == 0 and same_bits(pa, pb) and same_record(ra, rb) and len(ta) == len(tb) > 0
    for x, y in zip(ta, tb):
        assert x["n_valid"] == y["n_valid"] and x["status"] == y["status"] and u64(x["cost"]) == u64(y["cost"]) and same_bits(x["pose"], y["pose"])
    assert same_volume(volume_bits(a, storage, color), volume_bits(b, storage, color))       # the aligns changed nothing


def composed_sdf_loop(c, depth, cam, **kw):
    """icp_track_depth_sdf as a composition of public calls: integrate(raw_0), then per frame align(raw_k) -- filtered by the context when its
    filter is on -- and integrate(raw_k)."""
    pose = np.eye(4, dtype=f32)
    c.tsdf_integrate(depth[0], cam, pose)
    recs = []
    for k in range(1, len(depth)):
        pose, rec, rc = c.tsdf_align_depth(depth[k], cam, pose, **kw)
        if rc == 0:
            c.tsdf_integrate(depth[k], cam, pose)
        recs.append(rec)
    return pose, recs


@pytest.mark.parametrize("storage", ["dense", "hashed"])
def test_track_depth_sdf_equals_the_composition(gpu_ctx_factory, storage):
    """6 frames of 80 x 60 with 2 mm of depth noise: icp_track_depth_sdf == integrate(raw_0), then align(raw_k) and integrate(raw_k) per frame,
    poses, records and the volume bit for bit -- with the filter on, and with it off as the control (which the parent commit passes too:
    tests/test_gpu_sdf.py and tests/test_gpu_htsdf.py assert it on 5 frames of 40 x 30)."""
    K, depth, _, gt, cam = noisy_sequence()
    kw = dict(stride=1, n_iterations=12)
    poses = {}
    for on in (False, True):
        a, b = gpu_ctx_factory(), gpu_ctx_factory()
        for c in (a, b):
            if on:
                c.set_depth_filter(**ON)
            make_volume(c, storage)
        pose, recs, rc = a.track_depth_sdf(depth, cam, **kw)
        ref_pose, ref = composed_sdf_loop(b, depth, cam, **kw)
        assert rc == 0 and len(recs) == N_FRAMES - 1 and all(r["status"] == 0 for r in recs)
        for k, (r, h) in enumerate(zip(recs, ref)):
            assert same_record(r, h), (storage, on, k, r, h)
        assert same_bits(pose, ref_pose) and same_volume(volume_bits(a, storage), volume_bits(b, storage)), (storage, on)
        for r, g in zip(recs, gt):
            e = OF.pose_error(r["pose"], g)
            assert e[0] < 0.05 and e[1] < 0.1, e
        poses[on] = [r["pose"] for r in recs]
    assert not all(same_bits(x, y) for x, y in zip(poses[False], poses[True]))       # the filter took part


@pytest.mark.parametrize("storage", ["dense", "hashed"])
def test_model_loop_aligns_filtered_and_fuses_raw(gpu_ctx_factory, storage):
    """icp_track_depth_model / _hashed with the filter on: the source left resident is set_source_depth of the last frame FILTERED, and the
    model is what integrating the RAW frames at the returned poses gives."""
    K, depth, _, gt, cam = noisy_sequence()
    so = binding.depth_options(False, 2)
    a, b, off = gpu_ctx_factory(), gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b, off):
        S.configure(c, n_iterations=20, max_distance=0.1, seed=0)
        make_volume(c, storage)
    a.set_depth_filter(**ON)
    track = (lambda c: c.track_depth_model_hashed(depth, cam, so)) if storage == "hashed" else (lambda c: c.track_depth_model(depth, cam, so))
    pose, recs, rc = track(a)
    assert rc == 0 and all(r["status"] == 0 for r in recs)
    n = b.set_source_depth(a.filter_depth(depth[-1]), None, cam, so)
    assert n == recs[-1]["n_src"] and same_cloud(get_cloud(a, 1), get_cloud(b, 1))
    b.tsdf_integrate(depth[0], cam, np.eye(4, dtype=f32))
    for k, r in enumerate(recs, 1):
        b.tsdf_integrate(depth[k], cam, r["pose"])
    assert same_volume(volume_bits(a, storage), volume_bits(b, storage))
    _, recs_off, _ = track(off)
    assert not all(same_bits(x["pose"], y["pose"]) for x, y in zip(recs, recs_off))          # the filter took part


def test_radius_zero_is_a_context_that_never_heard_of_the_filter(gpu_ctx_factory):
    """a: the filter switched on, used, and off again (radius 0).  b: untouched.  Every call above returns the same."""
    K, depth, rgbx, gt, cam = noisy_sequence()
    so = binding.depth_options(False, 2)
    eye = np.eye(4, dtype=f32)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    a.set_depth_filter(**ON)
    a.set_source_depth(depth[0], None, cam, so)
    a.set_depth_filter(radius=0)
    for c in (a, b):
        S.configure(c, n_iterations=20, max_distance=0.1, seed=0)
    assert same_image(a.filter_depth(depth[0]), depth[0])
    for k, name in ((0, "set_target_depth"), (1, "set_source_depth")):
        na = getattr(a, name)(depth[k], rgbx[k], cam, so); nb = getattr(b, name)(depth[k], rgbx[k], cam, so)
        assert na == nb and same_cloud(get_cloud(a, k), get_cloud(b, k))
    pa, ra, rca = a.track_depth_frames(depth, rgbx, cam, binding.depth_options(False, 1), so)
    pb, rb, rcb = b.track_depth_frames(depth, rgbx, cam, binding.depth_options(False, 1), so)
    assert rca == rcb and same_bits(pa, pb) and all(same_bits(x["pose"], y["pose"]) for x, y in zip(ra, rb))
    for storage in ("dense", "hashed"):
        for c in (a, b):
            make_volume(c, storage)
            c.tsdf_integrate(depth[0], cam, eye)
        sa, ca = a.tsdf_sdf_system(depth[1], cam, eye); sb, cb = b.tsdf_sdf_system(depth[1], cam, eye)
        assert ca == cb and np.array_equal(u64(sa), u64(sb))
        xa = a.tsdf_align_depth(depth[1], cam, eye, n_iterations=8); xb = b.tsdf_align_depth(depth[1], cam, eye, n_iterations=8)
        assert xa[2] == xb[2] and same_bits(xa[0], xb[0]) and same_record(xa[1], xb[1])
        assert same_volume(volume_bits(a, storage), volume_bits(b, storage))
        for c in (a, b):
            make_volume(c, storage)
        ta = a.track_depth_sdf(depth, cam, n_iterations=12); tb = b.track_depth_sdf(depth, cam, n_iterations=12)
        assert ta[2] == tb[2] and all(same_record(x, y) for x, y in zip(ta[1], tb[1])) and same_volume(volume_bits(a, storage), volume_bits(b, storage))
        for c in (a, b):
            make_volume(c, storage)
        track = (lambda c: c.track_depth_model_hashed(depth, cam, so)) if storage == "hashed" else (lambda c: c.track_depth_model(depth, cam, so))
        ma, mb = track(a), track(b)
        assert ma[2] == mb[2] and all(same_bits(x["pose"], y["pose"]) and x["iterations"] == y["iterations"] for x, y in zip(ma[1], mb[1]))
        assert same_volume(volume_bits(a, storage), volume_bits(b, storage)) and same_cloud(get_cloud(a, 1), get_cloud(b, 1))


def test_tum_track_sets_the_filter_for_the_call_and_puts_the_previous_one_back(gpu_ctx_factory):
    from icp_amd import tum
    K, depth, rgbx, gt, cam = noisy_sequence(4)
    seq = dict(depth=depth, rgbx=rgbx, gt=gt, K=K, width=W, height=H)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    a.set_depth_filter(radius=1, sigma_space=2.0, sigma_range=0.02)
    b.set_depth_filter(**ON)
    pa, ra, rca = tum.track(a, seq, with_gt=False, model=ROOM_DENSE, sdf=dict(n_iterations=12), depth_filter=ON)
    o = a.depth_filter_options()
    assert (o.radius, f32(o.sigma_space), f32(o.sigma_range)) == (1, f32(2.0), f32(0.02))
    pb, rb, rcb = tum.track(b, seq, with_gt=False, model=ROOM_DENSE, sdf=dict(n_iterations=12))           # None: the context's own setting, untouched
    assert b.depth_filter_options().radius == 3
    assert rca == rcb == 0 and all(same_record(x, y) for x, y in zip(ra, rb))


def test_outcome_normals_equal_the_fixture(gpu_ctx_factory):
    """The fixture's noisy frame filtered and back-projected on the device: the restatement's figures to the digit (the filter's output is
    bit-identical, and so is the back-projection)."""
    with open(XF.GOLDEN) as f:
        ref = json.load(f)["normals"]
    K, depth, _, nrm_true = XF.noisy_frames(n_frames=1)
    c = gpu_ctx_factory()
    filt = c.filter_depth(depth[0], **XF.FILTER)
    assert same_image(filt, XF.restatement_filter(depth[0]))
    n_raw = c.backproject_depth(depth[0], None, K, max_distance=XF.MAX_DISTANCE)[1]
    n_filt = c.backproject_depth(filt, None, K, max_distance=XF.MAX_DISTANCE)[1]
    a_raw, a_filt, k_raw, k_filt = XF.normal_measures(n_raw, n_filt, nrm_true)
    print("normals on the device: raw %.5f rad / %d kept, filtered %.5f rad / %d kept" % (a_raw, k_raw, a_filt, k_filt))
    assert (k_raw, k_filt) == (ref["raw_kept"], ref["filtered_kept"])
    assert a_raw == ref["raw_mean_angle_rad"] and a_filt == ref["filtered_mean_angle_rad"]
    assert a_filt < a_raw and k_filt >= k_raw


def test_outcome_on_the_noisy_pan(gpu_ctx_factory):
    """The fixture's 41-frame pan with 2 mm of depth noise through tum.track with the model, sdf=dict(stride=4, n_iterations=20) and the
    filter at radius 3.  Figures of the restatement (tests/golden/depth_filter_outcome.json; worst frame, rotation [rad] / translation [m]):
      raw 0.0076 / 0.0399, filtered 0.0076 / 0.0409 -- no gain on this sequence: the direct tracker averages thousands of pixels.
    The bound is TWICE the restatement's filtered figures, the margin the other outcome tests give a device run over its restatement; the
    device's own figures are printed next to it."""
    from icp_amd import tum
    with open(XF.GOLDEN) as f:
        ref = json.load(f)
    K, depth, gt, _ = XF.noisy_frames()
    seq = dict(depth=depth, rgbx=None, gt=gt, K=K, width=OF.W, height=OF.H)
    c = gpu_ctx_factory()
    out = {}
    for name, filt in (("raw", None), ("filtered", XF.FILTER)):
        poses, recs, rc = tum.track(c, seq, with_gt=False, model=OF.VOLUME, sdf=dict(XF.OPTIONS), depth_filter=filt)
        assert rc == 0 and all(r["status"] == 0 for r in recs) and len(recs) == OF.N_FRAMES - 1
        out[name] = OF.worst_errors([np.eye(4)] + [r["pose"] for r in recs], gt)[:2]
        print("%s: restatement worst %.4f rad / %.4f m; device worst %.4f rad / %.4f m" % (name, ref[name]["worst_rotation_rad"], ref[name]["worst_translation_m"], *out[name]))
    assert c.depth_filter_options().radius == 0
    assert out["filtered"][0] <= 2 * ref["filtered"]["worst_rotation_rad"] and out["filtered"][1] <= 2 * ref["filtered"]["worst_translation_m"]
