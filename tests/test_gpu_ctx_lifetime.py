"""What a context owns goes away with it: create -> use -> destroy leaves the library's device bytes (icp_debug_live_bytes: its own
allocations, process-wide, views not counted) where they were, for every family of buffers a context can come to hold -- levels and
their packs, the sampling caches, the per-metric caches, the optimiser's and the multi-start's slices, the features, the depth slots, the
TSDF volume and the meshes' scratch -- and across a regrow of the buffers that others are views of.  The library against itself and the
counter against itself; results are pinned by the other suites."""
import ctypes as C
import gc

import numpy as np
import pytest

from support import bits

pytestmark = pytest.mark.gpu
f32 = np.float32
LBVH = 1
SELECT_RANDOM, SELECT_NORMAL_SPACE = 1, 2
POINT_TO_PLANE, GICP, COLORED = 1, 3, 4


def live():
    from icp_amd import binding
    v = C.c_int64(0)
    assert binding.load_library().icp_debug_live_bytes(C.byref(v)) == 0
    return v.value


def settled():
    """The counter with no context of an earlier test waiting to be collected."""
    gc.collect()
    return live()


def configure(c, **kw):                                         # not support.configure: this one starts from default_params()
    """The defaults, k-NN on the LBVH backend, point-to-plane, a threshold in metres; then what the case asks for."""
    from icp_amd import binding
    c.params = binding.default_params()
    c.params.knn_backend = LBVH; c.params.metric = POINT_TO_PLANE; c.params.max_distance = 10.0; c.params.n_iterations = 4
    for k, v in kw.items():
        setattr(c.params, k, v)
    c.push_params()


@pytest.fixture(scope="module")
def scans():
    from icp_amd import synth
    return synth.eth_like_pair(0, n_tilt=30, n_beam=100)        # ~3,000 points each, normals and colours


def test_every_buffer_family_then_destroy(scans):
    from icp_amd import binding
    p = scans
    before = settled()
    c = binding.Context(0)
    eye = np.eye(4)
    configure(c)
    c.set_target(p["tgt_pts"], p["tgt_nrm"], p["tgt_rgba"]); c.set_source(p["src_pts"], p["src_nrm"], p["src_rgba"])
    configure(c, multires=1)                                     # levels, their orders and sorted packs; the merged ring
    _, recs, _ = c.run(eye)
    assert len(recs) > 4
    for resample in (False, True):                               # normal-space sampling: a held draw (a level of its own), then resampling
        c.set_nss_options(resample=resample)
        configure(c, multires=1, selection=SELECT_NORMAL_SPACE, selection_proba=0.5, selection_seed=7)
        c.run(eye)
        assert len(c.selection(0)) > 0
    configure(c, selection=SELECT_RANDOM, selection_proba=0.5, selection_seed=7)
    c.run(eye)
    c.set_gicp_options(k=20)
    configure(c, metric=GICP)
    c.run(eye)
    configure(c, metric=COLORED)
    c.run(eye)
    configure(c)
    c.set_optimizer(True)                                        # the non-linear optimiser's state, partials and records
    c.run(eye)
    assert len(c.lm_summaries()) == 4
    c.set_optimizer(None)
    c.set_convergence_options(1e-3, 1e-3)                        # the run block's longer tail
    configure(c, n_iterations=12)
    c.run(eye)
    assert len(c.convergence_trace()) >= 1
    c.set_convergence_options(None)
    configure(c)
    results, _, best = c.run_multistart([eye, p["gt"]])
    assert len(results) == 2 and best in (0, 1)
    c.compute_features("both")
    c.register_global(check=False)
    nrm, _ = c.estimate_normals(p["src_pts"])
    assert np.isfinite(nrm).any()
    assert live() > before + 10 * len(p["tgt_pts"]) * 4        # (the two clouds' planes alone are more)
    c.close()
    assert live() == before


@pytest.fixture(scope="module")
def frames():
    """Three 64 x 48 frames of the synthetic hand-held camera: depth (MINF holes), RGBX bytes, gt transforms frame k -> frame 0."""
    from icp_amd import synth
    K, depth, rgbx, gt = synth.camera_sequence(3, 64, 48)
    return K, 64, 48, depth, rgbx, gt


def test_depth_and_model_paths_then_destroy(frames):
    """The depth slots and their page-locked blocks, the second stream, the tracked frames' RMSE bracket, the volume and both meshes'
    scratch.  Twice: destroy with the volume still there, then destroy after icp_tsdf_release (nothing is counted twice)."""
    from icp_amd import binding
    K, W, H, depth, rgbx, gt = frames
    volume = 32 ** 3 * 8
    for release_first in (False, True):
        before = settled()
        c = binding.Context(0)
        configure(c, max_distance=0.1, n_iterations=6)
        cam = binding.depth_camera(K, W, H)
        _, recs, _ = c.track_depth_frames(depth, rgbx, cam, binding.depth_options(False, 1), binding.depth_options(False, 2), gt=gt)
        assert len(recs) == 2 and recs[0]["n_src"] > 0 and recs[0]["initial_rmse"] >= 0
        c.tsdf_create(dims=(32, 32, 32), origin=(-4.0, -4.0, -1.0), voxel_size=0.25, truncation=0.75)
        _, recs, _ = c.track_depth_model(depth, cam, binding.depth_options(False, 2), gt=gt)
        assert len(recs) == 2 and recs[0]["n_src"] > 0
        verts, _, tris = c.tsdf_mesh()
        assert len(verts) > 0 and len(tris) > 0
        _, cols, _ = c.depth_mesh(depth[0], rgbx[0], cam, np.eye(4))
        assert cols is not None
        held = live()
        assert held > before + volume
        if release_first:
            c.tsdf_release()
            assert before < live() <= held - volume              # the volume and the mesh scratch have gone, the rest is still held
        c.close()
        assert live() == before, release_first


def test_views_across_a_regrow():
    """A 1,000-point source, a run, then a 5,000-point source and a run: the search-state pack regrows and its three views are re-pointed,
    the sorted levels' packs (ten views each) are dropped and rebuilt.  The second run equals a fresh context's, and destroy frees each
    pack once."""
    from icp_amd import binding, synth
    big = synth.eth_like_pair(0, n_tilt=43, n_beam=135)
    assert len(big["src_pts"]) >= 5000
    small = (big["src_pts"][::5][:1000], big["src_nrm"][::5][:1000])
    large = (big["src_pts"][:5000], big["src_nrm"][:5000])
    before = settled()
    a, b = binding.Context(0), binding.Context(0)
    for c in (a, b):
        configure(c, multires=1, n_iterations=6)
        c.set_target(big["tgt_pts"], big["tgt_nrm"])
    a.set_source(*small)
    a.run(np.eye(4))
    a.set_source(*large)
    pose_a, recs_a, _ = a.run(np.eye(4))
    b.set_source(*large)
    pose_b, recs_b, _ = b.run(np.eye(4))
    assert len(recs_a) == len(recs_b) and len({r["n_src"] for r in recs_b}) >= 6      # one sorted level per factor 32 .. 1
    for k, (ra, rb) in enumerate(zip(recs_a, recs_b)):
        assert (ra["n_src"], ra["n_valid"]) == (rb["n_src"], rb["n_valid"]), k
        assert np.array_equal(bits(ra["pose"]), bits(rb["pose"])), k
    assert np.array_equal(bits(pose_a), bits(pose_b))
    a.close(); b.close()
    assert live() == before
