"""Host side of the RGB-D tracking path, no GPU needed: the new C entry points without a device, the ctypes structs against the C
header, the register budget of the depth kernels, and icp_amd/tum.py on a directory written by write_synthetic_sequence."""
import ctypes as C
import os
import shutil
import subprocess
import numpy as np
import pytest
from device_asm import device_asm, kernel_resources

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_depth_entry_points_without_device_or_context():
    from icp_amd import binding
    lib = binding.load_library()
    h = C.c_void_p()
    rc = lib.icp_ctx_create(0, C.byref(h))
    if rc == 0:
        lib.icp_ctx_destroy(h)
        pytest.skip("a HIP device is visible")
    assert rc == 9                                                  # ICP_ERR_NO_DEVICE
    cam = binding.depth_camera(np.eye(3), 4, 3); opt = binding.depth_options()
    d = np.zeros(12, np.float32); p = binding.pose_to_c(np.eye(4)); out = (binding.IcpTrackFrame * 1)(); n = C.c_int32(-1)
    assert lib.icp_set_target_depth(None, binding._ptr(d), None, C.byref(cam), C.byref(opt), C.byref(n)) == 1
    assert lib.icp_set_source_depth(None, binding._ptr(d), None, C.byref(cam), C.byref(opt), C.byref(n)) == 1
    assert lib.icp_track_depth_frames(None, binding._ptr(d), None, 1, C.byref(cam), C.byref(opt), C.byref(opt), None, binding._ptr(p), out) == 1


C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "icp_hip.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m));
int main(void) {
    printf("icp_depth_camera %zu\nicp_depth_options %zu\nicp_track_frame %zu\n", sizeof(icp_depth_camera), sizeof(icp_depth_options), sizeof(icp_track_frame));
    F(icp_depth_camera, fx) F(icp_depth_camera, fy) F(icp_depth_camera, cx) F(icp_depth_camera, cy) F(icp_depth_camera, width) F(icp_depth_camera, height) F(icp_depth_camera, extrinsics)
    F(icp_depth_options, keep_original_size) F(icp_depth_options, downsample_factor) F(icp_depth_options, max_distance) F(icp_depth_options, fix_color_index)
    F(icp_track_frame, n_src) F(icp_track_frame, iterations) F(icp_track_frame, status) F(icp_track_frame, initial_rmse) F(icp_track_frame, final_rmse) F(icp_track_frame, pose)
    return 0;
}
"""


def test_ctypes_structs_match_the_c_header(tmp_path):
    from icp_amd import binding
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"; src.write_text(C_LAYOUT); exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    facts = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    for name, cls in (("icp_depth_camera", binding.IcpDepthCamera), ("icp_depth_options", binding.IcpDepthOptions), ("icp_track_frame", binding.IcpTrackFrame)):
        assert int(facts[name]) == C.sizeof(cls), name
        for field, _ in cls._fields_:
            assert int(facts["%s.%s" % (name, field)]) == getattr(cls, field).offset, (name, field)


def test_depth_kernels_register_budget():
    """The depth-frame kernels (dev_depth.hpp) and k_backproject, which shares their arithmetic: no scratch, and few enough VGPRs for
    full occupancy of a memory-bound pass (<= 32: 16 waves per SIMD)."""
    seen = kernel_resources(device_asm())
    for prefix in ("13k_depth_count", "15k_depth_scatter", "18k_conv_from_source", "13k_backproject"):
        ks = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev" + prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        for name, f in ks.items():
            assert f["num_vgpr"] <= 32 and f["private_seg_size"] == 0, (name, f)


@pytest.fixture(scope="module")
def tum_dir(tmp_path_factory):
    pytest.importorskip("PIL")
    from icp_amd import tum
    d = str(tmp_path_factory.mktemp("tum"))
    written = tum.write_synthetic_sequence(d, 25, width=64, height=48, K=np.array([[52.5, 0, 31.5], [0, 52.5, 23.5], [0, 0, 1]]))
    return d, written


def test_frame_schedule_follows_reconstruct_room():
    """main.cpp:278-281: frame 0, then (i + 1) * frameStep while the frame exists and i <= iMax (iMax = 10: at most 12 frames)."""
    from icp_amd import tum
    assert tum.frame_schedule(798) == [0] + [10 * (i + 1) for i in range(11)]
    assert tum.frame_schedule(25) == [0, 10, 20]
    assert tum.frame_schedule(21, frame_step=10) == [0, 10, 20]
    assert tum.frame_schedule(20, frame_step=10) == [0, 10]
    assert tum.frame_schedule(5, frame_step=1, i_max=2) == [0, 1, 2, 3]


def test_depth_pngs_hold_the_quantised_depth(tum_dir):
    from PIL import Image
    from icp_amd import formats, synth
    d, written = tum_dir
    _, names = formats.read_tum_file_list(os.path.join(d, "depth.txt"))
    assert len(names) == 25
    K = np.array([[52.5, 0, 31.5], [0, 52.5, 23.5], [0, 0, 1]])
    for k in (0, 7, 24):
        raw = np.array(Image.open(os.path.join(d, names[k])))
        assert raw.dtype == np.uint16 and raw.shape == (48, 64)
        pts, _, _ = synth.depth_frame(synth.camera_pose(k), K, 64, 48, 0x7A11 + k, 0.05)
        z = pts[:, 2].astype(np.float64).reshape(48, 64)
        holes = ~np.isfinite(z)
        assert holes.any() and np.all(raw[holes] == 0)
        assert np.array_equal(raw[~holes].astype(np.int64), np.round(z[~holes] * 5000).astype(np.int64))
        assert np.array_equal(written["depth"][k].view(np.uint32), formats.decode_tum_depth(raw).view(np.uint32))


def test_load_sequence_schedule_and_ground_truth(tum_dir):
    from icp_amd import tum
    d, written = tum_dir
    seq = tum.load_sequence(d)
    assert seq["frames"] == [0, 10, 20] and seq["depth"].shape == (3, 48, 64) and seq["rgbx"].shape == (3, 48 * 64, 4)
    assert np.array_equal(seq["depth"][1].view(np.uint32), written["depth"][10].view(np.uint32))
    # trajectory = readTrajectoryFile's inverted pose; gt_k = targetTrajectory * trajectory_k^-1 (main.cpp:298-300) = T_0^-1 T_k
    for i, k in enumerate(seq["frames"]):
        assert np.abs(seq["trajectory"][i] @ written["poses"][k] - np.eye(4)).max() < 1e-5
    for i, k in enumerate(seq["frames"][1:]):
        want = np.linalg.inv(written["poses"][0]) @ written["poses"][k]
        assert np.abs(seq["gt"][i] - want).max() < 1e-5
        assert np.abs(seq["gt"][i] - seq["trajectory"][0] @ np.linalg.inv(seq["trajectory"][i + 1])).max() < 1e-6
    seq2 = tum.load_sequence(d, frame_step=3, i_max=2)
    assert seq2["frames"] == [0, 3, 6, 9] and len(seq2["gt"]) == 3


def test_reconstruct_room_options():
    """Target keepOriginalSize = projective matching, factor 1 (main.cpp:201-207); source (true, 1) with multi-resolution, else
    (false, 8) (:287-292); 35 iterations and setMatchingMaxDistance(0.1) (:227-250)."""
    from icp_amd import binding, tum
    p = binding.IcpParams()
    for matching, multires, want_t, want_s in ((0, 0, (0, 1), (0, 8)), (1, 0, (1, 1), (0, 8)), (0, 1, (0, 1), (1, 1)), (1, 1, (1, 1), (1, 1))):
        p.matching, p.multires = matching, multires
        t, s = tum.reconstruct_room_options(p)
        assert (t.keep_original_size, t.downsample_factor) == want_t and (s.keep_original_size, s.downsample_factor) == want_s
        assert np.float32(t.max_distance) == np.float32(0.1) and np.float32(s.max_distance) == np.float32(0.1)
        assert t.fix_color_index == 0 and s.fix_color_index == 0
    p.matching = 1
    tum.reconstruct_room_params(p)
    assert p.n_iterations == 35 and np.float32(p.max_distance) == np.float32(0.1)
    assert (p.fx, p.fy, p.cx, p.cy, p.width, p.height) == (525.0, 525.0, 319.5, 239.5, 640, 480)


def test_track_applies_reconstruct_room_settings(tum_dir):
    """tum.track runs the variant with what reconstructRoom sets on top of it (main.cpp:227-250): 35 iterations, max distance 0.1 and,
    for projective matching, the sequence's camera; the clouds follow the options of main.cpp:201-207,287-292."""
    from icp_amd import binding, tum
    d, _ = tum_dir
    seq = tum.load_sequence(d, K=np.array([[52.5, 0, 31.5], [0, 52.5, 23.5], [0, 0, 1]]))       # the camera the directory was written with

    class FakeCtx:                                       # records what track hands to the library
        def __init__(self):
            self.params = binding.IcpParams(); self.pushed = None
        def push_params(self):
            self.pushed = (self.params.n_iterations, self.params.max_distance, self.params.fx, self.params.cx, self.params.width, self.params.height)
        def track_depth_frames(self, depth, rgbx, cam, to, so, gt=None, pose=None):
            self.call = (cam.fx, cam.width, cam.height, to.keep_original_size, so.downsample_factor, len(gt))
            return np.eye(4, dtype=np.float32), [dict(pose=np.eye(4, dtype=np.float32))] * (len(depth) - 1), 0

    ctx = FakeCtx()
    p = binding.IcpParams(); p.matching = 1; p.n_iterations = 7; p.max_distance = 0.0003
    poses, recs, rc = tum.track(ctx, seq, p)
    n_it, md, fx, cx, w, h = ctx.pushed
    assert n_it == 35 and np.float32(md) == np.float32(0.1) and (w, h) == (64, 48)
    assert np.float32(fx) == np.float32(52.5) and np.float32(cx) == np.float32(31.5)
    assert ctx.call == (np.float32(52.5), 64, 48, 1, 8, 2) and len(poses) == 3 and rc == 0
