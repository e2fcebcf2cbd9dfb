"""Laser scans into the TSDF volume on the host side, no device: the numpy restatement of the contract
(tests/tsdf_cloud_restatement.py) against one plain loop per ray, its independence of the order of the points, the integer accumulators
on repeated points, the rule that drops a repeated voxel, the outcome fixture's surface conditions, and the struct, the symbol, the
Python surface and the refusals that need no device."""
import ctypes
import inspect
import os
import re
import numpy as np
import pytest

import htsdf_restatement as HR
import tsdf_cloud_outcome_fixture as CF
import tsdf_cloud_restatement as CR
from support import pose_of, same_bits

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
OPTS = dict(origin=(0.25, 0.15, 1.3), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=6.0)
ODD = dict(OPTS, truncation=0.22)                   # 2 truncation / s = 4.4: the last sample is the fminf clamp
TILTED = pose_of((0.12, -0.2, 0.07), (0.1, -0.05, 0.02))


def cloud(n, seed=3):
    """n points of a wavy wall 1 .. 3 m in front of the sensor, in the sensor frame."""
    r = np.random.default_rng(seed)
    a, b = r.uniform(-0.9, 0.9, n), r.uniform(-0.6, 0.6, n)
    z = 2.0 + 0.8 * np.sin(3 * a) * np.cos(2 * b)
    return np.stack([np.tan(a) * z, np.tan(b) * z, z], 1).astype(f32)


def loop_walk(vol, pts, pose, origin=None):
    """The contract, one ray and one sample at a time, with numpy float32 scalars: (n_rays, n_samples, n_outside, {voxel: [S, N]}, blocks)."""
    P = np.asarray(pose, f32); c = CR.sensor_centre(pose, origin)
    s, tr = vol.s, vol.trunc
    acc, blocks = {}, set()
    n_rays = n_samples = n_outside = 0
    with np.errstate(all="ignore"):
        for p in np.asarray(pts, f32):
            if not np.isfinite(p).all():
                continue
            d = [f32(f32(f32(P[r, 0] * p[0]) + f32(f32(P[r, 1] * p[1]) + f32(P[r, 2] * p[2]))) + P[r, 3]) - c[r] for r in range(3)]
            rr = np.sqrt(f32(f32(d[0] * d[0]) + f32(f32(d[1] * d[1]) + f32(d[2] * d[2]))))
            if not (np.isfinite(rr) and rr > 0 and rr <= vol.max_d):
                continue
            n_rays += 1
            u = [f32(d[a] / rr) for a in range(3)]
            prev = None
            for m in range(CR.n_steps(vol) + 1):
                t = min(f32(f32(rr - tr) + f32(f32(m) * s)), f32(rr + tr))
                if not t > 0:
                    continue
                g = [np.floor(f32(f32(f32(f32(c[a] + f32(t * u[a])) - vol.o[a]) / s) + f32(0.5))) for a in range(3)]
                if not all(CR.VOX_LO <= x <= CR.VOX_HI for x in g):
                    n_outside += 1
                    continue
                gi = tuple(int(x) for x in g)
                if gi == prev:
                    continue
                prev = gi
                n_samples += 1
                blocks.add(tuple(x >> 3 for x in gi))
                e = [f32(f32(vol.o[a] + f32(g[a] * s)) - c[a]) for a in range(3)]
                sdf = f32(rr - f32(f32(e[0] * u[0]) + f32(f32(e[1] * u[1]) + f32(e[2] * u[2]))))
                if sdf < -tr:
                    continue
                k = int(np.rint(f32(min(f32(1), f32(sdf / tr)) * f32(32768.0))))
                a_ = acc.setdefault(gi, [0, 0])
                a_[0] += k; a_[1] += 1
    return n_rays, n_samples, n_outside, acc, blocks


@pytest.mark.parametrize("opts", [OPTS, ODD], ids=["integer", "clamped"])
def test_restatement_against_a_plain_loop(opts):
    """300 points (a NaN, an inf, one at the sensor centre, one beyond max_depth, one nearer than the truncation) from a tilted pose and a
    non-zero sensor origin: counts, the set of blocks, the accumulators of every voxel and the folded volume."""
    pts = cloud(300)
    e = np.array([0.05, -0.02, 0.1], f32)
    pts[3] = (np.nan, 0, 1); pts[5] = (0, np.inf, 1); pts[7] = e; pts[9] = (0, 0, 7.5); pts[11] = (0.05, 0.0, 0.2)
    vol = HR.HVolume(**opts)
    n_rays, n_samples, n_outside, acc, blocks = loop_walk(vol, pts, TILTED, e)
    w = CR.walk(vol, pts, TILTED, e)
    assert (w["n_points"], w["n_rays"], w["n_samples"], w["n_outside"]) == (300, n_rays, n_samples, n_outside) and n_rays == 296 and n_outside == 0
    assert CR.touch(vol, pts, TILTED, e) == blocks and len(blocks) > 10
    uv, S, N = CR.accumulate(w["voxels"], w["k"])
    assert {tuple(v): [int(s), int(n)] for v, s, n in zip(uv.tolist(), S, N)} == acc
    assert N.max() > 1 and n_samples > len(w["voxels"]) > 0          # voxels several rays reach; samples the sdf test dropped
    info = CR.integrate(vol, pts, TILTED, e)
    assert info == dict(n_points=300, n_rays=n_rays, n_updated=len(acc), n_blocks=len(blocks), n_samples=n_samples, n_outside=0)
    assert set(vol.blocks) == blocks
    for g, (s, n) in acc.items():
        b, l = tuple(x >> 3 for x in g), tuple(x & 7 for x in g)
        assert vol.blocks[b][0][l[2], l[1], l[0]] == f32(s / (n * 32768.0)) and vol.blocks[b][1][l[2], l[1], l[0]] == 1
    assert sum(int((wt > 0).sum()) for _, wt in vol.blocks.values()) == len(acc)


def test_a_permutation_of_the_cloud_gives_identical_blocks():
    pts = cloud(500, seed=9)
    a, b, c = HR.HVolume(**OPTS), HR.HVolume(**OPTS), HR.HVolume(**OPTS)
    perm = np.random.default_rng(2).permutation(len(pts))
    for _ in range(2):                                  # the second fold too
        ia, ib, ic = CR.integrate(a, pts, TILTED), CR.integrate(b, pts[perm], TILTED), CR.integrate(c, pts[::-1], TILTED)
        assert ia == ib == ic
    sa = a.sorted_blocks()
    for other in (b, c):
        so = other.sorted_blocks()
        assert np.array_equal(sa[0], so[0]) and same_bits(sa[1], so[1]) and same_bits(sa[2], so[2])
    assert sa[2].max() == 2


def test_a_thousand_copies_of_one_point():
    """N = 1000 in every voxel the ray observes, S = 1000 k, and the fold gives fbar == k / 32768 exactly -- the running average of a
    thousand equal floats would not."""
    p = np.array([[0.31, -0.17, 1.9]], f32)
    vol = HR.HVolume(**OPTS)
    one = CR.walk(vol, p, TILTED)
    w = CR.walk(vol, np.repeat(p, 1000, 0), TILTED)
    uv1, S1, N1 = CR.accumulate(one["voxels"], one["k"])
    uv, S, N = CR.accumulate(w["voxels"], w["k"])
    assert np.array_equal(uv, uv1) and (N1 == 1).all() and (N == 1000).all() and np.array_equal(S, 1000 * S1) and len(uv) >= 5
    assert w["n_rays"] == 1000 and w["n_samples"] == 1000 * one["n_samples"]
    CR.integrate(vol, np.repeat(p, 1000, 0), TILTED)
    for g, k in zip(uv1, S1):
        b, l = tuple(int(x) >> 3 for x in g), tuple(int(x) & 7 for x in g)
        assert vol.blocks[b][0][l[2], l[1], l[0]] == f32(int(k) / 32768.0) and vol.blocks[b][1][l[2], l[1], l[0]] == 1
    assert len(set(S1.tolist())) > 1 and S1.max() <= 32768 and S1.min() >= -32768


def test_a_repeated_voxel_is_dropped():
    """truncation 0.22 at 0.1 m voxels along +x: the samples sit at r - 0.22 + 0.1 m and the last at the clamp r + 0.22, 0.04 m behind the
    one before it -- for this range in the same voxel.  It is skipped and not counted; with the clamp in the next voxel it is counted."""
    opts = dict(ODD, origin=(0.0, 0.0, 0.0))
    vol = HR.HVolume(**opts)
    eye = np.eye(4, dtype=f32)
    same = CR.walk(vol, np.array([[1.0, 0, 0]], f32), eye)          # samples at 0.78 .. 1.18, then 1.22: voxels 8 .. 12, 12
    assert same["n_samples"] == 5 and sorted(same["sampled"][:, 0].tolist()) == [8, 9, 10, 11, 12] and same["n_outside"] == 0
    nxt = CR.walk(vol, np.array([[1.04, 0, 0]], f32), eye)          # 0.82 .. 1.22, then 1.26: voxels 8 .. 12, 13
    assert nxt["n_samples"] == 6 and sorted(nxt["sampled"][:, 0].tolist()) == [8, 9, 10, 11, 12, 13]
    assert loop_walk(vol, np.array([[1.0, 0, 0]], f32), eye)[1] == 5 and loop_walk(vol, np.array([[1.04, 0, 0]], f32), eye)[1] == 6
    # an out-of-range sample between two samples of one voxel does not reset the rule: only in-range samples are remembered
    d = CR.DVolume((10, 4, 4), (0.0, 0.0, 0.0), **{k: v for k, v in ODD.items() if k != "origin"})
    w = CR.walk(d, np.array([[0.9, 0, 0]], f32), eye)               # 0.68 .. 1.08, 1.12: voxels 7, 8, 9, then 10, 11, 11 outside
    assert w["n_samples"] == 3 and w["n_outside"] == 3


def test_dense_and_hashed_restatements_agree():
    """A dense box whose origin is the hashed volume's: equal voxel for voxel inside the box, n_outside the samples that leave it."""
    pts = cloud(400, seed=4)
    opts = dict(OPTS, origin=(-1.0, -1.0, 0.5))
    h = HR.HVolume(**opts); d = CR.DVolume((24, 20, 30), **opts)
    ih, idn = CR.integrate(h, pts, TILTED), CR.integrate(d, pts, TILTED)
    assert ih["n_outside"] == 0 and idn["n_outside"] > 0 and idn["n_samples"] < ih["n_samples"]
    coords, t, w = h.sorted_blocks()
    T, W = HR.blocks_to_dense(coords, t, w, (0, 0, 0), d.dims)
    assert same_bits(T, d.tsdf) and same_bits(W, d.weight) and idn["n_updated"] == int((d.weight > 0).sum()) > 100


def test_outcome_fixture_is_a_surface():
    """The 12 reduced scans fused by the restatement: the held-out scan's noise-free points lie in valid cells for at least half of them,
    and the median distance the field reports there is at most half a voxel (recorded: 97.8 %, 2.3 mm at 0.1 m voxels)."""
    vol, infos = CF.model()
    share, median = CF.assert_surface(vol)
    assert len(infos) == CF.N_SCANS and all(i["n_rays"] == i["n_points"] == CF.N_TILT * CF.N_BEAM and i["n_outside"] == 0 for i in infos)
    assert infos[-1]["n_blocks"] == len(vol.blocks) > 100 and share > 0.9


def test_struct_symbol_python_surface_and_refusals_without_a_device():
    from icp_amd import binding, eth
    assert ctypes.sizeof(binding.IcpTsdfCloudInfo) == 32 and [f[0] for f in binding.IcpTsdfCloudInfo._fields_] == list(CR.INFO)
    assert binding.IcpTsdfCloudInfo.n_samples.offset == 16 and binding.IcpTsdfCloudInfo.n_outside.offset == 24
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    assert "icp_tsdf_integrate_cloud" in binding.EXPORTS and hasattr(lib, "icp_tsdf_integrate_cloud")
    assert re.search(r"^int icp_tsdf_integrate_cloud\(icp_ctx\* ctx, int32_t which, const float pose\[16\], const float sensor_origin\[3\], icp_tsdf_cloud_info\* info_out\);", hdr, flags=re.M)
    assert re.search(r"^\} icp_tsdf_cloud_info;", hdr, flags=re.M)
    p = binding.pose_to_c(np.eye(4)); info = binding.IcpTsdfCloudInfo()
    assert lib.icp_tsdf_integrate_cloud(None, 1, binding._ptr(p), None, ctypes.byref(info)) == 1
    par = inspect.signature(binding.Context.tsdf_integrate_cloud).parameters
    assert list(par) == ["self", "which", "pose", "sensor_origin"] and par["which"].default == "source" and par["sensor_origin"].default is None
    with pytest.raises(ValueError):
        binding.Context.tsdf_integrate_cloud(None, "source", pose=np.eye(3))
    with pytest.raises(ValueError):
        binding.Context.tsdf_integrate_cloud(None, "source", pose=np.eye(4), sensor_origin=(0, 0))
    with pytest.raises(KeyError):
        binding.Context.tsdf_integrate_cloud(None, "neither", pose=np.eye(4))
    par = inspect.signature(eth.fuse_scans).parameters
    assert list(par) == ["ctx", "scans", "poses", "voxel_size", "truncation", "origin", "max_range", "block_capacity", "hashed", "dims"]
    assert (par["voxel_size"].default, par["truncation"].default, par["max_range"].default, par["block_capacity"].default, par["hashed"].default) == (0.05, None, 30.0, 1 << 14, True)
    assert "mesh_path" in inspect.signature(eth.reconstruct).parameters
    for kw in (dict(scans=[cloud(3)], poses=[]), dict(scans=[cloud(3)], poses=[np.eye(4)], hashed=False), dict(scans=[cloud(3)], poses=[np.eye(4)], dims=(8, 8, 8))):
        with pytest.raises(ValueError):
            eth.fuse_scans(None, **kw)
    with pytest.raises(ValueError):
        eth.reconstruct(None, [cloud(3)], np.eye(4), keep_radius=5.0)
