"""The cases of tests/tsdf_cloud_cases.py on the restatement alone, no device: every case reaches the edge it is named for, so a case that
drifts off its edge fails here and not silently on the device (tests/test_gpu_tsdf_cloud_shapes.py).  The conditions are caps on what a
case may leave out, not measurements."""
import itertools
import os
import numpy as np
import pytest

import htsdf_restatement as HR
import tsdf_cloud_cases as TC
import tsdf_cloud_restatement as CR

f32 = np.float32


def weights(vol):
    if isinstance(vol, CR.DVolume):
        return vol.weight
    return np.stack([w for _, w in vol.blocks.values()]) if vol.blocks else np.zeros((0, 8, 8, 8), f32)


def walk_of(step):
    opts, dims, pts, pose, origin, _ = step
    return CR.walk(TC.new_volume(opts, dims), pts, pose, origin)


def blocks_of(opts, pts, pose=TC.EYE, origin=None):
    return CR.touch(HR.HVolume(**opts), np.asarray(pts, f32).reshape(-1, 3), pose, origin)


def test_every_case_has_a_reason_and_one_volume():
    assert len(TC.ALL) == sum(len(t) for t in TC.TABLES.values()) == 49
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "icp_hip.h")).read()
    assert "nx, ny, nz >= 2" in header and all(min(d) == 1 for d in TC.REFUSED) and all(min(d) >= 2 for d in TC.SHAPES)
    assert [tuple(max(n, 2) for n in d) for d in TC.REFUSED] == TC.SHAPES[:4]          # each refused box beside the thinnest legal one
    for table, name in TC.ALL:
        reason, steps = TC.TABLES[table][name]
        assert isinstance(reason, str) and reason and "\n" not in reason and len(steps) >= 1
        for opts, dims, pts, pose, origin, capacity in steps:
            assert opts == steps[0][0] and dims == steps[0][1] and capacity == steps[0][5]
            assert pts.dtype == f32 and pts.ndim == 2 and pts.shape[1] == 3 and pose.dtype == f32 and pose.shape == (4, 4)
            assert dims is not None or capacity > 0                    # (a dense case's capacity is not used)


@pytest.mark.parametrize("dims", TC.SHAPES, ids=TC.shape_name)
def test_dense_shapes(dims):
    """Both poses write into the box and leave it; the second fold meets W = 1; the updated voxels spread along every axis longer than 1;
    and wherever an exchange of two strides, or of two extents in ((iz ny) + iy) nx + ix, moves any voxel of the box, it moves an
    updated one."""
    case = TC.DENSE_SHAPES[TC.shape_name(dims)]
    assert [s[1] for s in case[1]] == [dims, dims] and (case[1][0][4] is not None) == (TC.shape_name(dims) == TC.AS_TARGET)
    infos, vol = TC.reference("DENSE_SHAPES", TC.shape_name(dims))
    for i in infos:
        assert i["n_updated"] > 0 and i["n_outside"] > 0 and i["n_rays"] == 3000, i
    assert vol.weight.max() == 2 and vol.weight.shape == dims[::-1]
    index = lambda v, n: (v[:, 2] * n[1] + v[:, 1]) * n[0] + v[:, 0]
    box = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    visible = 0
    for k, step in enumerate(case[1]):
        v = np.unique(walk_of(step)["voxels"], axis=0)                         # the voxels this pose updates
        assert len(v) == infos[k]["n_updated"]
        for a in range(3):
            assert dims[a] == 1 or len(np.unique(v[:, a])) > 1, (dims, k, a)
        for a, b in itertools.combinations(range(3), 2):
            swap = list(range(3)); swap[a], swap[b] = b, a
            n2 = tuple(dims[j] for j in swap)
            for what, moved in (("strides", lambda w: index(w[:, swap], dims) != index(w, dims)), ("extents", lambda w: index(w, n2) != index(w, dims))):
                assert not moved(box).any() or moved(v).any(), (dims, k, what, a, b)
                visible += bool(moved(box).any())
    assert len(set(dims)) == 1 or visible >= 2 * 3                              # a non-cubic box: exchanges do show


def test_dense_faces():
    """For every face, a call whose counted samples all lie in the face layer and a twin 2^-10 voxel further out with every sample outside,
    with the counts worked out by hand in the cases module; the edge, the band's end and the corner."""
    assert len(TC.FACE_PAIRS) == 6 and {(a, l) for a, l, _, _ in TC.FACE_PAIRS} == {(a, l) for a, n in enumerate(TC.FACE_DIMS) for l in (0, n - 1)}
    for axis, layer, inside, outside in TC.FACE_PAIRS:
        si, so = TC.DENSE_FACES[inside][1][0], TC.DENSE_FACES[outside][1][0]
        assert np.array_equal(np.delete(si[2], axis, 1), np.delete(so[2], axis, 1)) and abs(si[4][axis] - so[4][axis]) == 0.25 * TC.EPS
        w = walk_of(si)
        n = TC.FACE_COUNTS[axis]
        assert w["n_rays"] == 4 and w["n_samples"] == n and w["n_outside"] == 28 - n and (w["sampled"][:, axis] == layer).all(), inside
        assert len(w["voxels"]) == n and sorted(w["k"].tolist())[-4:] == [32768] * 4, inside
        infos, vol = TC.reference("DENSE_FACES", inside)
        assert infos[0]["n_updated"] == n and int((vol.weight > 0).sum()) == n
        sel = [slice(None)] * 3; sel[2 - axis] = layer
        assert int((vol.weight[tuple(sel)] > 0).sum()) == n
        w = walk_of(so)
        assert w["n_rays"] == 4 and w["n_samples"] == 0 and w["n_outside"] == 28, outside
    w = walk_of(TC.DENSE_FACES["edge"][1][0])
    assert w["n_samples"] == 4 and w["n_outside"] == 3 and w["sampled"].tolist() == [[x, 0, 0] for x in (2, 3, 4, 5)]
    w = walk_of(TC.DENSE_FACES["band_end"][1][0])
    assert w["n_samples"] == 6 and w["n_outside"] == 1 and w["voxels"].tolist() == [[x, 2, 1] for x in range(6)] and w["k"][-1] == -32768
    _, vol = TC.reference("DENSE_FACES", "band_end")
    assert vol.tsdf[1, 2, 5] == -1 and vol.weight[1, 2, 5] == 1
    w = walk_of(TC.DENSE_FACES["corner"][1][0])
    assert w["n_samples"] > 0 and w["n_outside"] > 0 and w["sampled"].max(0).tolist() == [5, 4, 3]
    valid, g = TC.sample_voxels(*[TC.DENSE_FACES["corner"][1][0][j] for j in (0, 2, 3, 4)])
    assert valid.all() and (g[-1, 0] > np.array(TC.FACE_DIMS) - 1).all()          # the last sample is beyond the box on all three axes


@pytest.mark.parametrize("name", list(TC.RANGE_STRADDLE))
def test_range_straddle(name):
    """Samples on both sides of the last storable voxel in one call, and that voxel itself among them."""
    step = TC.RANGE_STRADDLE[name][1][0]
    w = walk_of(step)
    assert w["n_samples"] > 0 and w["n_outside"] > 0 and w["n_rays"] == 21, w
    axis, last = "xyz".index(name[0]), ((1 << 23) - 1 if name.endswith("plus") else -(1 << 23))
    assert (w["sampled"][:, axis] == last).any()
    blocks = blocks_of(step[0], step[2], step[3])
    assert {b[axis] for b in blocks} == {last >> 3} and len(blocks) >= 2
    infos, vol = TC.reference("RANGE_STRADDLE", name)
    assert vol.n_out_of_range == infos[0]["n_outside"] and infos[0]["n_updated"] > 0


@pytest.mark.parametrize("name", list(TC.PILE_UP))
def test_pile_up(name):
    """N of 2^17 + 1 (16384 in the mix), S beyond 32 bits and S below zero on the same call."""
    w = walk_of(TC.PILE_UP[name][1][0])
    uv, S, N = CR.accumulate(w["voxels"], w["k"])
    if name.startswith("one_point"):
        assert len(uv) == 6 and (N == TC.PILE_N).all() and TC.PILE_N == 131073 and w["n_samples"] == 917511
        assert S.max() == 4295000064 > 1 << 32 and S.min() < -(1 << 31)            # (2^17 + 1) 2^15; the low word alone would be wrong
    else:
        assert N.max() == 2 * 16384 and S.max() >= 16384 * 32768 and S.min() < -(1 << 28) and len(uv) > 1000 and N.min() == 1
        assert len(np.unique(TC.PILE_UP[name][1][0][2][:64], axis=0)) > 4         # shuffled: the first wave holds piles and wall alike


@pytest.mark.parametrize("name", list(TC.SATURATION))
def test_saturation(name):
    mw = TC.SATURATION[name][1][0][0]["max_weight"]
    top, low = [], []
    TC.replay(TC.SATURATION[name], lambda k, v, i: (top.append(float(weights(v).max())), low.append(float(weights(v)[weights(v) > 0].min()))))
    assert top == TC.SAT_WEIGHTS[mw] and low[-1] == 1.0          # beside the saturated voxels some seen once


def test_lanes():
    """What every order of points claims, on the block keys of the rays' samples."""
    key = lambda pts: blocks_of(TC.OPTS, pts)
    a, b = key([TC.A]), key([TC.B])
    assert a and b and not a & b
    valid, g = TC.sample_voxels(TC.OPTS, TC.LANE_CLOUDS["abab"][1], TC.EYE)
    first = (g[0] // 8).astype(np.int64)
    assert valid.all() and len(first) == 192 and (first[0::2] == first[0]).all() and (first[1::2] == first[1]).all() and (first[0] != first[1]).any()
    same = TC.LANE_CLOUDS["same_256"][1]
    assert len(same) == 256 and (same == same[0]).all() and key(same) == a
    nb = TC.LANE_CLOUDS["nan_between"][1]
    assert np.isnan(nb[2]).all() and (nb[[0, 1, 3, 4]] == f32(TC.A)).all() and key(nb) == a
    runs = TC.LANE_CLOUDS["runs"][1]
    rest = np.ones(len(runs), bool)
    for lo, hi, p in ((60, 70, TC.RUN_A), (250, 262, TC.RUN_B)):
        assert (runs[lo:hi + 1] == f32(p)).all() and not (runs[lo - 1] == f32(p)).all() and not (runs[hi + 1] == f32(p)).all()
        assert lo // 64 != hi // 64                              # the run crosses lane 0 of a wave
        rest[lo:hi + 1] = False
    assert 250 // 256 != 262 // 256
    others = key(runs[rest])
    assert key([TC.RUN_A]) and not key([TC.RUN_A]) & others and key([TC.RUN_B]) and not key([TC.RUN_B]) & others and not key([TC.RUN_A]) & key([TC.RUN_B])
    lone = TC.LANE_CLOUDS["last_wave_of_one"][1]
    assert len(lone) % 64 == 1 and key(lone[-1:]) and not key(lone[-1:]) & key(lone[:-1])
    for name, (_, steps) in TC.LANES.items():
        assert steps[0][1] is None and steps[0][5] == int(name.rsplit("_", 1)[1])
        assert len(TC.reference("LANES", name)[1].blocks) > (1 if steps[0][5] == 1 else 0)       # capacity 1: the pool has to grow


@pytest.mark.parametrize("name", list(TC.BAND))
def test_band(name):
    step = TC.BAND[name][1][0]
    vol = TC.new_volume(step[0], step[1])
    M = TC.BAND_STEPS[step[0]["truncation"]]
    assert CR.n_steps(vol) == M
    w = walk_of(step)
    assert w["n_rays"] == 300 and w["n_samples"] > 0
    valid, g = TC.sample_voxels(step[0], step[2], step[3], step[4])
    blocks = (g // 8).astype(np.int64)
    per_ray = [len({tuple(b) for b in blocks[:, i]}) for i in range(blocks.shape[1])]
    if M == 1:
        assert w["n_samples"] + w["n_outside"] < 2 * w["n_rays"] and valid.all()          # some ray's two samples share a voxel
    else:
        assert M == 20 and max(per_ray) >= 3                                              # one ray crosses three blocks
