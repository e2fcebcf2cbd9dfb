"""What tests/test_gpu_tsdf_shapes.py rests on, checked without a device: the shapes of tests/tsdf_shape_cases.py sit where they claim
against the tiles as the kernels' own source states them, and every input reaches the code it is meant for -- each integrate step writes
some voxels and (but for the 2 x 2 x 2 volume) not all, each ray-cast size sees a hit and a hole, each mesh has triangles, each target
frame has hits, holes and a padding, and the stale cloud covers the padding.  From the restatement alone, the 256-case volume: cells 0 and
255 give nothing, every other cell gives one triangle per tetrahedron with one corner apart and two per tetrahedron split two and two,
and case m and case 255 - m give the same vertices and the reversed triangles.  These are conditions on the inputs: one that fails needs
another placement, not another shape."""
import ctypes
import os
import re

import numpy as np
import pytest

import tsdf_mesh_restatement as TM
import tsdf_restatement as TS
import tsdf_shape_cases as SC
from support import raw_bits

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def source(name):
    with open(os.path.join(ROOT, "icp-variants_amd", "csrc", name)) as f:
        return f.read()


def test_constants_are_the_neighbours():
    import test_gpu_tsdf
    import test_gpu_tsdf_color
    assert SC.RAY_OPTS == test_gpu_tsdf.RAY_OPTS == test_gpu_tsdf_color.RAY_OPTS
    assert SC.ROOM_OPTS == test_gpu_tsdf.ROOM_OPTS == test_gpu_tsdf_color.ROOM_OPTS
    assert np.array_equal(SC.SOURCE_POSE, test_gpu_tsdf_color.RAY_POSES[1]) and np.array_equal(SC.RAY_POSES["inside"], test_gpu_tsdf_color.RAY_POSES[0])


def test_shapes_against_the_tiles_of_the_source():
    """The tile sizes as dev_tsdf.hpp, dev_tsdf_mesh.hpp and host_tsdf.hpp write them, and where each shape sits against them."""
    dev, mesh, host = source("dev_tsdf.hpp"), source("dev_tsdf_mesh.hpp"), source("host_tsdf.hpp")
    kchunk = int(re.search(r"constexpr int TSDF_KCHUNK = (\d+);", dev).group(1))
    runs = int(re.search(r"constexpr int TM_RUNS = (\d+);", mesh).group(1))
    assert "const dim3 grid((v.nx + 63) / 64, (v.ny + 3) / 4, (v.nz + TSDF_KCHUNK - 1) / TSDF_KCHUNK);" in host and "dim3(64, 4)" in host
    assert "constexpr int TM_BLOCK_VOXELS = 256 * TM_RUNS;" in mesh
    assert "const dim3 grid((cam.width + 15) / 16, (cam.height + 15) / 16);" in host
    assert "const int n = cam.width * cam.height, npad = (n + 63) / 64 * 64;" in host and "if (q < o.npad)" in dev
    tile, block = (64, 4, kchunk), 256 * runs
    grid = lambda d: tuple((d[a] + tile[a] - 1) // tile[a] for a in range(3))
    assert tile == (64, 4, 16) and block == 1024
    assert SC.VOLUMES == [(2, 2, 2), (64, 4, 16), (65, 5, 17), (128, 8, 32), (2, 3, 40), (128, 2, 2), (64, 16, 3), (2, 2, 130), (32, 32, 2)]
    assert grid((64, 4, 16)) == (1, 1, 1) and grid((65, 5, 17)) == (2, 2, 2) and grid((128, 8, 32)) == (2, 2, 2) and SC.BIG == (128, 8, 32)
    assert grid((2, 3, 40)) == (1, 1, 3) and grid((2, 2, 130)) == (1, 1, 9) and 130 % kchunk == 2
    assert all(d[a] <= SC.BIG[a] for d in SC.SLICES for a in range(3)) and set(SC.SLICES) <= set(SC.VOLUMES)
    assert 2 * 2 * 2 < 64 and 32 * 32 == block and 64 * 16 * 3 == 3 * block and 128 * 2 * 2 == block // 2
    assert [d[0] for d in SC.VOLUMES].count(64) == 2 and [d[0] for d in SC.VOLUMES].count(128) == 2 and [d[0] for d in SC.VOLUMES].count(2) == 3
    assert SC.RAY_SIZES == [(1, 1), (8, 8), (16, 16), (17, 17), (32, 16), (64, 1), (1, 30), (33, 15), (40, 30)]
    assert SC.TARGET_FRAMES == [(40, 30), (17, 17), (33, 15)]
    assert [SC.padded(w * h) - w * h for w, h in SC.TARGET_FRAMES] == [16, 31, 17]
    for dims in {d for d, _ in SC.LAYOUTS.values()}:
        assert min(dims) == 2 and sorted(dims)[1] == 47 and sorted(dims)[2] in (47, 64)


def test_smallest_volume_is_accepted():
    from icp_amd import binding
    lib = binding.load_library()
    for dims in SC.VOLUMES:
        assert lib.icp_tsdf_options_check(ctypes.byref(binding.tsdf_options(**SC.integrate_options(dims)))) == 0, dims


@pytest.mark.parametrize("dims", SC.VOLUMES)
def test_integrate_premises(dims):
    """Every step writes more than 0 voxels and, except in (2, 2, 2), fewer than all; it colours some and not all it writes; the marked
    voxels are written by no step; the clamp at max_weight = 2 is reached; TC.integrate_color leaves TS.integrate's tsdf and weight."""
    case = SC.integrate_case(dims)
    ref = SC.integrate_reference(dims)
    n_vox = dims[0] * dims[1] * dims[2]
    plain = SC.started_volume(case)
    for (depth, rgbx, pose), (n, ncol, t, w, rgb, wc) in zip(case["steps"], ref):
        assert 0 < n and (n < n_vox or dims == (2, 2, 2)), (dims, n)
        assert 0 < ncol < n, (dims, n, ncol)
        assert TS.integrate(plain, depth, SC.rcam_of(SC.W, SC.H), pose) == n
        assert np.array_equal(plain.tsdf.view(np.uint32), t.view(np.uint32)) and np.array_equal(plain.weight.view(np.uint32), w.view(np.uint32))
    m = case["marked"]
    assert m.sum() > 0 or dims == (2, 2, 2)
    assert (ref[-1][2].view(np.uint32)[m] == 0x7FC12345).all() and (ref[-1][5].view(np.uint32)[m] == 0xFFC0FACE).all()
    assert (ref[-1][3][~m] <= 2).all() and (ref[-1][3] == 2).sum() > 0 and (ref[-1][5] == 2).sum() > 0
    print("integrate %s: %d voxels, written per step %s, coloured %s, %d marked" % (dims, n_vox, [r[0] for r in ref], [r[1] for r in ref], m.sum()))


@pytest.mark.parametrize("dims", SC.SLICES)
def test_slice_premises(dims):
    """The volume `dims` at BIG's origin is written by every step too, and the restatement itself has the slice identity."""
    ref, big = SC.integrate_reference(dims, SC.BIG), SC.integrate_reference(SC.BIG)
    nx, ny, nz = dims
    for r, b in zip(ref, big):
        assert r[0] > 0
        for x, y in zip(r[2:], b[2:]):
            assert np.array_equal(x.view(np.uint32), np.ascontiguousarray(y[:nz, :ny, :nx]).view(np.uint32))


@pytest.mark.parametrize("size", SC.RAY_SIZES)
def test_raycast_premises(size):
    """Each size other than (1, 1) has a hit and a hole in one of the poses; (1, 1) is what ONE_PIXEL says; inside the 40 x 30 frame the
    restatement itself has the crop identity."""
    w, h = size
    both = False
    for name in SC.RAY_POSES:
        d, v, n, rgba, hits, ncol, path = SC.ray_reference(size, name)
        holes = int((d == SC.MINF).sum())
        assert hits + holes == w * h and d.shape == (h, w)
        both |= hits > 0 and holes > 0
        if size == (1, 1):
            assert ("hit" if hits else "hole") == SC.ONE_PIXEL[name]
        fd, fv, fn, frgba, _, _, _ = SC.ray_reference((SC.W, SC.H), name)
        cw, ch = min(w, SC.W), min(h, SC.H)
        assert np.array_equal(d[:ch, :cw].view(np.uint32), fd[:ch, :cw].view(np.uint32))
        if w <= SC.W and h <= SC.H:
            assert hits == int((fd[:h, :w] != SC.MINF).sum())
            for x, y in zip((d, v, n, rgba), SC.crop(size, fd, fv, fn, frgba)):
                assert np.array_equal(raw_bits(x), raw_bits(y))
        print("ray-cast %s %s: %d hits, %d holes, %d coloured" % (size, name, hits, holes, ncol))
    assert both or size == (1, 1)
    assert set(SC.ONE_PIXEL.values()) == {"hit", "hole"}
    if size == (SC.W, SC.H):                                           # every colour path is taken somewhere
        assert (np.bincount(SC.ray_reference(size, "inside")[6], minlength=4) >= 50).all()


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("size", SC.TARGET_FRAMES)
def test_target_premises(size, color):
    """0 < hits < W H, W H no multiple of 64, a source of more than 100 points, and a stale cloud that reaches beyond the padding with
    copies for every pose in every stretch of 16 entries."""
    w, h = size
    n = w * h
    v, nrm, rgba, hits = SC.target_reference(size, color)
    assert 0 < hits < n and n % 64 != 0 and hits == int((v[:, 2] != SC.MINF).sum())
    sp, sn, sc = SC.target_source(size, color)
    assert len(sp) > 100 and np.isfinite(sp).all() and np.isfinite(sn).all()
    moved = [(sp + np.float32(k), sn, sc) for k in range(2)]
    pts, nr, col = SC.stale_cloud(moved)
    assert len(pts) == SC.STALE_POINTS >= 4096 and len(pts) >= SC.padded(n)
    pad = np.arange(n, SC.padded(n))
    which = np.round(pts[pad, 0] - sp[(pad // 2) % len(sp), 0]).astype(int)
    assert set(which) == {0, 1} and np.array_equal(which, pad % 2)
    K, depth, rgbx, gt = SC.track_frames(size)
    assert depth.shape == (3, h, w) and rgbx.shape == (3, n, 4) and all(np.isfinite(d).sum() > 100 for d in depth)
    print("target %s%s: %d hits of %d, %d padded entries, source %d points" % (size, " coloured" if color else "", hits, n, SC.padded(n) - n, len(sp)))


@pytest.mark.parametrize("dims", SC.VOLUMES)
def test_mesh_premises(dims):
    v, n, t, col = SC.mesh_reference("shape", dims)
    assert len(t) > 0 and len(v) > 0 and int(t.max()) < len(v) and TM.edge_counts(t)[1] == 0
    vol = SC.mesh_volume(dims)
    runs = np.unique(np.floor((v.astype(np.float64) - vol.o) / vol.s + 1e-4).astype(np.int64) @ np.array([1, dims[0], dims[0] * dims[1]]) // 64)
    if dims in SC.PLANE_SHAPES:
        assert len(runs) >= 7, (dims, len(runs))
    assert (col[:, 3] == 255).any()
    print("mesh %s: V %d, T %d, vertices in %d runs, %d without colour" % (dims, len(v), len(t), len(runs), (col[:, 3] == 0).sum()))


def mixed_tetrahedra(m):
    """(tetrahedra of the Kuhn triangulation with corners of both signs, triangles the rule gives them) for corner-sign case m."""
    Q = TM.tet_corners() @ np.array([1, 2, 4])
    mixed = tris = 0
    for p in range(6):
        neg = sum((m >> int(c)) & 1 for c in Q[p])
        if 0 < neg < 4:
            mixed += 1; tris += 2 if neg == 2 else 1
    return mixed, tris


def cyclic(tri):
    k = int(np.argmin(tri))
    return tuple(tri[k:]) + tuple(tri[:k])


@pytest.mark.parametrize("layout", list(SC.LAYOUTS))
def test_case_volume(layout):
    """From the restatement alone.  Cells 0 and 255 give nothing.  Every other cell gives one triangle per tetrahedron that has one corner
    apart and two per tetrahedron split two and two: between 6 and 12 where corners 0 and 7, which all six tetrahedra share, differ in sign,
    and as few as 2 where a corner that only two tetrahedra hold stands alone (the issue's "between 6 and 12" for every cell overlooks
    those; the rule it gives in the same sentence is what is asserted, cell by cell).  Case m and case 255 - m give the same vertices (to
    the rounding of i + t at two different i), opposite normals and the reversed triangles, but for the cells of ZERO_CORNERS, whose zeros
    cannot change sign."""
    vol = SC.case_volume(layout)
    v, n, t, col = SC.mesh_reference("cases", layout)
    dims, (ax_a, ax_b, ax_l) = SC.LAYOUTS[layout]
    # the volume is what it claims: corner c of cell m negative iff bit c of m
    for m in (0, 1, 0x5A, 0x96, 0xFE, 255):
        for c in range(8):
            d = (c & 1, (c >> 1) & 1, c >> 2)
            p = [0, 0, 0]
            p[ax_a] = 3 * (m & 15) + d[ax_a]; p[ax_b] = 3 * (m >> 4) + d[ax_b]; p[ax_l] = d[ax_l]
            assert (vol.tsdf[p[2], p[1], p[0]] < 0) == bool((m >> c) & 1) and vol.weight[p[2], p[1], p[0]] == 1
    assert TM.valid_cells(vol).sum() == 256
    zeros = vol.tsdf[vol.weight > 0] == 0
    assert zeros.sum() == sum(len(c) for c in SC.ZERO_CORNERS.values()) and np.signbit(vol.tsdf[vol.weight > 0][zeros]).any() and not np.signbit(vol.tsdf[vol.weight > 0][zeros]).all()
    cell = SC.cell_of_vertices(layout, v)
    tc = cell[t.astype(np.int64)]
    assert (tc == tc[:, :1]).all()                                      # no triangle joins two cells
    per = np.bincount(tc[:, 0], minlength=256)
    assert per[0] == 0 and per[255] == 0 and not (cell == 0).any() and not (cell == 255).any()
    for m in range(1, 255):
        mixed, tris = mixed_tetrahedra(m)
        assert mixed >= 2 and per[m] == tris and mixed <= per[m] <= 2 * mixed, (m, mixed, tris, per[m])
        if ((m >> 0) & 1) != ((m >> 7) & 1):
            assert mixed == 6 and 6 <= per[m] <= 12, m
    assert per[1:255].min() == 2 and per[1:255].max() == 12 and TM.edge_counts(t)[1] == 0
    # complements: vertices relative to the cell's lowest corner, triangles as cyclic triples of them
    base = np.zeros((256, 3)); base[:, ax_a] = 3 * (np.arange(256) & 15); base[:, ax_b] = 3 * (np.arange(256) >> 4)
    rel = v.astype(np.float64) - base[cell]
    skip = set(SC.ZERO_CORNERS) | {255 - m for m in SC.ZERO_CORNERS}
    checked = 0
    for m in range(1, 128):
        if m in skip:
            continue
        a, b = np.nonzero(cell == m)[0], np.nonzero(cell == 255 - m)[0]
        # the same vertices, in the same order: t has the same bits in both cells, and i + t is rounded once at each cell's own
        # coordinates, which lie below 64 -- half an ulp there, 2^-19, on either side
        assert len(a) == len(b) and np.abs(rel[a] - rel[b]).max() <= 2.0 ** -18, m
        assert np.array_equal(rel[a] == np.floor(rel[a]), rel[b] == np.floor(rel[b])), m  # (the same edges carry them)
        ta = sorted(cyclic(np.searchsorted(a, x)) for x in t[tc[:, 0] == m].astype(np.int64))             # (a vertex by its rank in its cell)
        tb = sorted(cyclic(np.searchsorted(b, x[::-1])) for x in t[tc[:, 0] == 255 - m].astype(np.int64))
        assert ta == tb, m
        assert np.array_equal(n[a].view(np.uint32) ^ np.uint32(0x80000000), n[b].view(np.uint32)) or (n[a] == 0).any(), m
        checked += 1
    assert checked >= 120
    print("cases %s: V %d, T %d, triangles per cell %d .. %d, %d complement pairs" % (layout, len(v), len(t), per[1:255].min(), per[1:255].max(), checked))


def test_layouts_hold_the_same_cells():
    """The three layouts differ in where the cells lie, not in what they are: cell m has the same triangle count in each."""
    per = []
    for layout in SC.LAYOUTS:
        v, _, t, _ = SC.mesh_reference("cases", layout)
        per.append(np.bincount(SC.cell_of_vertices(layout, v)[t[:, 0].astype(np.int64)], minlength=256))
    assert np.array_equal(per[0], per[1]) and np.array_equal(per[0], per[2])
