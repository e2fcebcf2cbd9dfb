"""icp_mesh_cluster and icp_tsdf_mesh_clustered on the device: against the numpy restatement of the contract
(tests/mesh_cluster_restatement.py) bit for bit on crafted and random meshes (tests/mesh_cluster_cases.py); the calling contract; the
clustered mesh of a dense and of a hashed volume against icp_mesh_cluster of the unclustered call; the pipelines that write a mesh."""
import ctypes as C
import functools
import os
import numpy as np
import pytest

import htsdf_mesh_cases as HMC
import mesh_cluster_cases as K
import mesh_cluster_restatement as R
import tsdf_mesh_restatement as TM
from support import bits, same_bits, upload

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG = 1
CRAFTED = list(K.crafted())


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


def assert_same(got, want, what):
    """(vertices, normals | None, colors | None, triangles, info): every array bit for bit, every count equal."""
    assert got[4] == want[4], (what, got[4], want[4])
    assert got[3].dtype == np.uint32 and got[3].shape == want[3].shape and np.array_equal(got[3], want[3]), what
    assert got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])), what
    assert (got[1] is None) == (want[1] is None) and (got[2] is None) == (want[2] is None), what
    if want[1] is not None:
        assert np.array_equal(bits(got[1]), bits(want[1])), what
    if want[2] is not None:
        assert got[2].dtype == np.uint8 and np.array_equal(got[2], want[2]), what


@functools.lru_cache(maxsize=None)
def reference(kind, key, normals=True, colors=True):
    case = K.crafted()[key] if kind == "crafted" else getattr(K, kind)(*key)
    a, kw = K.args(case, normals, colors)
    return case, R.cluster(*a, **kw)


def run(ctx, kind, key=(), normals=True, colors=True):
    case, want = reference(kind, key, normals, colors)
    a, kw = K.args(case, normals, colors)
    got = ctx.mesh_cluster(*a, **kw)
    i = got[4]
    print("%s %s: V %d -> %d, T %d -> %d, cells %d, invalid %d / %d, degenerate %d, duplicate %d"
          % (kind, key, i["n_vertices_in"], i["n_vertices"], i["n_triangles_in"], i["n_triangles"], i["n_cells"], i["n_invalid_vertices"], i["n_invalid_triangles"],
             i["n_degenerate"], i["n_duplicate"]))
    assert_same(got, want, (kind, key))
    assert i["n_triangles"] + i["n_degenerate"] + i["n_duplicate"] + i["n_invalid_triangles"] == i["n_triangles_in"]
    assert ctx.mesh_cluster_info() == i
    return case, got


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_meshes_bit_for_bit(ctx, name):
    case, (v, n, c, t, info) = run(ctx, "crafted", name)
    counts = (info["n_vertices"], info["n_triangles"], info["n_degenerate"], info["n_duplicate"], info["n_invalid_vertices"], info["n_invalid_triangles"])
    if name == "empty":
        assert counts == (0, 0, 0, 0, 0, 0) and info["n_cells"] == 0
    elif name == "vertices without triangles":
        assert counts == (0, 0, 0, 0, 0, 0) and info["n_cells"] == 3
    elif name == "triangles without vertices":
        assert counts == (0, 0, 0, 0, 0, 2)
    elif name == "one triangle over three cells":                     # comes back unchanged
        assert counts == (3, 1, 0, 0, 0, 0) and same_bits(v, case["vertices"]) and np.array_equal(t, case["triangles"])
    elif name == "one triangle inside one cell":
        assert counts == (0, 1 - 1, 1, 0, 0, 0) and info["n_cells"] == 1
    elif name == "same triple in two rotations":                      # the lowest index survives, with its own corner order
        assert counts == (3, 1, 0, 2, 0, 0) and t.tolist() == [[1, 2, 0]]
    elif name == "opposite orientations":                             # both orientations stay; the third triangle repeats the second
        assert counts == (3, 2, 0, 1, 0, 0) and t.tolist() == [[0, 1, 2], [0, 2, 1]]
    elif name == "a cluster whose triangles all degenerate":          # the first cell is absent and the later ranks shift down
        assert counts == (3, 1, 2, 1, 0, 0) and info["n_cells"] == 4 and t.tolist() == [[0, 1, 2]] and (v < 2).all()
    elif name == "negative coordinates":
        assert counts[4:] == (0, 0) and info["n_triangles"] > 0
    elif name == "cells at -2^20 and 2^20 - 1":
        assert counts[4:] == (0, 0) and info["n_triangles"] == 4 and np.abs(v).max() >= float(1 << 20) - 1
    elif name == "outside the range, NaN and inf":
        assert counts[4:] == (5, 5) and info["n_triangles"] == 2 and info["n_duplicate"] == 1
    elif name == "indices beyond the vertices":                       # counted, and nothing read out of bounds
        assert counts == (3, 1, 0, 1, 0, 4)
    elif name == "normals that cancel, a NaN normal, uncoloured members":
        assert n[0].tolist() == [0, 0, 0] and n[1].tolist() == [1, 0, 0] and c[2].tolist() == [0, 0, 0, 0] and c[0].tolist() == [11, 21, 31, 255]


def test_4096_vertices_in_one_cell(ctx):
    case, (v, n, c, t, info) = run(ctx, "one_cell")
    assert (info["n_vertices"], info["n_triangles"], info["n_degenerate"], info["n_duplicate"]) == (3, 2, 1, 4) and info["n_cells"] == 3


def test_distinct_cells_fill_half_the_table(ctx):
    case, (v, n, c, t, info) = run(ctx, "distinct_cells", (5000,))
    assert info["n_cells"] == 5000 and info["n_duplicate"] > 1000 and info["n_vertices"] > 4900


@pytest.mark.parametrize("V", K.RANDOM_SIZES)
def test_random_meshes_bit_for_bit(ctx, V):
    case, (v, n, c, t, info) = run(ctx, "random_mesh", (V,))
    assert info["n_invalid_vertices"] > 0 and info["n_invalid_triangles"] > 0 and info["n_duplicate"] > 0 and info["n_triangles"] > 0


@pytest.mark.parametrize("normals,colors", [(True, False), (False, True), (False, False)])
def test_attributes_given_and_not_given(ctx, normals, colors):
    case, got = run(ctx, "random_mesh", (1025,), normals, colors)
    full = reference("random_mesh", (1025,))[1]
    assert (got[1] is None) == (not normals) and (got[2] is None) == (not colors)
    assert same_bits(got[0], full[0]) and np.array_equal(got[3], full[3])      # geometry does not depend on the attributes


def _raw(ctx, case, max_v, max_t, fill=True, normals=True, colors=True):
    """One icp_mesh_cluster through ctypes with the given capacities; the arrays are pre-filled with a sentinel."""
    from icp_amd import binding
    v, t, nr, col = case["vertices"], case["triangles"], case["normals"], case["colors"]
    ov = np.full((max(max_v, 1), 3), 7.0, f32); on = np.full((max(max_v, 1), 3), 7.0, f32); oc = np.full((max(max_v, 1), 4), 7, np.uint8)
    ot = np.full((max(max_t, 1), 3), 7, np.uint32)
    info = binding.IcpMeshClusterInfo()
    P = binding._ptr
    opt = binding.mesh_cluster_options(case["cell_size"], case["origin"])
    rc = ctx.lib.icp_mesh_cluster(ctx.h, len(v), len(t), P(v), P(nr) if normals else None, P(col) if colors else None, P(t), C.byref(opt), max_v, max_t,
                                  P(ov) if fill else None, P(on) if fill and normals else None, P(oc) if fill and colors else None, P(ot) if fill else None, C.byref(info))
    return rc, (ov, on, oc, ot), binding._record(info), ctx.lib.icp_last_error(ctx.h).decode()


def test_capacity_one_short_is_refused_and_writes_nothing(ctx):
    case, want = reference("random_mesh", (257,))
    nv, nt = want[4]["n_vertices"], want[4]["n_triangles"]
    for mv, mt in ((nv - 1, nt), (nv, nt - 1)):
        rc, arrays, info, msg = _raw(ctx, case, mv, mt)
        assert rc == ERR_INVALID_ARG and info == want[4]
        assert all(str(x) in msg for x in (nv, nt, mv, mt)) and "icp_mesh_cluster" in msg
        assert all((a == 7).all() for a in arrays)
    rc, arrays, info, msg = _raw(ctx, case, nv, nt)
    assert rc == 0 and same_bits(arrays[0][:nv], want[0]) and np.array_equal(arrays[3][:nt], want[3])
    assert same_bits(arrays[1][:nv], want[1]) and np.array_equal(arrays[2][:nv], want[2])


def test_counting_call_and_refusals(ctx):
    from icp_amd import binding
    case, want = reference("random_mesh", (257,))
    rc, _, info, _ = _raw(ctx, case, 0, 0, fill=False)
    assert rc == 0 and info == want[4]                               # a counting call equals the filling call's counts
    P = binding._ptr
    v, t = case["vertices"], case["triangles"]
    out_v, out_t, out_n, out_c = np.zeros((len(v), 3), f32), np.zeros((len(t), 3), np.uint32), np.zeros((len(v), 3), f32), np.zeros((len(v), 4), np.uint8)
    info = binding.IcpMeshClusterInfo()

    def call(opt, vo=out_v, to=out_t, no=None, co=None, nrm=None, col=None, nv=len(v), nt=len(t), inf=info):
        rc = ctx.lib.icp_mesh_cluster(ctx.h, nv, nt, P(v), nrm, col, P(t), C.byref(opt) if opt is not None else None, len(v), len(t), P(vo), P(no), P(co), P(to),
                                      C.byref(inf) if inf is not None else None)
        return rc, ctx.lib.icp_last_error(ctx.h).decode()
    good = binding.mesh_cluster_options(0.5)
    for bad in (binding.mesh_cluster_options(0.0), binding.mesh_cluster_options(-1.0), binding.mesh_cluster_options(np.inf), binding.mesh_cluster_options(np.nan),
                binding.mesh_cluster_options(0.5, (np.nan, 0, 0)), binding.mesh_cluster_options(0.5, (0, np.inf, 0)), None):
        rc, msg = call(bad)
        assert rc == ERR_INVALID_ARG and "icp_mesh_cluster" in msg
    assert call(good, to=None)[0] == ERR_INVALID_ARG and call(good, vo=None)[0] == ERR_INVALID_ARG          # vertices_out and triangles_out go together
    assert call(good, no=out_n)[0] == ERR_INVALID_ARG and call(good, co=out_c)[0] == ERR_INVALID_ARG        # normals_out needs normals, colors_out colors
    assert call(good, nv=-1)[0] == ERR_INVALID_ARG and call(good, nt=(1 << 27) + 1)[0] == ERR_INVALID_ARG
    assert call(good, inf=None)[0] == ERR_INVALID_ARG
    assert call(good)[0] == 0 and info.n_vertices == R.cluster(v, t, 0.5)[4]["n_vertices"]


def test_two_calls_give_identical_arrays(ctx):
    for kind, key in (("random_mesh", (1025,)), ("one_cell", ()), ("distinct_cells", (5000,))):
        case = reference(kind, key)[0]
        a, kw = K.args(case)
        x, y = ctx.mesh_cluster(*a, **kw), ctx.mesh_cluster(*a, **kw)
        assert_same(x, y, kind)


# ---- the composite: the clustered mesh of a volume == icp_mesh_cluster of the unclustered mesh

CENTRE = np.array([0.013, -0.021, 0.034])


def dense_sphere(factory, color):
    vol = TM.analytic_volume(TM.sphere(CENTRE, 0.6))
    if color:
        rng = np.random.default_rng(5)
        vol.rgb = rng.uniform(0, 255, vol.tsdf.shape + (3,)).astype(f32)
        vol.wc = (rng.random(vol.tsdf.shape) > 0.2).astype(f32)
    c = factory()
    upload(c, vol, color=color)
    return c, (-0.95, -0.95, -0.95), 0.1


def hashed_sphere(factory, color):
    coords, t, w = HMC.case_b()                                       # 2 x 2 x 2 blocks around the origin: blocks at negative coordinates
    c = factory()
    c.tsdf_create_hashed(color=color, **HMC.OPTS)
    if color:
        rng = np.random.default_rng(6)
        c.tsdf_upload_blocks(coords, t, w, rng.uniform(0, 255, t.shape + (3,)).astype(f32), (rng.random(t.shape) > 0.2).astype(f32))
    else:
        c.tsdf_upload_blocks(coords, t, w)
    return c, HMC.OPTS["origin"], HMC.OPTS["voxel_size"]


@pytest.mark.parametrize("storage", ["dense", "hashed"])
@pytest.mark.parametrize("color", [False, True])
def test_clustered_volume_mesh_equals_cluster_of_the_mesh(gpu_ctx_factory, storage, color):
    c, origin, voxel = (dense_sphere if storage == "dense" else hashed_sphere)(gpu_ctx_factory, color)
    mesh = c.tsdf_mesh if storage == "dense" else c.tsdf_mesh_hashed
    plain = mesh(colors=color)
    again = mesh(colors=color, cluster=None)                          # cluster=None is the call without the keyword
    assert all(np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b) for a, b in zip(plain, again))
    assert len(plain[2]) > 1000
    other = gpu_ctx_factory()
    for cells, cluster_origin in ((2, None), (3, None), (2, (0.01, 0.02, -0.03))):
        got = mesh(colors=color, cluster=cells * voxel, cluster_origin=cluster_origin)
        info = c.mesh_cluster_info()
        want = other.mesh_cluster(plain[0], plain[2], cells * voxel, normals=plain[1], colors=plain[3] if color else None,
                                  origin=origin if cluster_origin is None else cluster_origin)
        rest = R.cluster(plain[0], plain[2], cells * voxel, normals=plain[1], colors=plain[3] if color else None, origin=origin if cluster_origin is None else cluster_origin)
        print("%s%s, cells of %d voxels: V %d -> %d, T %d -> %d" % (storage, " with colours" if color else "", cells, len(plain[0]), len(got[0]), len(plain[2]), len(got[2])))
        assert_same((got[0], got[1], got[3] if color else None, got[2], info), want, (storage, color, cells))
        assert_same(want, rest, (storage, color, cells, "restatement"))
        assert 0 < len(got[2]) < len(plain[2]) and len(got) == len(plain)
    if storage == "hashed":
        v, n, t = mesh(normals=False, cluster=2 * voxel)[:3]
        assert n is None and same_bits(v, mesh(cluster=2 * voxel)[0])
    still = mesh(colors=color)                                        # the volume and the plain call are what they were
    assert all(np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b) for a, b in zip(plain, still))


def test_clustered_volume_mesh_refusals(gpu_ctx_factory):
    from icp_amd import binding
    c = gpu_ctx_factory()
    with pytest.raises(binding.IcpError, match="no volume"):
        c.tsdf_mesh(cluster=0.2)
    for make in (dense_sphere, hashed_sphere):
        c, origin, voxel = make(gpu_ctx_factory, False)
        mesh = c.tsdf_mesh if make is dense_sphere else c.tsdf_mesh_hashed
        with pytest.raises(binding.IcpError, match="colour"):
            mesh(colors=True, cluster=2 * voxel)                      # with_colors on a volume without colours
        with pytest.raises(binding.IcpError, match="cell_size"):
            mesh(cluster=0.0)
        with pytest.raises(binding.IcpError, match="min_weight"):
            c._tsdf_mesh_clustered(-1.0, True, False, 2 * voxel, None)
        # capacities one short: refused with the four numbers, nothing written
        v, n, t = mesh(cluster=2 * voxel)
        opt = binding.mesh_cluster_options(2 * voxel, origin)
        nv, nt, info = C.c_int32(0), C.c_int32(0), binding.IcpMeshClusterInfo()
        ov, ot = np.full((len(v), 3), 7.0, f32), np.full((len(t), 3), 7, np.uint32)
        rc = c.lib.icp_tsdf_mesh_clustered(c.h, 0.0, C.byref(opt), 0, len(v) - 1, len(t), binding._ptr(ov), None, None, binding._ptr(ot), C.byref(nv), C.byref(nt), C.byref(info))
        msg = c.lib.icp_last_error(c.h).decode()
        assert rc == ERR_INVALID_ARG and (nv.value, nt.value) == (len(v), len(t)) and all(str(x) in msg for x in (len(v), len(t), len(v) - 1))
        assert (ov == 7).all() and (ot == 7).all() and info.n_vertices == len(v)


# ---- the pipelines that end in one mesh

def test_reconstruct_room_writes_a_clustered_mesh(tmp_path, gpu_ctx_factory):
    pytest.importorskip("PIL")
    from icp_amd import meshio, tum
    from icp_amd.synth import tum_K
    W, H = 80, 60
    Kc = tum_K(W)
    d = str(tmp_path / "seq")
    tum.write_synthetic_sequence(d, 2, width=W, height=H, K=Kc)
    seq = tum.load_sequence(d, frame_step=1, K=Kc)
    out = str(tmp_path / "out")
    model = dict(hashed=True, origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)
    ctx = gpu_ctx_factory()
    tum.reconstruct_room(ctx, seq, out_dir=out, model=model, sdf=dict(stride=1, n_iterations=10), model_mesh="m.ply", densify=False, mesh_cluster=0.2)
    info = ctx.mesh_cluster_info()
    v, n, t = meshio.load_ply_mesh(os.path.join(out, "m.ply"))
    full = ctx.tsdf_mesh_hashed()
    assert len(v) == info["n_vertices"] and len(t) == info["n_triangles"] and 0 < len(t) < len(full[2]) and info["n_triangles_in"] == len(full[2])
    with pytest.raises(ValueError):
        tum.reconstruct_room(ctx, seq, model=model, mesh_cluster=0.2)                  # no mesh to write
    dense = dict(dims=(64, 40, 48), origin=(-3.15, -1.95, 0.05), voxel_size=0.1, truncation=0.4)
    tum.reconstruct_room(ctx, seq, out_dir=out, model=dense, model_mesh="d.ply", mesh_cluster=0.2)
    info = ctx.mesh_cluster_info()
    v, n, t = meshio.load_ply_mesh(os.path.join(out, "d.ply"))
    assert len(v) == info["n_vertices"] > 0 and len(t) == info["n_triangles"] > 0


def test_eth_reconstruct_writes_a_clustered_mesh(tmp_path, gpu_ctx_factory):
    import tsdf_cloud_outcome_fixture as CF
    from icp_amd import eth, meshio
    clouds, poses, normals = CF.scans()
    scans = list(zip(clouds, normals))[:3]
    ctx = gpu_ctx_factory()
    ctx.set_gicp_options(1e-3, 0)
    path = str(tmp_path / "room.ply")
    args = dict(tsdf_voxel_size=CF.VOXEL, truncation=CF.TRUNCATION, voxel_size=0.25, hashed=True, n_iterations=30, min_valid=64)
    _, _, _, mesh = eth.reconstruct(ctx, scans, poses[0], mesh_path=path, mesh_cluster=2 * CF.VOXEL, **args)
    info = ctx.mesh_cluster_info()
    back = meshio.load_ply_mesh(path)
    assert len(back[0]) == info["n_vertices"] > 0 and len(back[2]) == info["n_triangles"] > 0 and info["n_triangles"] < info["n_triangles_in"]
    assert all(same_bits(a, b) if a.dtype == f32 else np.array_equal(a, b) for a, b in zip(mesh, back))
    with pytest.raises(ValueError):
        eth.reconstruct(ctx, scans, poses[0], mesh_cluster=2 * CF.VOXEL, **args)      # no mesh to write
