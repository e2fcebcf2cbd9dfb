"""Vertex clustering on the host side: properties of the numpy restatement of the contract (tests/mesh_cluster_restatement.py) -- the
consistency identity of the counts, every output vertex near its members, independence of the input order, and what clustering does to the
analytic sphere and torus of tests/test_tsdf_mesh_host.py.  No device code runs here."""
import numpy as np
import pytest

import mesh_cluster_cases as K
import mesh_cluster_restatement as R
import tsdf_mesh_restatement as TM

f32 = np.float32
CENTRE = np.array([0.013, -0.021, 0.034])
SMALL = [K.random_mesh(V) for V in (63, 257, 1025)] + [K.one_cell(), K.distinct_cells()] + list(K.crafted().values())


def test_counts_are_consistent():
    for case in SMALL:
        a, kw = K.args(case)
        v, n, c, t, info = R.cluster(*a, **kw)
        assert info["n_triangles"] + info["n_degenerate"] + info["n_duplicate"] + info["n_invalid_triangles"] == info["n_triangles_in"]
        assert (info["n_vertices"], info["n_triangles"]) == (len(v), len(t)) and info["n_vertices"] <= info["n_cells"] <= info["n_vertices_in"] - info["n_invalid_vertices"]
        assert (info["n_vertices_in"], info["n_triangles_in"]) == (len(case["vertices"]), len(case["triangles"]))
        if len(t):
            tt = t.astype(np.int64)
            assert tt.max() < len(v) and len(np.unique(tt)) == len(v)                  # every output vertex is referenced
            assert (tt[:, 0] != tt[:, 1]).all() and (tt[:, 1] != tt[:, 2]).all() and (tt[:, 0] != tt[:, 2]).all()
        if n is not None:
            ln = np.linalg.norm(n.astype(np.float64), axis=1)
            assert np.isfinite(n).all() and ((np.abs(ln - 1) < 1e-6) | (ln == 0)).all()
        if c is not None:
            assert np.isin(c[:, 3], (0, 255)).all() and (c[c[:, 3] == 0] == 0).all()


def test_every_output_vertex_lies_near_its_members():
    """Within cell_size sqrt(3), the diagonal of the cell, plus four ulp of the coordinate."""
    for case in SMALL:
        a, kw = K.args(case)
        v, _, _, _, info, rank = R.cluster(*a, **kw, members=True)
        mem = np.nonzero(rank >= 0)[0]
        if not len(mem):
            continue
        p = case["vertices"][mem].astype(np.float64); q = v[rank[mem]].astype(np.float64)
        bound = case["cell_size"] * np.sqrt(3.0) + 4 * np.spacing(np.abs(case["vertices"][mem]).max(1).astype(f32)).astype(np.float64)
        assert (np.linalg.norm(p - q, axis=1) <= bound).all()


def _rows(a):
    return np.unique(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1), axis=0) if len(a) else np.zeros((0, 0), np.uint8)


def _triangle_positions(v, t):
    """Every triangle as nine floats, rotated so that its smallest corner (as bytes) comes first; as a sorted array of rows."""
    if not len(t):
        return np.zeros((0, 36), np.uint8)
    p = v[t.astype(np.int64)].view(np.uint32).astype(np.int64)                          # (T, 3, 3)
    key = (p[:, :, 0] << 42) ^ (p[:, :, 1] << 21) ^ p[:, :, 2]
    k = np.argmin(key, axis=1)
    p = np.take_along_axis(p, ((k[:, None] + np.arange(3)[None, :]) % 3)[:, :, None], axis=1)
    return np.unique(p.reshape(len(t), 9), axis=0)


def test_input_order_does_not_change_the_result():
    """Permuting the vertices, with the triangles re-indexed: the SET of output positions, normals and colours is unchanged, and so is the set
    of triangles as position triples.  (Which of two equal triangles survives depends on the order; what it is does not.)"""
    for case in [K.random_mesh(257), K.random_mesh(1025), K.one_cell(), K.distinct_cells()]:
        a, kw = K.args(case)
        v, n, c, t, info = R.cluster(*a, **kw)
        rng = np.random.default_rng(1)
        V = len(case["vertices"])
        perm = rng.permutation(V)                                                       # new index j holds old vertex perm[j]
        new_of_old = np.empty(V, np.int64); new_of_old[perm] = np.arange(V)
        tri = case["triangles"].astype(np.int64)
        tri2 = np.where(tri < V, new_of_old[np.minimum(tri, V - 1)], tri)
        tri2 = tri2[rng.permutation(len(tri2))]
        v2, n2, c2, t2, info2 = R.cluster(case["vertices"][perm], tri2, case["cell_size"], origin=case["origin"], normals=case["normals"][perm], colors=case["colors"][perm])
        assert info2 == info
        both = lambda x, y, z: np.concatenate([x.view(np.uint32), y.view(np.uint32), z.view(np.uint32)[:, None] if z.ndim == 1 else z.view(np.uint32)], 1)
        assert np.array_equal(_rows(both(v, n, c)), _rows(both(v2, n2, c2)))
        assert np.array_equal(_triangle_positions(v, t), _triangle_positions(v2, t2))


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_analytic_surfaces_lose_triangles_and_keep_their_shape(name):
    """The 20^3 sphere and torus of tests/test_tsdf_mesh_host.py at cells of 2 and 3 voxels: fewer triangles, nothing invalid, every normal
    within 90 degrees of the outward direction.  The reduction and the change of the enclosed volume are printed."""
    fn = TM.sphere(CENTRE, 0.6) if name == "sphere" else TM.torus(CENTRE, 0.55, 0.25)
    vol = TM.analytic_volume(fn)
    vert, nrm, tris = TM.mesh(vol)
    vol_in = TM.signed_volume(vert, tris)
    for cells in (2, 3):
        v, n, _, t, info = R.cluster(vert, tris, cells * 0.1, normals=nrm, origin=(-0.95, -0.95, -0.95))
        vol_out = TM.signed_volume(v, t)
        print("%s, cells of %d voxels: V %d -> %d, T %d -> %d (x %.1f), degenerate %d, duplicate %d, enclosed volume %.4f -> %.4f (%+.1f %%)"
              % (name, cells, len(vert), len(v), len(tris), len(t), len(tris) / len(t), info["n_degenerate"], info["n_duplicate"], vol_in, vol_out,
                 100 * (vol_out - vol_in) / vol_in))
        assert 0 < len(t) < len(tris)
        assert info["n_invalid_vertices"] == 0 and info["n_invalid_triangles"] == 0
        q = v.astype(np.float64) - CENTRE
        if name == "sphere":
            radial = q
        else:
            radial = q - np.concatenate([q[:, :2] / np.linalg.norm(q[:, :2], axis=1, keepdims=True) * 0.55, np.zeros((len(q), 1))], 1)
        assert (np.einsum("ij,ij->i", n.astype(np.float64), radial) > 0).all()
