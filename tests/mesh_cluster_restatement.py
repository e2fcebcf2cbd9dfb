"""icp_mesh_cluster restated in numpy (the contract: include/icp_hip.h): np.unique over the cell keys with first
indices, integer sums, the canonical triples.  Every fp32 operation is one numpy float32 operation, in the contract's order.  The GPU tests
compare with it exactly; no tolerance appears anywhere."""
import numpy as np

f32 = np.float32
RANGE = 1 << 20
INFO_KEYS = ("n_vertices_in", "n_triangles_in", "n_invalid_vertices", "n_invalid_triangles", "n_cells", "n_vertices", "n_triangles", "n_degenerate", "n_duplicate")


def cells(vertices, cell_size, origin=(0, 0, 0)):
    """(valid (V,), cell (V, 3) int64, offset q (V, 3) int64); cell and offset are 0 for an invalid vertex."""
    v = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    o = np.asarray(origin, f32); cs = f32(cell_size)
    with np.errstate(all="ignore"):
        g = (v - o) / cs
        f = np.floor(g)
        valid = np.isfinite(v).all(1) & ((f >= f32(-RANGE)) & (f < f32(RANGE))).all(1)
        frac = (g - f) * f32(65536.0)
    c = np.where(valid[:, None], f, 0).astype(np.int64)
    q = np.where(valid[:, None], frac, 0).astype(np.int64)      # (int) truncates; the values are >= 0
    return valid, c, q


def cell_key(c):
    return ((c[:, 2] + RANGE) << 42) | ((c[:, 1] + RANGE) << 21) | (c[:, 0] + RANGE)


def _sums(rank, n_out, values):
    """Integer sums of `values` (n,) or (n, 3) into n_out bins by rank."""
    out = np.zeros((n_out,) + values.shape[1:], np.int64)
    np.add.at(out, rank, values.astype(np.int64))
    return out


def cluster(vertices, triangles, cell_size, normals=None, colors=None, origin=(0, 0, 0), members=False):
    """Returns (vertices (V', 3) f32, normals | None, colors | None, triangles (T', 3) u32, info dict) -- and with members=True a sixth
    value, the output index of every input vertex (-1: invalid, or its cluster is not referenced)."""
    v = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    V, T = len(v), len(t)
    o = np.asarray(origin, f32); cs = f32(cell_size)
    valid, c, q = cells(v, cell_size, origin)
    # clusters: the valid vertices of one cell; identity = first member
    iv = np.nonzero(valid)[0]
    uk, first_pos, inv = np.unique(cell_key(c[iv]), return_index=True, return_inverse=True)
    first_of_cell = iv[first_pos]                               # (np.unique's indices are those of the first occurrences)
    first = np.full(V, -1, np.int64)                            # per vertex: the first member of its cluster
    first[iv] = first_of_cell[inv.reshape(-1)]
    # triangles
    inb = t < V
    corner_first = np.where(inb, first[np.where(inb, t, 0)], -1) if V else np.full((T, 3), -1, np.int64)
    t_invalid = (corner_first < 0).any(1)
    F = corner_first
    t_degenerate = ~t_invalid & ((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2]))
    live = np.nonzero(~t_invalid & ~t_degenerate)[0]
    k = np.argmin(F[live], axis=1)
    canon = np.take_along_axis(F[live], (k[:, None] + np.arange(3)[None, :]) % 3, axis=1)      # rotated, never mirrored
    if len(live):
        _, first_occ = np.unique(canon, axis=0, return_index=True)
        survivors = np.sort(live[first_occ])
    else:
        survivors = live
    # output vertices: the referenced clusters in ascending first member
    ref_first = np.unique(F[survivors])
    nv, nt = len(ref_first), len(survivors)
    tris_out = np.searchsorted(ref_first, F[survivors]).astype(np.uint32).reshape(-1, 3)
    rank = np.full(V, -1, np.int64)
    pos = np.searchsorted(ref_first, first[iv])
    hit = (pos < nv) & (ref_first[np.minimum(pos, max(nv - 1, 0))] == first[iv]) if nv else np.zeros(len(iv), bool)
    rank[iv[hit]] = pos[hit]
    mem = np.nonzero(rank >= 0)[0]
    r = rank[mem]
    n = _sums(r, nv, np.ones(len(mem), np.int64))
    S = _sums(r, nv, q[mem])
    Q = (2 * S + n[:, None]) // (2 * n[:, None]) if nv else np.zeros((0, 3), np.int64)
    cc = c[ref_first].astype(f32)
    vert_out = (o + (cc + Q.astype(f32) * f32(2.0 ** -16)) * cs).astype(f32)
    nrm_out = col_out = None
    if normals is not None:
        nr = np.ascontiguousarray(normals, f32).reshape(-1, 3)[mem]
        with np.errstate(all="ignore"):
            fin = np.isfinite(nr).all(1)
            m = np.where(fin[:, None], np.rint(np.minimum(np.maximum(nr, f32(-1)), f32(1)) * f32(32767.0)), 0).astype(np.int64)
            N = _sums(r, nv, m).astype(f32)
            length = np.sqrt(N[:, 0] * N[:, 0] + (N[:, 1] * N[:, 1] + N[:, 2] * N[:, 2]))
            nrm_out = (N / length[:, None]).astype(f32)
            nrm_out[~np.isfinite(nrm_out).all(1)] = 0
    if colors is not None:
        co = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)[mem].astype(np.int64)
        has = co[:, 3] != 0
        kk = _sums(r[has], nv, np.ones(int(has.sum()), np.int64))
        Cs = _sums(r[has], nv, co[has, :3])
        col_out = np.zeros((nv, 4), np.uint8)
        w = kk > 0
        col_out[w, :3] = ((2 * Cs[w] + kk[w, None]) // (2 * kk[w, None])).astype(np.uint8)
        col_out[w, 3] = 255
    info = dict(n_vertices_in=V, n_triangles_in=T, n_invalid_vertices=int((~valid).sum()), n_invalid_triangles=int(t_invalid.sum()), n_cells=len(uk),
                n_vertices=nv, n_triangles=nt, n_degenerate=int(t_degenerate.sum()), n_duplicate=len(live) - nt)
    out = (vert_out.reshape(-1, 3), nrm_out, col_out, tris_out, info)
    return out + (rank,) if members else out
