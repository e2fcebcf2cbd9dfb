"""The icp_tsdf_mesh_hashed contract of include/icp_hip.h restated in numpy fp32: the zero level set of a HASHED TSDF volume (blocks of
8 x 8 x 8 voxels at signed block coordinates) as an indexed triangle mesh, in the contract's order -- blocks in ascending key order (z, then y,
then x), voxels in local linear order inside a block.  Written from the contract; the table and the small helpers are those of
tests/tsdf_mesh_restatement.py.  Every fp32 operation is one numpy float32 operation in the order the contract writes it, positions from
o + f32(g) * s with g the signed global voxel coordinate, so the device is compared bit for bit.  Contains no device code.

The blocks are laid out over their bounding box with a margin of one voxel (a voxel no block covers reads (0, 0)); that array is scratch of
this file only -- nothing of the result depends on it, and the order is taken from (block rank, local index), never from the array's."""
import numpy as np

from tsdf_mesh_restatement import table_arrays, tet_corners, _shift, _lerp

f32 = np.float32


def sort_blocks(coords):
    """The permutation that puts block coordinates (B, 3) into ascending key order: z, then y, then x."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    return np.lexsort((c[:, 0], c[:, 1], c[:, 2]))


def from_dict(blocks):
    """{(bx, by, bz): (tsdf (8, 8, 8), weight (8, 8, 8))}, indexed [z, y, x] -> (coords, tsdf, weight) in the dict's order."""
    keys = list(blocks)
    coords = np.array(keys, np.int32).reshape(-1, 3)
    t = np.array([blocks[k][0] for k in keys], f32).reshape(-1, 8, 8, 8); w = np.array([blocks[k][1] for k in keys], f32).reshape(-1, 8, 8, 8)
    return coords, t, w


def mesh(coords, tsdf, weight, origin, voxel_size, min_weight=0.0, stats=None):
    """coords (B, 3) block coordinates in any order, tsdf / weight (B, 8, 8, 8) indexed [z, y, x] (Context.tsdf_blocks' arrays).
    Returns (vertices (V, 3) f32, normals (V, 3) f32, triangles (T, 3) u32).  stats (a dict, optional) receives counts the tests use:
    cells_spanning[1 | 2 | 4 | 8] -- cells with triangles by the number of blocks their corners lie in -- and vertices_held_below, the
    vertices whose holding cell lies in another (lower) block than their owner."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    tsdf = np.asarray(tsdf, f32).reshape(-1, 8, 8, 8); weight = np.asarray(weight, f32).reshape(-1, 8, 8, 8)
    o = np.asarray(origin, f32); s = f32(voxel_size)
    empty = (np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32))
    if stats is not None:
        stats.update(cells_spanning={1: 0, 2: 0, 4: 0, 8: 0}, vertices_held_below=0)
    if len(coords) == 0:
        return empty
    order = sort_blocks(coords)
    coords, tsdf, weight = coords[order], tsdf[order], weight[order]
    lo = coords.min(0) * 8 - 1                                   # the array's voxel (0, 0, 0) as a global coordinate: one voxel of margin
    nx, ny, nz = (int(v) for v in (coords.max(0) + 1) * 8 + 1 - lo)
    F = np.zeros((nz, ny, nx), f32); W = np.zeros((nz, ny, nx), f32)
    sortkey = np.full((nz, ny, nx), -1, np.int64)               # rank * 512 + local; -1 where no block is
    local = np.arange(512).reshape(8, 8, 8)
    for rank, (b, t, w) in enumerate(zip(coords, tsdf, weight)):
        x0, y0, z0 = (int(v) for v in b * 8 - lo)
        F[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = t; W[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = w
        sortkey[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = rank * 512 + local
    N = nx * ny * nz
    with np.errstate(all="ignore"):
        obs = (W > 0) & (W >= f32(min_weight)) & np.isfinite(F)
        neg = F < 0
    valid = np.ones(obs.shape, bool)
    for c in range(8):
        valid &= _shift(obs, c >> 2, (c >> 1) & 1, c & 1)
    # ---- which edges carry a vertex: has[a, code - 1], a the array's linear index
    has = np.zeros((N, 7), bool)
    for code in range(1, 8):
        d = (code & 1, (code >> 1) & 1, code >> 2)
        cross = neg != _shift(neg, d[2], d[1], d[0])
        cell = np.zeros(F.shape, bool)
        for off in range(8):
            if off & code:
                continue
            cell |= _shift(valid, -(off >> 2), -((off >> 1) & 1), -(off & 1))
        has[:, code - 1] = (cross & cell).reshape(-1)
    key = sortkey.reshape(-1)
    va, vc = np.nonzero(has)
    assert (key[va] >= 0).all()                                  # an owner is observed, so its block exists
    perm = np.lexsort((vc, key[va]))                             # ascending (rank, local), then code
    va, vc = va[perm], vc[perm] + 1
    V = len(va)
    vid = np.full((N, 7), -1, np.int64)
    vid[va, vc - 1] = np.arange(V)
    ia = [va % nx, (va // nx) % ny, va // (nx * ny)]             # array coordinates
    d = [vc & 1, (vc >> 1) & 1, vc >> 2]
    stride = [1, nx, nx * ny]
    Ff = F.reshape(-1)
    with np.errstate(all="ignore"):
        Fv = Ff[va]; Fd = Ff[va + d[0] + d[1] * nx + d[2] * nx * ny]
        t = Fv / (Fv - Fd)
        ts = t * s
        vert = np.empty((V, 3), f32)
        for r in range(3):
            g = ia[r] + lo[r]                                    # the signed global coordinate
            base = o[r] + g.astype(f32) * s
            vert[:, r] = np.where(d[r] == 1, base + ts, base)
        # ---- normals: the first valid cell, in ascending off, that contains the edge
        vf = valid.reshape(-1)
        cell_a = np.full(V, -1, np.int64); cell_off = np.zeros(V, np.int64)
        for off in range(7):
            oo = (off & 1, (off >> 1) & 1, off >> 2)
            ok = (cell_a < 0) & ((vc & off) == 0)
            cand = va - (oo[0] + oo[1] * nx + oo[2] * nx * ny)
            ok &= vf[np.where(ok, cand, 0)]
            cell_a[ok] = cand[ok]; cell_off[ok] = off
        assert (cell_a >= 0).all()
        c = [Ff[cell_a + (k & 1) + ((k >> 1) & 1) * nx + (k >> 2) * nx * ny] for k in range(8)]
        tx, ty, tz = [np.where(d[r] == 1, t, ((cell_off >> r) & 1).astype(f32)).astype(f32) for r in range(3)]
        gx = _lerp(_lerp(c[1] - c[0], c[3] - c[2], ty), _lerp(c[5] - c[4], c[7] - c[6], ty), tz)
        gy = _lerp(_lerp(c[2] - c[0], c[3] - c[1], tx), _lerp(c[6] - c[4], c[7] - c[5], tx), tz)
        gz = _lerp(_lerp(c[4] - c[0], c[5] - c[1], tx), _lerp(c[6] - c[2], c[7] - c[3], tx), ty)
        ln = np.sqrt(gx * gx + (gy * gy + gz * gz))
        nrm = np.stack([gx / ln, gy / ln, gz / ln], 1).astype(f32).reshape(V, 3)
        nrm[~np.isfinite(nrm).all(1)] = 0
    # ---- triangles: valid cells in ascending (rank, local) of their lowest corner, the six tetrahedra, the table's order
    cnt, own, code = table_arrays()
    Q = tet_corners()
    ca = np.nonzero(vf)[0]
    assert (key[ca] >= 0).all()
    ca = ca[np.argsort(key[ca], kind="stable")]
    negf = neg.reshape(-1)
    tri = np.zeros((len(ca), 6, 2, 3), np.int64); keep = np.zeros((len(ca), 6, 2), bool)
    for p in range(6):
        m = np.zeros(len(ca), np.int64)
        for a in range(4):
            q = Q[p, a]
            m |= negf[ca + q[0] + q[1] * nx + q[2] * nx * ny].astype(np.int64) << a
        n = cnt[p][m]
        keep[:, p, 0] = n >= 1; keep[:, p, 1] = n >= 2
        ow = own[p][m]; e = code[p][m]
        owner = ca[:, None, None] + (ow & 1) + ((ow >> 1) & 1) * nx + (ow >> 2) * nx * ny
        idx = vid[owner, e - 1]
        assert (idx[keep[:, p]] >= 0).all()                      # every triangle corner is a vertex
        tri[:, p] = idx
    tris = tri[keep].astype(np.uint32).reshape(-1, 3)
    if stats is not None:
        crossing = ca[keep.reshape(len(ca), -1).any(1)]
        loc = key[crossing] & 511
        n7 = ((loc & 7) == 7).astype(int) + (((loc >> 3) & 7) == 7).astype(int) + ((loc >> 6) == 7).astype(int)
        stats["cells_spanning"] = {1 << k: int((n7 == k).sum()) for k in range(4)}
        stats["vertices_held_below"] = int((key[cell_a] >> 9 != key[va] >> 9).sum())
    return vert, nrm, tris


def mesh_blocks(blocks, origin, voxel_size, min_weight=0.0, stats=None):
    """`mesh` over a dict {(bx, by, bz): (tsdf, weight)}."""
    return mesh(*from_dict(blocks), origin, voxel_size, min_weight, stats)


def triangle_rows(vert, nrm, tris):
    """The mesh as a sorted multiset of triangles, free of the order of vertices and triangles: each triangle its three corners' positions
    and normals as 18 uint32 bit patterns, rotated so that its smallest corner comes first (the orientation kept), the rows sorted."""
    v = np.ascontiguousarray(vert, f32).view(np.uint32).reshape(-1, 3); n = np.ascontiguousarray(nrm, f32).view(np.uint32).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    if len(t) == 0:
        return np.zeros((0, 18), np.uint32)
    corner = np.concatenate([v[t], n[t]], 2).astype(np.int64)      # (T, 3, 6)
    first = np.zeros(len(t), np.int64)
    for k in (1, 2):                                             # lexicographic minimum of the three corners
        a, b = corner[np.arange(len(t)), k], corner[np.arange(len(t)), first]
        diff = a != b
        col = np.argmax(diff, 1)
        less = diff.any(1) & (a[np.arange(len(t)), col] < b[np.arange(len(t)), col])
        first[less] = k
    rows = np.stack([corner[np.arange(len(t)), (first + k) % 3] for k in range(3)], 1).reshape(len(t), 18)
    rows = rows[np.lexsort(rows.T[::-1])]
    return rows.astype(np.uint32)
