"""The icp_tsdf_mesh contract of include/icp_hip.h restated in numpy fp32: the zero level set of a TSDF volume as an indexed triangle mesh,
by the six tetrahedra of the Kuhn triangulation of every cell.  Written from the contract alone; the case table is generated from its
rule (permutations, edge ranks, the midpoint orientation test), every fp32 operation is one numpy float32 operation in the order the
contract writes it, so the device is compared bit for bit.  Contains no device code."""
import itertools
import numpy as np

from tsdf_restatement import Volume  # noqa: F401  (the volume the mesh is taken from)

f32 = np.float32
EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]            # local edge ranks 0..5
PERMS = sorted(itertools.permutations(range(3)))                     # xyz, xzy, yxz, yzx, zxy, zyx


def tet_corners():
    """(6, 4, 3) int: corner q_a of tetrahedron pi as an offset in {0,1}^3 (x, y, z)."""
    out = np.zeros((6, 4, 3), np.int64)
    for p, pi in enumerate(PERMS):
        out[p, 1, pi[0]] = 1
        out[p, 2, pi[0]] = 1; out[p, 2, pi[1]] = 1
        out[p, 3] = 1
    return out


def _rank(a, b):
    return EDGES.index((min(a, b), max(a, b)))


def tet_table():
    """The case table from the rule: table[p][m] = list of triangles, each three local edge ranks, for tetrahedron p and case mask m."""
    Q = tet_corners()
    table = []
    for p in range(6):
        mid = [(Q[p, a] + Q[p, b]) / 2.0 for a, b in EDGES]
        row = []
        for m in range(16):
            neg = [a for a in range(4) if (m >> a) & 1]
            pos = [a for a in range(4) if not (m >> a) & 1]
            if not neg or not pos:
                row.append([])
                continue
            if len(neg) == 1 or len(pos) == 1:
                lone = neg[0] if len(neg) == 1 else pos[0]
                cyc = sorted(r for r, e in enumerate(EDGES) if lone in e)
            else:
                (a, b), (c, d) = neg, pos
                cyc = [_rank(a, c), _rank(a, d), _rank(b, d), _rank(b, c)]
                s = cyc.index(min(cyc))
                cyc = cyc[s:] + cyc[:s]
            tris = [(cyc[0], cyc[1], cyc[2])] + ([(cyc[0], cyc[2], cyc[3])] if len(cyc) == 4 else [])
            free = np.mean([Q[p, a] for a in pos], axis=0) - np.mean([Q[p, a] for a in neg], axis=0)
            nrm = np.zeros(3)
            for t in tris:
                nrm = np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]])
                if nrm.any():
                    break
            if nrm @ free < 0:
                cyc = [cyc[0]] + cyc[:0:-1]
                tris = [(cyc[0], cyc[1], cyc[2])] + ([(cyc[0], cyc[2], cyc[3])] if len(cyc) == 4 else [])
            row.append(tris)
        table.append(row)
    return table


def table_arrays():
    """The table as arrays: count (6, 16), owner corner code (6, 16, 2, 3) and edge code (6, 16, 2, 3) of every triangle vertex; a corner
    or edge code is d_x + 2 d_y + 4 d_z.  The local edge (a, b), a < b, runs from corner q_a (its owner's offset in the cell) along q_b - q_a."""
    Q = tet_corners()
    T = tet_table()
    cnt = np.zeros((6, 16), np.int64); own = np.zeros((6, 16, 2, 3), np.int64); code = np.ones((6, 16, 2, 3), np.int64)
    w = np.array([1, 2, 4])
    for p in range(6):
        for m in range(16):
            cnt[p, m] = len(T[p][m])
            for t, tri in enumerate(T[p][m]):
                for s, e in enumerate(tri):
                    a, b = EDGES[e]
                    own[p, m, t, s] = Q[p, a] @ w
                    code[p, m, t, s] = (Q[p, b] - Q[p, a]) @ w
    return cnt, own, code


def _lerp(a, b, t):
    return a + t * (b - a)


def _shift(a, dz, dy, dx, fill=False):
    """a[k + dz, j + dy, i + dx] with `fill` outside; offsets in {-1, 0, 1}."""
    out = np.full(a.shape, fill, a.dtype)
    nz, ny, nx = a.shape
    def sl(d, n):
        return (slice(max(d, 0), n + min(d, 0)), slice(max(-d, 0), n + min(-d, 0)))
    (sz, tz), (sy, ty), (sx, tx) = sl(dz, nz), sl(dy, ny), sl(dx, nx)
    out[tz, ty, tx] = a[sz, sy, sx]
    return out


def observed(vol, min_weight=0.0):
    with np.errstate(all="ignore"):
        return (vol.weight > 0) & (vol.weight >= f32(min_weight)) & np.isfinite(vol.tsdf)


def valid_cells(vol, min_weight=0.0):
    """(nz, ny, nx) bool: the cell whose lowest corner is the voxel is in range with its eight corners observed."""
    obs = observed(vol, min_weight)
    v = np.ones(obs.shape, bool)
    for c in range(8):
        v &= _shift(obs, c >> 2, (c >> 1) & 1, c & 1)
    return v


def mesh(vol, min_weight=0.0):
    """Returns (vertices (V, 3) f32, normals (V, 3) f32, triangles (T, 3) u32)."""
    nx, ny, nz = vol.nx, vol.ny, vol.nz
    N = nx * ny * nz
    F = vol.tsdf
    with np.errstate(all="ignore"):
        neg = F < 0
    valid = valid_cells(vol, min_weight)
    # ---- which edges carry a vertex: has[l, code - 1]
    has = np.zeros((N, 7), bool)
    for code in range(1, 8):
        d = (code & 1, (code >> 1) & 1, code >> 2)
        inside = _shift(np.ones(F.shape, bool), d[2], d[1], d[0])
        cross = inside & (neg != _shift(neg, d[2], d[1], d[0]))
        cell = np.zeros(F.shape, bool)
        for off in range(8):
            o = (off & 1, (off >> 1) & 1, off >> 2)
            if any(o[r] and d[r] for r in range(3)):
                continue
            cell |= _shift(valid, -o[2], -o[1], -o[0])
        has[:, code - 1] = (cross & cell).reshape(-1)
    vid = np.cumsum(has.reshape(-1)).reshape(N, 7) - 1
    vl, vc = np.nonzero(has)                                 # ascending owner linear index, then ascending code
    vc = vc + 1
    V = len(vl)
    i = [vl % nx, (vl // nx) % ny, vl // (nx * ny)]
    d = [vc & 1, (vc >> 1) & 1, vc >> 2]
    Ff = F.reshape(-1)
    stride = [1, nx, nx * ny]
    with np.errstate(all="ignore"):
        Fv = Ff[vl]; Fd = Ff[vl + d[0] + d[1] * nx + d[2] * nx * ny]
        t = Fv / (Fv - Fd)
        ts = t * vol.s
        vert = np.empty((V, 3), f32)
        for r in range(3):
            base = vol.o[r] + i[r].astype(f32) * vol.s
            vert[:, r] = np.where(d[r] == 1, base + ts, base)
        # ---- normals: the first valid cell that contains the edge
        vf = valid.reshape(-1)
        cell_l = np.full(V, -1, np.int64); cell_off = np.zeros(V, np.int64)
        for off in range(8):
            o = (off & 1, (off >> 1) & 1, off >> 2)
            ok = cell_l < 0
            for r in range(3):
                if o[r]:
                    ok &= (d[r] == 0) & (i[r] >= 1)
            cand = vl - (o[0] + o[1] * nx + o[2] * nx * ny)
            ok &= vf[np.where(ok, cand, 0)]
            cell_l[ok] = cand[ok]; cell_off[ok] = off
        assert (cell_l >= 0).all()
        c = [Ff[cell_l + (k & 1) + ((k >> 1) & 1) * nx + (k >> 2) * nx * ny] for k in range(8)]
        tx, ty, tz = [np.where(d[r] == 1, t, ((cell_off >> r) & 1).astype(f32)).astype(f32) for r in range(3)]
        gx = _lerp(_lerp(c[1] - c[0], c[3] - c[2], ty), _lerp(c[5] - c[4], c[7] - c[6], ty), tz)
        gy = _lerp(_lerp(c[2] - c[0], c[3] - c[1], tx), _lerp(c[6] - c[4], c[7] - c[5], tx), tz)
        gz = _lerp(_lerp(c[4] - c[0], c[5] - c[1], tx), _lerp(c[6] - c[2], c[7] - c[3], tx), ty)
        ln = np.sqrt(gx * gx + (gy * gy + gz * gz))
        nrm = np.stack([gx / ln, gy / ln, gz / ln], 1).astype(f32)
        nrm[~np.isfinite(nrm).all(1)] = 0
    # ---- triangles: valid cells in ascending linear index, the six tetrahedra, the table's order
    cnt, own, code = table_arrays()
    Q = tet_corners()
    cl = np.nonzero(valid.reshape(-1))[0]
    negf = neg.reshape(-1)
    tri = np.zeros((len(cl), 6, 2, 3), np.int64); keep = np.zeros((len(cl), 6, 2), bool)
    for p in range(6):
        m = np.zeros(len(cl), np.int64)
        for a in range(4):
            q = Q[p, a]
            m |= negf[cl + q[0] + q[1] * nx + q[2] * nx * ny].astype(np.int64) << a
        n = cnt[p][m]
        keep[:, p, 0] = n >= 1; keep[:, p, 1] = n >= 2
        o = own[p][m]; e = code[p][m]                                # (ncell, 2, 3)
        owner = cl[:, None, None] + (o & 1) + ((o >> 1) & 1) * nx + (o >> 2) * nx * ny
        idx = vid[owner, e - 1]
        assert has[owner, e - 1][keep[:, p]].all()                   # every triangle corner is a vertex
        tri[:, p] = idx
    tris = tri[keep].astype(np.uint32).reshape(-1, 3)
    return vert, nrm, tris


# ---- what the tests measure on a mesh

def edge_counts(tris):
    """(undirected edge -> number of triangles, number of directed edges that appear more than once)."""
    t = np.asarray(tris, np.int64)
    de = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = de[:, 0] * (t.max() + 1 if len(t) else 1) + de[:, 1]
    _, dc = np.unique(key, return_counts=True)
    ue = np.sort(de, axis=1)
    _, uc = np.unique(ue[:, 0] * (t.max() + 1 if len(t) else 1) + ue[:, 1], return_counts=True)
    return uc, int((dc > 1).sum())


def signed_volume(vert, tris):
    v = np.asarray(vert, np.float64); t = np.asarray(tris, np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


# ---- analytic volumes the tests take meshes from: the signed distance written straight into a Volume, all weights 1

def analytic_volume(fn, dims=(20, 20, 20), s=0.1, origin=(-0.95, -0.95, -0.95)):
    vol = Volume(dims, origin, voxel_size=s)
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    P = np.stack([origin[0] + x * s, origin[1] + y * s, origin[2] + z * s], -1)
    vol.tsdf = fn(P).astype(f32); vol.weight = np.ones_like(vol.tsdf)
    return vol


def sphere(centre, r):
    return lambda P: np.linalg.norm(P - np.asarray(centre), axis=-1) - r


def torus(centre, R, r):
    def fn(P):
        q = P - np.asarray(centre)
        return np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - R) ** 2 + q[..., 2] ** 2) - r
    return fn
