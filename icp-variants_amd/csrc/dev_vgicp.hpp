// dev_vgicp.hpp -- voxelized GICP (Koide, Yokozuka, Oishi, Banno, ICRA 2021): the target reduced once to a dense grid of cells, each a mean
// and a normalised sum of plane covariances; a moved source point looks up the ONE cell it falls in and is scored by GICP's plane-to-plane
// Mahalanobis distance against it: no index, no search.  Contract: include/icp_hip.h; tests/vgicp_restatement.py states
// the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_gicp.hpp and dev_sdf.hpp).
// ------------------------------------------------------------------------------------------------
// The grid build sums INTEGERS per cell (a count, three quantised offsets from the cell's centre, six products of quantised normal
// components): exact in any order, so integer atomics keep the build bit-reproducible.  The iterations are section 6q's: the pose lives in
// SdfState, k_vgicp_accumulate reads it there, k_sdf_solve (launched as it is) folds the partials, solves and writes the next one, and once
// SdfState::stop is set every launch still queued returns on its first instructions.  No floating-point atomics anywhere.
constexpr int VG_CLAMP = 1 << 30;                   // cell coordinates are clamped to +-2^30: the conversion to int is always defined
constexpr int VG_NSUM = 9;                          // int64 sums per cell: sum q (3), sum m_a m_b for a <= b (6)
struct VgBox { int lo[3], hi[3], n_enter, n_occupied; };
struct VgTarget { const float* x; const float* y; const float* z; const float* nx; const float* ny; const float* nz; int n; float vs; };
struct VgGrid { int lo[3], dims[3]; float vs; int min_points; };

__device__ __forceinline__ int vg_cell_coord(float p, float vs) {
    const float c = floorf(p / vs);
    return (int)fminf(fmaxf(c, -(float)VG_CLAMP), (float)VG_CLAMP);      // (a NaN never gets here: every caller has tested finiteness)
}
// linear cell index of the coordinates c, or -1 outside the grid (unsigned differences: +-2^30 - lo cannot trap)
__device__ __forceinline__ int vg_cell_index(const int (&lo)[3], const int (&dims)[3], int cx, int cy, int cz) {
    const unsigned ix = (unsigned)cx - (unsigned)lo[0], iy = (unsigned)cy - (unsigned)lo[1], iz = (unsigned)cz - (unsigned)lo[2];
    if (ix >= (unsigned)dims[0] || iy >= (unsigned)dims[1] || iz >= (unsigned)dims[2]) return -1;
    return (int)((iz * (unsigned)dims[1] + iy) * (unsigned)dims[0] + ix);
}
__device__ __forceinline__ bool vg_enters(const VgTarget& t, int i, float& px, float& py, float& pz, float& nx, float& ny, float& nz) {
    px = t.x[i]; py = t.y[i]; pz = t.z[i]; nx = t.nx[i]; ny = t.ny[i]; nz = t.nz[i];
    return finite3(px, py, pz) && finite3(nx, ny, nz);
}

__global__ void k_vg_box_init(VgBox* box) {
    const int t = threadIdx.x;
    if (t < 3) { box->lo[t] = INT_MAX; box->hi[t] = INT_MIN; }
    if (t == 3) { box->n_enter = 0; box->n_occupied = 0; }
}

// Bounds: per block the min / max of the entering points' cell coordinates (shuffle tree per wave, the four waves through LDS), then an
// integer atomicMin / atomicMax per axis -- issued only where the block's value would still move the bound it has just read: the bounds
// only ever tighten towards their final value, so a stale read can cost a redundant atomic, never a missed one.  (Six unconditional atomics
// per block, all blocks on the same six addresses, took 52 us at 1448 blocks; the streaming pass itself takes a tenth of that.)
__global__ __launch_bounds__(256) void k_vg_bounds(const VgTarget t, VgBox* __restrict__ box) {
    __shared__ int red[4][6];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = blockIdx.x * 256 + tid;
    int v[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    if (i < t.n) {
        float px, py, pz, nx, ny, nz;
        if (vg_enters(t, i, px, py, pz, nx, ny, nz)) {
            v[0] = v[3] = vg_cell_coord(px, t.vs); v[1] = v[4] = vg_cell_coord(py, t.vs); v[2] = v[5] = vg_cell_coord(pz, t.vs);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) { v[a] = min(v[a], __shfl_down(v[a], off, WAVE)); v[3 + a] = max(v[3 + a], __shfl_down(v[3 + a], off, WAVE)); }
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 6; a++) red[wave][a] = v[a];
    }
    __syncthreads();
    if (tid < 6) {
        const int a = red[0][tid], b = red[1][tid], c = red[2][tid], d = red[3][tid];
        if (tid < 3) {
            const int m = min(min(a, b), min(c, d));
            if (m < __hip_atomic_load(&box->lo[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&box->lo[tid], m);
        } else {
            const int m = max(max(a, b), max(c, d));
            if (m > __hip_atomic_load(&box->hi[tid - 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&box->hi[tid - 3], m);
        }
    }
}

// Accumulate into cells: one target point per lane over the resident order.  Neighbouring points of a scan mostly share a cell, and ten
// atomics per lane all landing on one address serialise; so the lanes of a wave are cut into RUNS of equal cell index, a segmented shuffle
// sum adds each run into its first lane, and only that lane issues the ten integer atomics.  The sums are integers: the grouping changes nothing.
__global__ __launch_bounds__(256) void k_vg_cells_add(const VgTarget t, const VgGrid g, int* __restrict__ count, unsigned long long* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int cell = -1, cnt = 0, q[3] = {0, 0, 0};
    long long mm[6] = {0, 0, 0, 0, 0, 0};
    if (i < t.n) {
        float p[3], nr[3];
        if (vg_enters(t, i, p[0], p[1], p[2], nr[0], nr[1], nr[2])) {
            int c[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                c[a] = vg_cell_coord(p[a], t.vs);
                const float off = ((p[a] - ((float)c[a] + 0.5f) * t.vs) / t.vs) * 65536.0f;
                q[a] = (int)lrintf(fminf(fmaxf(off, -32768.0f), 32768.0f));
            }
            cell = vg_cell_index(g.lo, g.dims, c[0], c[1], c[2]);      // (inside by construction of the bounds)
            if (cell >= 0) {
                cnt = 1;
                long long m[3];
#pragma unroll
                for (int a = 0; a < 3; a++) m[a] = (long long)lrintf(fminf(fmaxf(nr[a], -2.0f), 2.0f) * 16384.0f);
                mm[0] = m[0] * m[0]; mm[1] = m[0] * m[1]; mm[2] = m[0] * m[2]; mm[3] = m[1] * m[1]; mm[4] = m[1] * m[2]; mm[5] = m[2] * m[2];
            } else { q[0] = q[1] = q[2] = 0; }
        }
    }
    // runs: a lane heads one when its cell differs from the lane before it; run = how many heads lie at or below the lane
    const int prev = __shfl_up(cell, 1, WAVE);
    const bool head = lane == 0 || prev != cell;
    const unsigned long long heads = __ballot(head);
    const int run = __popcll(heads & (~0ull >> (63 - lane)));
    for (int off = 1; off < WAVE; off <<= 1) {
        const bool same = __shfl_down(run, off, WAVE) == run && lane + off < WAVE;
        const int oc = __shfl_down(cnt, off, WAVE);
        int oq[3]; long long om[6];
#pragma unroll
        for (int a = 0; a < 3; a++) oq[a] = __shfl_down(q[a], off, WAVE);
#pragma unroll
        for (int a = 0; a < 6; a++) om[a] = __shfl_down(mm[a], off, WAVE);
        if (same) {
            cnt += oc;
#pragma unroll
            for (int a = 0; a < 3; a++) q[a] += oq[a];       // (at most 64 x 32768)
#pragma unroll
            for (int a = 0; a < 6; a++) mm[a] += om[a];
        }
    }
    if (head && cell >= 0) {
        atomicAdd(&count[cell], cnt);
        unsigned long long* s = sums + (size_t)cell * VG_NSUM;
#pragma unroll
        for (int a = 0; a < 3; a++) atomicAdd(&s[a], (unsigned long long)(long long)q[a]);
#pragma unroll
        for (int a = 0; a < 6; a++) atomicAdd(&s[3 + a], (unsigned long long)mm[a]);
    }
}

// The record of cell i from its count n and its nine sums: fp64 from the integers, each of the nine values rounded once to fp32; nine
// floats and the count, 40 bytes, written as five 8-byte stores.  (k_vg_finalise, k_vmap_records)
__device__ __forceinline__ void vg_record(const VgGrid& g, int i, int n, const long long* __restrict__ sums, float2* __restrict__ cells) {
    float rec[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
        const long long* s = sums + (size_t)i * VG_NSUM;
        const int ix = i % g.dims[0], iy = (i / g.dims[0]) % g.dims[1], iz = i / (g.dims[0] * g.dims[1]);
        const int c[3] = {g.lo[0] + ix, g.lo[1] + iy, g.lo[2] + iz};
        const double vs = (double)g.vs, dn = (double)n;
#pragma unroll
        for (int a = 0; a < 3; a++) rec[a] = (float)(((double)c[a] + 0.5) * vs + ((double)s[a] / dn) * (vs / 65536.0));
        const long long tr = (s[3] + s[6]) + s[8];
        if (tr > 0) {
            const double dt = (double)tr;
#pragma unroll
            for (int a = 0; a < 6; a++) rec[3 + a] = (float)((double)s[3 + a] / dt);
        }
    }
    float2* o = cells + (size_t)i * 5;
    o[0] = make_float2(rec[0], rec[1]); o[1] = make_float2(rec[2], rec[3]); o[2] = make_float2(rec[4], rec[5]); o[3] = make_float2(rec[6], rec[7]);
    o[4] = make_float2(rec[8], __int_as_float(n));
}

// Finalise: one cell per lane, vg_record.  The occupied cells and the points that entered are counted here.
__global__ __launch_bounds__(256) void k_vg_finalise(const VgGrid g, int n_cells, const int* __restrict__ count, const long long* __restrict__ sums,
                                                     float2* __restrict__ cells, VgBox* __restrict__ box) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int n = 0;
    if (i < n_cells) {
        n = count[i];
        vg_record(g, i, n, sums, cells);
    }
    // per wave: the occupied cells by ballot, the points by a shuffle sum; one pair of atomics from the waves that have any
    const unsigned long long occ = __ballot(n > 0);
    int pts = n;
    for (int off = 32; off > 0; off >>= 1) pts += __shfl_down(pts, off, WAVE);
    if (lane == 0 && occ) { atomicAdd(&box->n_occupied, __popcll(occ)); atomicAdd(&box->n_enter, pts); }
}

constexpr int VG_POINTS_PER_LANE = 2;              // k_vgicp_accumulate: a block takes 2 x 256 consecutive source points
struct VgSource { const float* x; const float* y; const float* z; const float* nx; const float* ny; const float* nz; int n; double one_minus_eps; };

// entry e = 3 row + column of (R^-1)^T of the pose, fp64 cofactors rounded once: the operations of normal_matrix_from_pose on the same
// values, so nine lanes give the nine floats icp_transform_normals uses
__device__ __forceinline__ float vg_normal_matrix_entry(const float* __restrict__ pose, int e) {
    const double a = pose[0], b = pose[4], c = pose[8];
    const double d = pose[1], e_ = pose[5], f = pose[9];
    const double g = pose[2], h = pose[6], i = pose[10];
    const double c00 = e_ * i - f * h, c01 = f * g - d * i, c02 = d * h - e_ * g;
    const double det = (a * c00 + b * c01) + c * c02;
    double cof;
    switch (e) {
        case 0: cof = c00; break;  case 1: cof = c01; break;  case 2: cof = c02; break;
        case 3: cof = c * h - b * i; break;  case 4: cof = a * i - c * g; break;  case 5: cof = b * g - a * h; break;
        case 6: cof = b * f - c * e_; break;  case 7: cof = c * d - a * f; break;  default: cof = a * e_ - b * d; break;
    }
    return (float)(cof / det);
}

// One source point per lane and pass over the SoA planes, VG_POINTS_PER_LANE passes of 256 consecutive points per block (half the blocks:
// half the partials k_sdf_solve's single block folds, which is the longer half of an iteration).  The lane moves its point and its GICP normal by the state's pose, finds
// its cell, and fetches the 40-byte record as five 8-byte loads issued together.  Sigma = 2I - (1 - eps)(S + b b^T), M = adj / det as
// gicp_accumulate; J = [-[p]x | I], r = mu - p, every term scaled by the cell's count.  The 28 terms of a lane are folded over the block by
// block_reduce_wide, the two counts by ballot and popcount: one column of partials[28][n_blocks] and of counts[2][n_blocks] per block.
__global__ __launch_bounds__(256) void k_vgicp_accumulate(const VgGrid g, const float2* __restrict__ cells, const VgSource s, const SdfState* __restrict__ st,
                                                          double* __restrict__ partials, int* __restrict__ counts) {
    __shared__ double lds[4 * SDF_NSUM * 17];
    __shared__ int red[8];
    __shared__ float nm[9];
    if (st->stop) return;                              // (uniform) the alignment has ended: nothing of this launch is needed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* __restrict__ P = st->pose;
    if (tid < 9) nm[tid] = vg_normal_matrix_entry(P, tid);
    __syncthreads();
    double acc[SDF_NSUM];
#pragma unroll
    for (int a = 0; a < SDF_NSUM; a++) acc[a] = 0.0;
    int n_considered = 0, n_valid = 0;
#pragma unroll 1
    for (int j = 0; j < VG_POINTS_PER_LANE; j++) {
        const int i = (blockIdx.x * VG_POINTS_PER_LANE + j) * 256 + tid;
        bool considered = false, valid = false;
        if (i < s.n) {
            const float sx = s.x[i], sy = s.y[i], sz = s.z[i];
            considered = finite3(sx, sy, sz);
            float p0, p1, p2;
            xform_point(P, sx, sy, sz, p0, p1, p2);
            if (considered && finite3(p0, p1, p2)) {
                const int cell = vg_cell_index(g.lo, g.dims, vg_cell_coord(p0, g.vs), vg_cell_coord(p1, g.vs), vg_cell_coord(p2, g.vs));
                if (cell >= 0) {
                    const float2* __restrict__ rec = cells + (size_t)cell * 5;
                    const float2 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
                    const int n = __float_as_int(r4.y);
                    float b0, b1, b2;
                    xform_normal(nm, s.nx[i], s.ny[i], s.nz[i], b0, b1, b2);
                    double b[3];
                    if (n >= g.min_points && gicp_unit(b0, b1, b2, b)) {
                        valid = true;
                        const double ome = s.one_minus_eps, N = (double)n;
                        const double S00 = 2.0 - ome * ((double)r1.y + b[0] * b[0]), S01 = -ome * ((double)r2.x + b[0] * b[1]), S02 = -ome * ((double)r2.y + b[0] * b[2]);
                        const double S11 = 2.0 - ome * ((double)r3.x + b[1] * b[1]), S12 = -ome * ((double)r3.y + b[1] * b[2]), S22 = 2.0 - ome * ((double)r4.x + b[2] * b[2]);
                        const double c00 = S11 * S22 - S12 * S12, c01 = S02 * S12 - S01 * S22, c02 = S01 * S12 - S02 * S11;
                        const double c11 = S00 * S22 - S02 * S02, c12 = S01 * S02 - S00 * S12, c22 = S00 * S11 - S01 * S01;
                        const double det = (S00 * c00 + S01 * c01) + S02 * c02;
                        const double M[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
                        const double q0 = p0, q1 = p1, q2 = p2;
                        const double A[3][3] = {{0.0, q2, -q1}, {-q2, 0.0, q0}, {q1, -q0, 0.0}};      // -[p]x
                        const double r[3] = {(double)r0.x - q0, (double)r0.y - q1, (double)r1.x - q2};
                        double MA[3][3], Mr[3];
#pragma unroll
                        for (int a = 0; a < 3; a++) {
#pragma unroll
                            for (int c = 0; c < 3; c++) MA[a][c] = (M[a][0] * A[0][c] + M[a][1] * A[1][c]) + M[a][2] * A[2][c];
                            Mr[a] = (M[a][0] * r[0] + M[a][1] * r[1]) + M[a][2] * r[2];
                        }
                        int k = 0;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
#pragma unroll
                            for (int c = a; c < 6; c++) {
                                double h;
                                if (a < 3 && c < 3) h = (A[0][a] * MA[0][c] + A[1][a] * MA[1][c]) + A[2][a] * MA[2][c];      // A^T M A
                                else if (a < 3) h = MA[c - 3][a];                                                              // A^T M
                                else h = M[a - 3][c - 3];
                                acc[k++] += N * h;
                            }
                        }
#pragma unroll
                        for (int a = 0; a < 3; a++) acc[21 + a] += N * ((A[0][a] * Mr[0] + A[1][a] * Mr[1]) + A[2][a] * Mr[2]);
#pragma unroll
                        for (int a = 0; a < 3; a++) acc[24 + a] += N * Mr[a];
                        acc[27] += N * ((r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2]);
                    }
                }
            }
        }
        const unsigned long long bu = __ballot(considered), bv = __ballot(valid);
        n_considered += __popcll(bu); n_valid += __popcll(bv);
    }
    if (lane == 0) { red[2 * wave] = n_considered; red[2 * wave + 1] = n_valid; }
    const double tot = block_reduce_wide<SDF_NSUM, 4>(acc, lds);      // (its barrier also covers red)
    const int nb = gridDim.x, blk = blockIdx.x;
    if (tid < SDF_NSUM) partials[(size_t)tid * nb + blk] = tot;
    if (tid >= 64 && tid < 66) { const int q = tid - 64; counts[(size_t)q * nb + blk] = (red[q] + red[2 + q]) + (red[4 + q] + red[6 + q]); }
}
