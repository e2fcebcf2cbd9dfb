// dev_body_sym_accumulate.hpp -- the body of k_sym_accumulate, shared text: included by that kernel and by its multi-start sibling (dev_multi.hpp), so that the
// existing kernel compiles to exactly the code it had (a call of a shared inline function reorders its instructions).
    __shared__ double lds[4 * 27 * 17];
    double acc[27];
#pragma unroll
    for (int a = 0; a < 27; a++) acc[a] = 0.0;
    const float* __restrict__ P = pp.ps->pose;
    const float* __restrict__ N = pp.ps->nmat;
    const float ms0 = pp.ps->mean_s[0], ms1 = pp.ps->mean_s[1], ms2 = pp.ps->mean_s[2];
    const float md0 = pp.ps->mean_d[0], md1 = pp.ps->mean_d[1], md2 = pp.ps->mean_d[2];
    for (int k = blockIdx.x * POST_THREADS + threadIdx.x; k < pp.n; k += gridDim.x * POST_THREADS) {
        const icp_match_t m = pp.matches[k];
        if (m.idx < 0) continue;
        const int i = pp.sel ? pp.sel[k] : k;
        float s0, s1, s2, ns0, ns1, ns2;
        xform_point(P, pp.sx[i], pp.sy[i], pp.sz[i], s0, s1, s2);
        const int j = m.idx;
        const float d0 = pp.tx[j], d1 = pp.ty[j], d2 = pp.tz[j];
        if (!(finite3(s0, s1, s2) && finite3(d0, d1, d2))) continue;
        xform_normal(N, pp.snx[i], pp.sny[i], pp.snz[i], ns0, ns1, ns2);
        const float n0 = pp.tnx[j] + ns0, n1 = pp.tny[j] + ns1, n2 = pp.tnz[j] + ns2;    // :809
        accumulate_rows(1, s0 - ms0, s1 - ms1, s2 - ms2, d0 - md0, d1 - md1, d2 - md2, n0, n1, n2, m.weight, acc);
    }
    const double tot = block_reduce_wide<27, 4>(acc, lds);
    if (threadIdx.x < 27) pp.partials[(size_t)(SUM_M + threadIdx.x) * gridDim.x + blockIdx.x] = tot;
