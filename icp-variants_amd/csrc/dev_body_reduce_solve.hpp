// dev_body_reduce_solve.hpp -- the body of k_reduce_solve, shared text: included by that kernel and by its multi-start sibling (dev_multi.hpp), so that the
// existing kernel compiles to exactly the code it had (a call of a shared inline function reorders its instructions).
    __shared__ double tot[NSUM];
    __shared__ double wsum[SOLVE_THREADS / WAVE];
    __shared__ int is_last;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, a = blockIdx.x;
    {
        const double* __restrict__ row = sp.partials + (size_t)a * sp.nblocks;
        // The partials come from the producer kernel's write-back: every load is a trip to memory, and what this kernel costs is the
        // number of DEPENDENT trips.  All of a thread's loads are issued before the first add (fixed assignment b = t + 256 j, added in
        // the order of j: the same sum on every run); 2 895 partials are one round, not three.
        double x = 0.0;
        for (int b0 = 0; b0 < sp.nblocks; b0 += SOLVE_INFLIGHT * SOLVE_THREADS) {
            double v[SOLVE_INFLIGHT];
#pragma unroll
            for (int j = 0; j < SOLVE_INFLIGHT; j++) { const int b = b0 + j * SOLVE_THREADS + (int)threadIdx.x; v[j] = b < sp.nblocks ? row[b] : 0.0; }
#pragma unroll
            for (int j = 0; j < SOLVE_INFLIGHT; j++) { const int b = b0 + j * SOLVE_THREADS + (int)threadIdx.x; if (b < sp.nblocks) x += v[j]; }
        }
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
        if (lane == 0) wsum[w] = x;
    }
    __syncthreads();
    if (sp.spin) {
        // Hand-over without a ticket: every total is ONE naturally aligned 8-byte write-through store and validates itself (anything
        // but the sentinel the slots hold between launches), so nothing has to be ordered against anything: block 0 -- always
        // resident, like the other 33 -- polls the 34 slots with sc1 loads, one lane per slot, takes the values, puts the sentinels
        // back and solves.  Against store -> drain -> ticket -> re-load that is two dependent trips to memory less per launch.  The
        // wait is bounded: after SPIN_LIMIT polls (seconds) the launch gives up, raises PoseState::fault and the run reports
        // ICP_ERR_HIP instead of hanging or solving with a slot that was never written.
        if (threadIdx.x == 0) {
            double x = wsum[0];
            for (int k = 1; k < SOLVE_THREADS / WAVE; k++) x += wsum[k];
            unsigned long long bits = (unsigned long long)__double_as_longlong(x);
            if (bits == TOTAL_SENTINEL) bits ^= 1ull;         // (still a NaN: the solve's result is the same)
            __hip_atomic_store((unsigned long long*)sp.totals + a, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (a != 0) return;
        if (threadIdx.x < NSUM) {
            double v = 0.0;
            if (threadIdx.x < NSUM_USED) {
                unsigned long long* slot = (unsigned long long*)sp.totals + threadIdx.x;
                unsigned long long bits = TOTAL_SENTINEL;
                for (int spin = 0; spin < SPIN_LIMIT; spin++) {
                    bits = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bits != TOTAL_SENTINEL) break;
                    __builtin_amdgcn_s_sleep(2);
                }
                if (bits == TOTAL_SENTINEL) sp.ps->fault = 1;         // never written within the bound
                v = __longlong_as_double((long long)bits);
                __hip_atomic_store(slot, TOTAL_SENTINEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
            }
            tot[threadIdx.x] = v;
        }
        __syncthreads();
        solve_tail(sp, tot);
        return;
    }
    if (threadIdx.x == 0) {
        double x = wsum[0];
        for (int k = 1; k < SOLVE_THREADS / WAVE; k++) x += wsum[k];
        // hand-over without fences (MI355X_MICROARCH.md, valid forms): write-through store of the total, drained, then the ticket; the
        // last arriver reads the totals with sc1 loads issued after its add has returned.  A release / acquire fence pair here is an L2
        // write-back plus an L1 invalidate per block, ~3 us of this kernel's ~9.
        __hip_atomic_store(sp.totals + a, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(sp.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (t == (unsigned)(NSUM_USED - 1));
    }
    __syncthreads();
    if (!is_last) return;
    if (threadIdx.x < NSUM) tot[threadIdx.x] = threadIdx.x < NSUM_USED ? __hip_atomic_load(sp.totals + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;   // rows NSUM_USED.. are padding
    __syncthreads();
    if (threadIdx.x == 0) *sp.ticket = 0u;                // ready for the next launch on this stream
    solve_tail(sp, tot);
