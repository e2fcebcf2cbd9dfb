// dev_converge.hpp -- stopping a run on a converged pose (icp_set_convergence_options): the measure of one iteration and the streak
// logic as ONE device function, used by the reducer of the merged loop (ring_reduce_solve, dev_solve.hpp) and by k_converge_step, the
// one-wave kernel the separate form enqueues behind every iteration.
// Part of icp_device.hpp (included from there, inside namespace icpdev, in front of dev_solve.hpp).
// ------------------------------------------------------------------------------------------------
// The run's control words (zero at the start of a run).  Merged form: the spare words beside the run's fault word, which travel back with
// the records; separate form: the head of the state block k_converge_step keeps (CONV_PREV / CONV_FINAL below).
enum { CONV_STREAK = 0, CONV_STOPPED = 1, CONV_RUN = 2, CONV_ROT = 3, CONV_TRANS = 4, CONV_WORDS = 16 };
constexpr int CONV_PREV = 16;             // separate form: the pose the iteration searched at, 16 floats
constexpr int CONV_FINAL = 32;            // separate form: the PoseState after the stopping iteration, 32 words
constexpr int CONV_STATE_BYTES = 256;
// The third meaning of a pose slot's last word (PoseState::fault) in the merged loop: 0 = a pose to search at, 1 / 2 = the chain was cut
// by a fault (the host repeats the run in the separate form), SLOT_STOPPED = the run has converged -- the slot holds the final pose; the
// matcher blocks of the remaining launches leave at once and their reducers pass the slot on, exactly as for a fault.
constexpr int SLOT_STOPPED = 3;

struct ConvergeParams {
    int on;                               // 0: the option is off (callers branch on this first, uniformly)
    int eligible;                         // the host's half of the eligibility: the iteration's decimation factor against the schedule's last and the previous one
    int index;                            // the iteration
    int min_iterations, patience;
    float rotation_eps, translation_eps;
    icp_convergence_step* trace;          // [iterations] of the run
    int* words;                           // CONV_* above
};

__device__ __forceinline__ void wave_sync();      // dev_solve.hpp

// All lanes of ONE wave call it.  A = the pose after the iteration, B = the pose it searched at (16 floats each, column-major, global or
// shared), status_ok = the iteration's record says ICP_OK.  Writes the trace entry and the control words; returns, to every lane, whether
// the run stops after this iteration.  fp64 throughout, on values widened from fp32: the nine products of dR = R_A R_B^T are exact, what
// rounds is their sums, dt and the two norms (include/icp_hip.h states the operation order; tests/converge_restatement.py follows it).
// Nine lanes take one entry of dR each, then lane 0 the rotation and lane 1 the translation side by side: a wave pays per instruction.
__device__ __forceinline__ bool converge_step(const ConvergeParams& cp, const float* A, const float* B, bool status_ok, int lane) {
    __shared__ double dr[9];
    __shared__ float tmeasure;
    __shared__ int stop_s;
    if (lane < 9) {
        const int r = lane / 3, c = lane - 3 * r;
        dr[lane] = ((double)A[r] * (double)B[c] + (double)A[4 + r] * (double)B[4 + c]) + (double)A[8 + r] * (double)B[8 + c];
    }
    wave_sync();
    double v0, v1, v2;
    if (lane == 1) {                      // dt = t_A - dR t_B
        const double b0 = B[12], b1 = B[13], b2 = B[14];
        v0 = (double)A[12] - ((dr[0] * b0 + dr[1] * b1) + dr[2] * b2);
        v1 = (double)A[13] - ((dr[3] * b0 + dr[4] * b1) + dr[5] * b2);
        v2 = (double)A[14] - ((dr[6] * b0 + dr[7] * b1) + dr[8] * b2);
    } else { v0 = dr[7] - dr[5]; v1 = dr[2] - dr[6]; v2 = dr[3] - dr[1]; }      // twice the axis times sin theta
    const double nrm = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    if (lane == 1) tmeasure = (float)nrm;
    wave_sync();
    if (lane == 0) {
        const float rot = ((dr[0] + dr[4]) + dr[8]) - 1.0 <= 0.0 ? INFINITY : (float)(0.5 * nrm), tr = tmeasure;
        const int elig = cp.eligible && status_ok ? 1 : 0;
        const bool met = rot <= cp.rotation_eps && tr <= cp.translation_eps;      // (false for a NaN)
        const int streak = elig && met ? cp.words[CONV_STREAK] + 1 : 0;
        const int stop = streak >= cp.patience && cp.index + 1 >= cp.min_iterations ? 1 : 0;
        icp_convergence_step* e = cp.trace + cp.index;
        e->rotation = rot; e->translation = tr; e->eligible = elig; e->streak = streak;
        cp.words[CONV_STREAK] = streak; cp.words[CONV_ROT] = __float_as_int(rot); cp.words[CONV_TRANS] = __float_as_int(tr);
        if (stop) { cp.words[CONV_RUN] = cp.index + 1; cp.words[CONV_STOPPED] = 1; }
        stop_s = stop;
    }
    wave_sync();
    return stop_s != 0;
}

// The separate form: one wave behind every iteration of a run with the option on.  ps = the context's pose state after the iteration,
// st = the iteration's record (nullptr: the iteration had no work, nothing was launched for it).  Keeps the pose the next iteration
// searches at in its state block (the host sets it to the incoming pose), saves the final PoseState there when the run stops, and does
// nothing from then on: the iterations still enqueued behind a stop run on, and the host reads neither their records nor c->ps.
__global__ __launch_bounds__(64) void k_converge_step(const ConvergeParams cp, const PoseState* __restrict__ ps, const icp_iter_stats* __restrict__ st) {
    if (cp.words[CONV_STOPPED]) return;
    const int lane = threadIdx.x;
    float* prev = (float*)(cp.words + CONV_PREV);
    const bool ok = st && st->status == ICP_OK;
    if (converge_step(cp, ps->pose, prev, ok, lane)) { if (lane < 32) ((unsigned int*)(cp.words + CONV_FINAL))[lane] = ((const unsigned int*)ps)[lane]; }
    else if (lane < 16) prev[lane] = ps->pose[lane];
}
// In front of such a run: the control words zero, the incoming pose (already in ps) as the first iteration's search pose.
__global__ __launch_bounds__(64) void k_converge_init(const PoseState* __restrict__ ps, int* words) {
    const int t = threadIdx.x;
    words[t] = t >= CONV_PREV && t < CONV_PREV + 16 ? __float_as_int(ps->pose[t - CONV_PREV]) : 0;
}
