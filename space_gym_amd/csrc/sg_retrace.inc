// Retrace(lambda) / Q(lambda) targets over replayed sequences (sg_retrace_device; DESIGN section 35).  One backward scan on the frame of
// sg_returns.inc -- one lane per column, one wave per workgroup, the time axis in stages of rows, three stages in registers
// (returns_pipeline) -- over a time-major [L, n] sequence batch whose width n is the caller's, not num_envs.  Per column, in float64,
// every operation rounded on its own (__dmul_rn / __dadd_rn / __dsub_rn: nothing contracts):
//     carry = 0;  v_next = last_value[i] (0 if NULL)
//     for t = L - 1 .. 0:
//         boot = done ? (truncated && terminal values ? terminal_value[t, i] : 0) : v_next + carry
//         G = reward[t, i] + gamma * boot;   target[t, i] = (float) G
//         cc = c_bar < ratio[t, i] ? c_bar : ratio[t, i]   (ratio 1 if NULL; a NaN ratio stays NaN)
//         carry = (lambda * cc) * (G - q[t, i]);   v_next = value[t, i]
// -- Munos et al. 2016 with c_t = lambda min(c_bar, ratio_t); the caller's ratio picks Retrace, tree backup, Peng's or Watkins'
// Q(lambda) or plain importance sampling, with no mode in the kernel and no exp on the device.  tests/retrace_model.py states it in
// NumPy, bit for bit.
//
//   retrace_kernel<HAS_RATIO, HAS_TV, LOSS>   8 instantiations.  LOSS: a stage holds the online net's q_online too and the kernel writes
//                                             td_error = q_online - target and g = (w * clip(td, -delta, delta)) / (float)(L n) in
//                                             float32, sg_dqn_td_grad_device's arithmetic; no statistics, no reduction
// The discounts are the two double arguments, or -- discounts given -- the two floats of a DEVICE tensor read at every launch (a graph
// replay sees what it holds then) and widened: the recurrence multiplies gamma and lambda into different operands, so there is no
// gamma * lambda product to round and the tensor form is bit for bit the scalar form at gamma = (double)(float) g, lambda likewise.

// Rows per stage: a row is up to 6 floats and 2 flags here (V-trace: 4 and 2), three stages are live.  With 4 rows the instantiations
// take 78 .. 143 VGPRs without scratch or a spilled vector register; 6 and 8 rows need up to 256, and 3, 6 and 8 rows measured no faster
// at L = 1 000 (DESIGN section 35 has the compiler's figures and the times).
constexpr int kRetraceRows = 4;

struct RetraceStage {
    float r[kRetraceRows], q[kRetraceRows], v[kRetraceRows], rho[kRetraceRows], qo[kRetraceRows], x[kRetraceRows];
    uint32_t d[kRetraceRows], tr[kRetraceRows];
};

// row j of stage c, counted from the sequence's end; in 64 bits: L may be 2^31 - 1 and the rotation loads two stages past the last
__device__ __forceinline__ int64_t retrace_row(int L, int c, int j) { return (int64_t)L - 1 - ((int64_t)c * kRetraceRows + j); }

// A row before the sequence's first reads row 0 (and stores nothing).  The loads go ARRAY BY ARRAY, not row by row (section 27's
// measured lesson).  rho and qo stay unwritten, and unread, in the instantiations without them.
template <bool HAS_RATIO, bool LOSS>
__device__ __forceinline__ void retrace_load_raw(RetraceStage &s, int c, int L, size_t n, int i, const float *__restrict__ reward,
                                                 const uint8_t *__restrict__ done, const uint8_t *__restrict__ trunc,
                                                 const float *__restrict__ q, const float *__restrict__ value,
                                                 const float *__restrict__ ratio, const float *__restrict__ q_online) {
    size_t at[kRetraceRows];
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) at[j] = (size_t)max(retrace_row(L, c, j), (int64_t)0) * n + (size_t)i;
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) s.d[j] = done[at[j]];
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) s.tr[j] = trunc[at[j]];
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) s.r[j] = reward[at[j]];
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) s.q[j] = q[at[j]];
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) s.v[j] = value[at[j]];
    if (HAS_RATIO) {
#pragma unroll
        for (int j = 0; j < kRetraceRows; j++) s.rho[j] = ratio[at[j]];
    }
    if (LOSS) {
#pragma unroll
        for (int j = 0; j < kRetraceRows; j++) s.qo[j] = q_online[at[j]];
    }
}

// terminal_value is read ONLY where done && truncated (the sampler leaves the rest unwritten); every other lane reads its own reward[0]
__device__ __forceinline__ void retrace_load_terminal(RetraceStage &s, int c, int L, size_t n, int i, const float *__restrict__ tv,
                                                      const float *fallback) {
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) {
        const int64_t t = retrace_row(L, c, j);
        const bool want = t >= 0 && s.d[j] != 0u && s.tr[j] != 0u;
        s.x[j] = *(want ? tv + ((size_t)t * n + (size_t)i) : fallback);
    }
}

struct RetraceLoss {
    const float *weight;  // [n] or NULL
    float *td_error, *g;  // [L, n] or NULL
    float delta, count;   // huber_delta, (float)(L n)
};

template <bool HAS_RATIO, bool HAS_TV, bool LOSS>
__device__ __forceinline__ void retrace_compute(const RetraceStage &s, int c, int L, size_t n, int i, double gamma, double lambda, double c_bar,
                                                double &carry, double &v_next, float *__restrict__ target, const RetraceLoss &loss, float w) {
#pragma unroll
    for (int j = 0; j < kRetraceRows; j++) {
        const int64_t t = retrace_row(L, c, j);
        const bool dn = s.d[j] != 0u;
        const double term = (HAS_TV && s.tr[j] != 0u) ? (double)s.x[j] : 0.0;
        const double boot = dn ? term : __dadd_rn(v_next, carry);  // a select: nothing of the later episode crosses the boundary
        const double G = __dadd_rn((double)s.r[j], __dmul_rn(gamma, boot));
        const double cc = vtrace_clip(c_bar, HAS_RATIO ? (double)s.rho[j] : 1.0);
        carry = __dmul_rn(__dmul_rn(lambda, cc), __dsub_rn(G, (double)s.q[j]));
        v_next = (double)s.v[j];
        if (t >= 0) {  // (wave-uniform)
            const size_t at = (size_t)t * n + (size_t)i;
            const float y = __double2float_rn(G);
            target[at] = y;
            if (LOSS) {
                const float td = s.qo[j] - y;
                const float cl = fminf(fmaxf(td, -loss.delta), loss.delta);
                if (loss.td_error) loss.td_error[at] = td;      // (kernel-uniform)
                if (loss.g) loss.g[at] = (w * cl) / loss.count;  // the product rounded, then the quotient
            }
        }
    }
}

template <bool HAS_RATIO, bool HAS_TV, bool LOSS>
__global__ __launch_bounds__(kGaeBlock) void retrace_kernel(int L, int n_cols, const float *__restrict__ discounts, double gamma_arg,
                                                          double lambda_arg, double c_bar, const float *__restrict__ reward,
                                                          const uint8_t *__restrict__ done, const uint8_t *__restrict__ trunc,
                                                          const float *__restrict__ q, const float *__restrict__ value,
                                                          const float *__restrict__ last_value, const float *__restrict__ ratio,
                                                          const float *__restrict__ tv, float *__restrict__ target,
                                                          const float *__restrict__ q_online, RetraceLoss loss) {
    const int64_t col = (int64_t)blockIdx.x * kGaeBlock + (int64_t)threadIdx.x;  // (n_cols may be 2^31 - 1)
    if (col >= n_cols) return;
    const int i = (int)col;
    const size_t n = (size_t)n_cols;
    const float *fallback = reward + i;
    double gamma = gamma_arg, lambda = lambda_arg;
    if (discounts) {  // (kernel-uniform) read at every launch; widened, exact
        gamma = (double)discounts[0];
        lambda = (double)discounts[1];
    }
    const float w = (LOSS && loss.weight) ? loss.weight[i] : 1.0f;
    double carry = 0.0;
    double v_next = last_value ? (double)last_value[i] : 0.0;
    returns_pipeline<RetraceStage, HAS_TV>(
        (int)(((int64_t)L + kRetraceRows - 1) / kRetraceRows),
        [&](RetraceStage &s, int c) { retrace_load_raw<HAS_RATIO, LOSS>(s, c, L, n, i, reward, done, trunc, q, value, ratio, q_online); },
        [&](RetraceStage &s, int c) { retrace_load_terminal(s, c, L, n, i, tv, fallback); },
        [&](const RetraceStage &s, int c) { retrace_compute<HAS_RATIO, HAS_TV, LOSS>(s, c, L, n, i, gamma, lambda, c_bar, carry, v_next, target, loss, w); });
}
