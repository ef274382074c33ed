// Generalized advantage estimation over a rollout (sg_gae_device / sg_gae; DESIGN section 14): the backward recurrence
//     done:      A = (r + gamma * nv) - v              nv = the terminal value where truncated and bootstrapped, else 0
//     otherwise: A = ((r + gamma * nv) - v) + gl * A   nv = value[t + 1] (t = K - 1: last_value)
//     advantage[t] = float(A), ret[t] = float(A + v)
// per env in float64, every operation rounded on its own (__dmul_rn / __dadd_rn: nothing contracts), so tests/gae_model.py gives
// the same bits.  Nothing of a handle is read: the kernels depend on their arguments only.
//
// One lane per env, one wave per workgroup, rows walked backward in t.  Every access is one element per lane (dword / byte), so the
// pointers need no more than their natural alignment (odd B, views at an odd element offset).  At 65 536 envs there is one wave
// per SIMD and nothing else hides the memory latency, so the time axis is software-pipelined in stages of kGaeRows rows, three
// stages in registers: while stage c is computed the raw rows (reward, value, done, truncated) of stage c + 2 and the terminal
// values of stage c + 1 are in flight.  The terminal value is wanted at ~1 % of the elements only; its load is issued for every
// lane, but lanes without a truncation read reward[0, i] instead (a line that stays in the vector L1), so the load costs no HBM
// traffic, needs no branch and the compiler's counted waits stay linear.  That is why it trails the raw rows by one stage: its
// address needs their flags.
//
// List form: gae_scatter_kernel first writes value[k] to advantage[t_k, i_k]; the scan then reads its terminal values from
// `advantage` itself (tv == adv) and overwrites each element, in the same lane, after it has read it -- no scratch.
constexpr int kGaeBlock = 64;
constexpr int kGaeRows = 8;
constexpr int kStatusGaeList = 7;  // status word: a value list with count > capacity, or a (step, env) outside the rollout

struct GaeStage {
    float r[kGaeRows], v[kGaeRows], x[kGaeRows];
    uint32_t d[kGaeRows], tr[kGaeRows];
};

// rows of stage c: t = K - 1 - (c * kGaeRows + j); a row before the rollout's first reads row 0 (and stores nothing)
template <bool HAS_V>
__device__ __forceinline__ void gae_load_raw(GaeStage &s, int c, int K, size_t B, int i, const float *__restrict__ reward,
                                             const uint8_t *__restrict__ done, const uint8_t *__restrict__ trunc,
                                             const float *__restrict__ value) {
#pragma unroll
    for (int j = 0; j < kGaeRows; j++) {
        const int t = max(K - 1 - (c * kGaeRows + j), 0);
        const size_t at = (size_t)t * B + (size_t)i;
        s.r[j] = reward[at];
        s.v[j] = HAS_V ? value[at] : 0.0f;
        s.d[j] = done[at];
        s.tr[j] = trunc[at];
    }
}

__device__ __forceinline__ void gae_load_terminal(GaeStage &s, int c, int K, size_t B, int i, const float *tv, const float *fallback) {
#pragma unroll
    for (int j = 0; j < kGaeRows; j++) {
        const int t = K - 1 - (c * kGaeRows + j);
        const bool want = t >= 0 && s.d[j] != 0u && s.tr[j] != 0u;
        const float *p = want ? tv + ((size_t)t * B + (size_t)i) : fallback;
        s.x[j] = *p;
    }
}

template <bool HAS_V, bool HAS_TV>
__device__ __forceinline__ void gae_compute(const GaeStage &s, int c, int K, size_t B, int i, double gamma, double gl, double &A,
                                            double &v_next, float *adv, float *__restrict__ ret) {
#pragma unroll
    for (int j = 0; j < kGaeRows; j++) {
        const int t = K - 1 - (c * kGaeRows + j);
        const double r = (double)s.r[j], v = (double)s.v[j];
        const bool dn = s.d[j] != 0u;
        const double term = (HAS_TV && s.tr[j] != 0u) ? (double)s.x[j] : 0.0;
        const double nv = dn ? term : v_next;
        const double delta = __dsub_rn(__dadd_rn(r, __dmul_rn(gamma, nv)), v);
        const double carried = __dadd_rn(delta, __dmul_rn(gl, A));
        A = dn ? delta : carried;  // a select: nothing of the later episode, NaN included, crosses the boundary
        v_next = v;
        if (t >= 0) {  // (wave-uniform)
            const size_t at = (size_t)t * B + (size_t)i;
            adv[at] = __double2float_rn(A);
            ret[at] = __double2float_rn(__dadd_rn(A, v));
        }
    }
}

// tv: NULL (no bootstrap from truncations), the dense terminal values, or `adv` itself (list form, after gae_scatter_kernel):
// `adv` and `tv` may alias and carry no __restrict__.  The other inputs must not overlap the outputs.
template <bool HAS_V, bool HAS_TV>
__global__ __launch_bounds__(kGaeBlock) void gae_scan_kernel(int K, int num_envs, double gamma, double gl,
                                                           const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                           const uint8_t *__restrict__ trunc, const float *__restrict__ value,
                                                           const float *__restrict__ last_value, const float *tv, float *adv,
                                                           float *__restrict__ ret) {
    const int i = (int)blockIdx.x * kGaeBlock + (int)threadIdx.x;
    if (i >= num_envs) return;
    const size_t B = (size_t)num_envs;
    const int stages = (K + kGaeRows - 1) / kGaeRows;
    const float *fallback = reward + i;
    double A = 0.0;
    double v_next = last_value ? (double)last_value[i] : 0.0;
    GaeStage s0, s1, s2;
    gae_load_raw<HAS_V>(s0, 0, K, B, i, reward, done, trunc, value);
    gae_load_raw<HAS_V>(s1, 1, K, B, i, reward, done, trunc, value);
    if (HAS_TV) gae_load_terminal(s0, 0, K, B, i, tv, fallback);
    // one pipeline step: `cur` is computed while the terminal values of `nxt` and the raw rows of `far` are loaded
#define SG_GAE_STEP(cur, nxt, far, c)                                                  \
    do {                                                                               \
        if (HAS_TV) gae_load_terminal(nxt, (c) + 1, K, B, i, tv, fallback);            \
        gae_load_raw<HAS_V>(far, (c) + 2, K, B, i, reward, done, trunc, value);        \
        gae_compute<HAS_V, HAS_TV>(cur, (c), K, B, i, gamma, gl, A, v_next, adv, ret); \
    } while (0)
    for (int c = 0; c < stages; c += 3) {  // the three stage registers rotate by name: no indexed register array
        SG_GAE_STEP(s0, s1, s2, c);
        if (c + 1 >= stages) break;
        SG_GAE_STEP(s1, s2, s0, c + 1);
        if (c + 2 >= stages) break;
        SG_GAE_STEP(s2, s0, s1, c + 2);
    }
#undef SG_GAE_STEP
}

// List form, first launch: value[k] -> adv[t_k, i_k] for the records the list holds.  A count past the capacity (values are
// missing) and a record outside the rollout (ignored) set the status word.
__global__ __launch_bounds__(256) void gae_scatter_kernel(int K, int num_envs, const uint32_t *__restrict__ count,
                                                          const int32_t *__restrict__ step_env, const float *__restrict__ value,
                                                          uint32_t capacity, float *__restrict__ adv, int *__restrict__ status) {
    const uint32_t have = *count;
    const uint32_t n = min(have, capacity);
    if (have > capacity && blockIdx.x == 0 && threadIdx.x == 0) *status = kStatusGaeList;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        const int t = step_env[2 * (size_t)k], i = step_env[2 * (size_t)k + 1];
        if (t < 0 || t >= K || i < 0 || i >= num_envs) {
            *status = kStatusGaeList;
            continue;
        }
        adv[(size_t)t * (size_t)num_envs + (size_t)i] = value[k];
    }
}
