// Return targets with per-group discounts (sg_gae_groups_device / sg_vtrace_device; DESIGN section 27).  Two backward scans on the frame
// of sg_gae.inc -- one lane per env, one wave per workgroup, the time axis in stages of rows, three stages in registers -- with the
// discounts read from a DEVICE table float32 [G, 2] of (gamma, lambda) rows instead of two kernel arguments: env i reads row
// i / (num_envs / G), the population's block rule.  Each lane loads its two floats once, before the scan, at every launch (a graph replay
// sees what the table holds then), and forms in float64
//     gamma = (double)row[0],  gl = __dmul_rn((double)row[0], (double)row[1])
// -- the product of two float32 values is exact in float64, so the table form is bit for bit the scalar form at gamma = float64(float32 g),
// lambda = float64(float32 l).  THE TABLE'S VALUES ARE NOT CHECKED: a NaN or a value outside [0, 1] affects the envs of its group only
// (a lane reads no other row and nothing crosses lanes).
//
//   discounted_gae_kernel<HAS_V, HAS_TV>   gae_scan_kernel's recurrence: gae_load_raw / gae_load_terminal / gae_compute of sg_gae.inc as
//                                          they stand (they take gamma and gl as per-lane doubles already)
//   vtrace_kernel<HAS_TV, TABLE>           V-trace (Espeholt et al. 2018, equation 1, c_t = lambda min(c_bar, ratio)): one more float per
//                                          element in a stage, the caller's importance ratio, in stages of kVtraceRows rows loaded array by
//                                          array; TABLE false: scalar gamma and gl arguments
// tests/returns_model.py states both in NumPy, bit for bit: float64, every operation rounded on its own (__dmul_rn / __dadd_rn /
// __dsub_rn: nothing contracts), no exp or other library function on the device.
//
// The list form of the terminal values is sg_gae.inc's: gae_scatter_kernel writes value[k] to the first output (advantage / vs), the scan
// reads its terminal values from that output (tv == out) and overwrites each element, in the same lane, after it has read it.

// The three-stage rotation of gae_scan_kernel as a frame: raw(s, c) loads stage c's rows, terminal(s, c) the terminal values its flags
// ask for, compute(s, c) consumes it.  While stage c is computed the raw rows of stage c + 2 and the terminal values of stage c + 1 are
// in flight.  The stage registers rotate by name: no indexed register array.
template <typename Stage, bool HAS_TV, typename Raw, typename Terminal, typename Compute>
__device__ __forceinline__ void returns_pipeline(int stages, Raw raw, Terminal terminal, Compute compute) {
    Stage s0, s1, s2;
    raw(s0, 0);
    raw(s1, 1);
    if (HAS_TV) terminal(s0, 0);
#define SG_RETURNS_STEP(cur, nxt, far, c)   \
    do {                                    \
        if (HAS_TV) terminal(nxt, (c) + 1); \
        raw(far, (c) + 2);                  \
        compute(cur, (c));                  \
    } while (0)
    for (int c = 0; c < stages; c += 3) {
        SG_RETURNS_STEP(s0, s1, s2, c);
        if (c + 1 >= stages) break;
        SG_RETURNS_STEP(s1, s2, s0, c + 1);
        if (c + 2 >= stages) break;
        SG_RETURNS_STEP(s2, s0, s1, c + 2);
    }
#undef SG_RETURNS_STEP
}

// the lane's row of the table: per_group = num_envs / G envs share a row
__device__ __forceinline__ void returns_discounts(const float *__restrict__ table, int i, int per_group, double &gamma, double &gl) {
    const float *row = table + 2 * (size_t)(i / per_group);
    const double g = (double)row[0], l = (double)row[1];
    gamma = g;
    gl = __dmul_rn(g, l);
}

// tv: NULL, the dense terminal values, or `adv` itself (list form): `adv` and `tv` may alias and carry no __restrict__
template <bool HAS_V, bool HAS_TV>
__global__ __launch_bounds__(kGaeBlock) void discounted_gae_kernel(int K, int num_envs, int per_group, const float *__restrict__ table,
                                                                 const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                                 const uint8_t *__restrict__ trunc, const float *__restrict__ value,
                                                                 const float *__restrict__ last_value, const float *tv, float *adv,
                                                                 float *__restrict__ ret) {
    const int i = (int)blockIdx.x * kGaeBlock + (int)threadIdx.x;
    if (i >= num_envs) return;
    const size_t B = (size_t)num_envs;
    const float *fallback = reward + i;
    double gamma, gl;
    returns_discounts(table, i, per_group, gamma, gl);
    double A = 0.0;
    double v_next = last_value ? (double)last_value[i] : 0.0;
    returns_pipeline<GaeStage, HAS_TV>(
        (K + kGaeRows - 1) / kGaeRows, [&](GaeStage &s, int c) { gae_load_raw<HAS_V>(s, c, K, B, i, reward, done, trunc, value); },
        [&](GaeStage &s, int c) { gae_load_terminal(s, c, K, B, i, tv, fallback); },
        [&](const GaeStage &s, int c) { gae_compute<HAS_V, HAS_TV>(s, c, K, B, i, gamma, gl, A, v_next, adv, ret); });
}

// V-trace.  A stage holds one more float per row, the importance ratio (ratio NULL: on-policy, every ratio 1), and has fewer rows: with 8
// the terminal-value kernels spilled 41 scalar registers to vector lanes; with 6 they spill 8 to 12, fewer than gae_scan_kernel's, and
// the measured time is the same (DESIGN section 27).
constexpr int kVtraceRows = 6;

struct VtraceStage {
    float r[kVtraceRows], v[kVtraceRows], rho[kVtraceRows], x[kVtraceRows];
    uint32_t d[kVtraceRows], tr[kVtraceRows];
};

// gae_load_raw / gae_load_terminal for a VtraceStage: a row before the rollout's first reads row 0 (and stores nothing).  The loads go
// ARRAY BY ARRAY, not row by row: measured at (1 000, 65 536), with 8 rows, 301 us against 433 us with the five loads of a row together
// and 348 us with only the ratios apart (DESIGN section 27).
__device__ __forceinline__ void vtrace_load_raw(VtraceStage &s, int c, int K, size_t B, int i, const float *__restrict__ reward,
                                                const uint8_t *__restrict__ done, const uint8_t *__restrict__ trunc,
                                                const float *__restrict__ value, const float *__restrict__ ratio) {
    size_t at[kVtraceRows];
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) at[j] = (size_t)max(K - 1 - (c * kVtraceRows + j), 0) * B + (size_t)i;
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) s.d[j] = done[at[j]];
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) s.tr[j] = trunc[at[j]];
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) s.r[j] = reward[at[j]];
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) s.v[j] = value[at[j]];
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) s.rho[j] = ratio ? ratio[at[j]] : 1.0f;  // (kernel-uniform)
}

__device__ __forceinline__ void vtrace_load_terminal(VtraceStage &s, int c, int K, size_t B, int i, const float *tv, const float *fallback) {
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) {
        const int t = K - 1 - (c * kVtraceRows + j);
        const bool want = t >= 0 && s.d[j] != 0u && s.tr[j] != 0u;
        s.x[j] = *(want ? tv + ((size_t)t * B + (size_t)i) : fallback);
    }
}

// min(bar, rho) in the form that keeps a NaN ratio a NaN (and lets bar = +inf through)
__device__ __forceinline__ double vtrace_clip(double bar, double rho) { return bar < rho ? bar : rho; }

template <bool HAS_TV>
__device__ __forceinline__ void vtrace_compute(const VtraceStage &s, int c, int K, size_t B, int i, double gamma, double gl, double rho_bar,
                                               double c_bar, double pg_rho_bar, double &acc, double &v_next, float *vs, float *__restrict__ pg) {
#pragma unroll
    for (int j = 0; j < kVtraceRows; j++) {
        const int t = K - 1 - (c * kVtraceRows + j);
        const double r = (double)s.r[j], v = (double)s.v[j], rho = (double)s.rho[j];
        const double rc = vtrace_clip(rho_bar, rho), cc = vtrace_clip(c_bar, rho), rp = vtrace_clip(pg_rho_bar, rho);
        const bool dn = s.d[j] != 0u;
        const double term = (HAS_TV && s.tr[j] != 0u) ? (double)s.x[j] : 0.0;
        const double nv = dn ? term : v_next;
        const double vs_next = dn ? term : __dadd_rn(v_next, acc);  // v_s of step t + 1, before acc moves to step t
        const double delta = __dmul_rn(rc, __dsub_rn(__dadd_rn(r, __dmul_rn(gamma, nv)), v));
        const double carried = __dadd_rn(delta, __dmul_rn(__dmul_rn(gl, cc), acc));
        acc = dn ? delta : carried;  // a select, as GAE's: nothing of the later episode crosses the boundary
        v_next = v;
        if (t >= 0) {  // (wave-uniform)
            const size_t at = (size_t)t * B + (size_t)i;
            vs[at] = __double2float_rn(__dadd_rn(acc, v));
            pg[at] = __double2float_rn(__dmul_rn(rp, __dsub_rn(__dadd_rn(r, __dmul_rn(gamma, vs_next)), v)));
        }
    }
}

// tv: NULL, the dense terminal values, or `vs` itself (list form): `vs` and `tv` may alias and carry no __restrict__.  TABLE: the
// discounts come from the table; otherwise from the arguments gamma and gl (= gamma * lambda, rounded once on the host)
template <bool HAS_TV, bool TABLE>
__global__ __launch_bounds__(kGaeBlock) void vtrace_kernel(int K, int num_envs, int per_group, const float *__restrict__ table, double gamma_arg,
                                                         double gl_arg, double rho_bar, double c_bar, double pg_rho_bar,
                                                         const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                         const uint8_t *__restrict__ trunc, const float *__restrict__ value,
                                                         const float *__restrict__ last_value, const float *__restrict__ ratio,
                                                         const float *tv, float *vs, float *__restrict__ pg) {
    const int i = (int)blockIdx.x * kGaeBlock + (int)threadIdx.x;
    if (i >= num_envs) return;
    const size_t B = (size_t)num_envs;
    const float *fallback = reward + i;
    double gamma = gamma_arg, gl = gl_arg;
    if (TABLE) returns_discounts(table, i, per_group, gamma, gl);
    double acc = 0.0;
    double v_next = last_value ? (double)last_value[i] : 0.0;
    returns_pipeline<VtraceStage, HAS_TV>(
        (K + kVtraceRows - 1) / kVtraceRows, [&](VtraceStage &s, int c) { vtrace_load_raw(s, c, K, B, i, reward, done, trunc, value, ratio); },
        [&](VtraceStage &s, int c) { vtrace_load_terminal(s, c, K, B, i, tv, fallback); },
        [&](const VtraceStage &s, int c) { vtrace_compute<HAS_TV>(s, c, K, B, i, gamma, gl, rho_bar, c_bar, pg_rho_bar, acc, v_next, vs, pg); });
}
