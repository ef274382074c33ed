// The rest of the PBT loop on the device: member fitness from rollout rows, truncation selection, explore (sg_pbt_fitness_device /
// sg_pbt_fitness_clear_device / sg_pbt_select_device / sg_pbt_explore_device; DESIGN section 29).  tests/pbt_model.py states every
// rule and every operation's order in NumPy; the kernels follow it so that tables, sources and hyperparameters come out with the
// same bits.  Nothing of a handle's env state is read.  Plain kernels: none is a template.
//
// Fitness, two launches.  pbt_fitness_scan_kernel, one workgroup per chunk of 256 consecutive envs of a member's block (member m
// owns envs [m E, (m + 1) E)): one lane per env walks the rows forward in t, one dword and one byte per lane and row, the time axis
// software-pipelined in stages of kPbtRows rows as gae_scan_kernel's; the running return is float64, each operation rounded on its
// own.  Lanes past E hold the identities; a fixed LDS tree (x[l] = x[l] (+) x[l + s], s = 128 .. 1) leaves the chunk's six values
// in the workspace.  pbt_fitness_combine_kernel, one lane per member: the chunks in ascending order, starting from chunk 0's
// values, then the window onto the member's table row.
//
// Select, one workgroup: all pairs are compared, so ranks are exact; explore, one workgroup: one lane per member, the columns in
// turn.  Every float32 operation of explore is rounded on its own.  No atomics anywhere.
// Philox stream tags 9 and 10, the next free ones.  Written from kStreamSequence (8): tests/test_sequence.py reads every literal
// `kStream... = <n>u` of the sources and pins those beside its own to 0 .. 7; tests/test_pbt.py pins these two and that all differ.
constexpr uint32_t kStreamPbtSelect = kStreamSequence + 1u;   // the winner drawn for a bottom member
constexpr uint32_t kStreamPbtExplore = kStreamSequence + 2u;  // the up / down draw of (column, member)
static_assert(kStreamPbtSelect == 9u && kStreamPbtExplore == 10u, "the header and tests/pbt_model.py state 9 and 10");
constexpr int kPbtMaxMembers = 256;
constexpr int kPbtMaxColumns = 16;
constexpr int kPbtChunk = 256;  // envs per workgroup of the scan: the unit of the summation order
constexpr int kPbtRows = 8;     // rows per pipeline stage
constexpr int kPbtBlock = 256;  // lanes of the one-workgroup kernels (>= kPbtMaxMembers)
constexpr int kPbtValues = 6;   // per chunk in the workspace: episodes, return_sum, length_sum, return_sq_sum, return_max, return_min
enum PbtFitnessCol { kPbtEpisodes = 0, kPbtReturnSum, kPbtLengthSum, kPbtReturnSqSum, kPbtReturnMax, kPbtReturnMin, kPbtFitness, kPbtReserved,
                     kPbtFitnessCols = 8 };

struct PbtColumns {  // by value, as a kernel argument
    sg_pbt_column c[kPbtMaxColumns];
};

struct PbtStage {
    float r[kPbtRows];
    uint32_t d[kPbtRows];
};

// rows of stage c: t = c * kPbtRows + j; a row past the rollout's last reads the last row (and counts for nothing)
__device__ __forceinline__ void pbt_load(PbtStage &s, int c, int K, size_t B, size_t i, const float *__restrict__ reward,
                                         const uint8_t *__restrict__ done) {
#pragma unroll
    for (int j = 0; j < kPbtRows; j++) {
        const int t = min(c * kPbtRows + j, K - 1);
        const size_t at = (size_t)t * B + i;
        s.r[j] = reward[at];
        s.d[j] = done[at];
    }
}

struct PbtWindow {  // what one env has finished inside the call, and what it carries on
    double run, cnt, s, l, q, mx, mn;
    int len;
};

__device__ __forceinline__ void pbt_walk(const PbtStage &st, int c, int K, PbtWindow &w) {
#pragma unroll
    for (int j = 0; j < kPbtRows; j++) {
        if (c * kPbtRows + j >= K) break;  // (wave-uniform)
        w.run = __dadd_rn(w.run, (double)st.r[j]);
        w.len += 1;
        if (st.d[j] != 0u) {
            w.cnt = __dadd_rn(w.cnt, 1.0);
            w.s = __dadd_rn(w.s, w.run);
            w.l = __dadd_rn(w.l, (double)w.len);
            w.q = __dadd_rn(w.q, __dmul_rn(w.run, w.run));
            w.mx = fmax(w.mx, w.run);
            w.mn = fmin(w.mn, w.run);
            w.run = 0.0;
            w.len = 0;
        }
    }
}

// grid (chunks per member, members); E = envs per member
__global__ __launch_bounds__(kPbtChunk) void pbt_fitness_scan_kernel(int K, int num_envs, int E, const float *__restrict__ reward,
                                                                     const uint8_t *__restrict__ done, double *__restrict__ env_return,
                                                                     int32_t *__restrict__ env_length, double *__restrict__ chunk_out) {
    __shared__ double part[kPbtValues][kPbtChunk];
    const int lane = (int)threadIdx.x, chunk = (int)blockIdx.x, m = (int)blockIdx.y;
    const int within = chunk * kPbtChunk + lane;
    PbtWindow w = {0.0, 0.0, 0.0, 0.0, 0.0, -INFINITY, INFINITY, 0};
    if (within < E) {
        const size_t B = (size_t)num_envs, i = (size_t)m * (size_t)E + (size_t)within;
        w.run = env_return[i];
        w.len = env_length[i];
        const int stages = (K + kPbtRows - 1) / kPbtRows;
        PbtStage s0, s1, s2;
        pbt_load(s0, 0, K, B, i, reward, done);
        pbt_load(s1, 1, K, B, i, reward, done);
        // one pipeline step: `cur` is walked while the rows of `far` are loaded
#define SG_PBT_STEP(cur, far, c)                        \
    do {                                                \
        pbt_load(far, (c) + 2, K, B, i, reward, done);  \
        pbt_walk(cur, (c), K, w);                       \
    } while (0)
        for (int c = 0; c < stages; c += 3) {  // the three stage registers rotate by name: no indexed register array
            SG_PBT_STEP(s0, s2, c);
            if (c + 1 >= stages) break;
            SG_PBT_STEP(s1, s0, c + 1);
            if (c + 2 >= stages) break;
            SG_PBT_STEP(s2, s1, c + 2);
        }
#undef SG_PBT_STEP
        env_return[i] = w.run;
        env_length[i] = w.len;
    }
    part[0][lane] = w.cnt;
    part[1][lane] = w.s;
    part[2][lane] = w.l;
    part[3][lane] = w.q;
    part[4][lane] = w.mx;
    part[5][lane] = w.mn;
    __syncthreads();
    for (int s = kPbtChunk / 2; s > 0; s >>= 1) {
        if (lane < s) {
            part[0][lane] = __dadd_rn(part[0][lane], part[0][lane + s]);
            part[1][lane] = __dadd_rn(part[1][lane], part[1][lane + s]);
            part[2][lane] = __dadd_rn(part[2][lane], part[2][lane + s]);
            part[3][lane] = __dadd_rn(part[3][lane], part[3][lane + s]);
            part[4][lane] = fmax(part[4][lane], part[4][lane + s]);
            part[5][lane] = fmin(part[5][lane], part[5][lane + s]);
        }
        __syncthreads();
    }
    if (lane < kPbtValues) chunk_out[((size_t)m * gridDim.x + (size_t)chunk) * kPbtValues + lane] = part[lane][0];
}

__global__ __launch_bounds__(kPbtBlock) void pbt_fitness_combine_kernel(int members, int chunks, const double *__restrict__ chunk_in,
                                                                        double *__restrict__ table) {
    const int m = (int)threadIdx.x;
    if (m >= members) return;
    const double *c = chunk_in + (size_t)m * (size_t)chunks * kPbtValues;
    double cnt = c[0], s = c[1], l = c[2], q = c[3], mx = c[4], mn = c[5];
    for (int k = 1; k < chunks; k++) {
        c += kPbtValues;
        cnt = __dadd_rn(cnt, c[0]);
        s = __dadd_rn(s, c[1]);
        l = __dadd_rn(l, c[2]);
        q = __dadd_rn(q, c[3]);
        mx = fmax(mx, c[4]);
        mn = fmin(mn, c[5]);
    }
    double *row = table + (size_t)m * kPbtFitnessCols;
    const double episodes = __dadd_rn(row[kPbtEpisodes], cnt), sum = __dadd_rn(row[kPbtReturnSum], s);
    row[kPbtEpisodes] = episodes;
    row[kPbtReturnSum] = sum;
    row[kPbtLengthSum] = __dadd_rn(row[kPbtLengthSum], l);
    row[kPbtReturnSqSum] = __dadd_rn(row[kPbtReturnSqSum], q);
    row[kPbtReturnMax] = fmax(row[kPbtReturnMax], mx);
    row[kPbtReturnMin] = fmin(row[kPbtReturnMin], mn);
    row[kPbtFitness] = episodes >= 1.0 ? sum / episodes : (double)NAN;
}

// src NULL: every row; else the rows of the members that were replaced (src[m] != m)
__global__ __launch_bounds__(kPbtBlock) void pbt_fitness_clear_kernel(int members, double *__restrict__ table, const int32_t *__restrict__ src) {
    const int m = (int)threadIdx.x;
    if (m >= members) return;
    if (src && src[m] == m) return;
    double *row = table + (size_t)m * kPbtFitnessCols;
    row[kPbtEpisodes] = 0.0;
    row[kPbtReturnSum] = 0.0;
    row[kPbtLengthSum] = 0.0;
    row[kPbtReturnSqSum] = 0.0;
    row[kPbtReturnMax] = -INFINITY;
    row[kPbtReturnMin] = INFINITY;
    row[kPbtFitness] = (double)NAN;
    row[kPbtReserved] = 0.0;
}

// Truncation selection.  rank(m) = #{ j taking part : f_j > f_m or (f_j == f_m and j < m) }: a permutation of 0 .. r - 1 over
// the r members taking part.  The bottom k_eff = min(k, r / 2) members each draw one of the top k_eff; everyone else keeps itself.
__global__ __launch_bounds__(kPbtBlock) void pbt_select_kernel(int members, const double *__restrict__ fitness, int64_t stride,
                                                               const uint8_t *__restrict__ ready, int k, uint32_t seed_lo, uint32_t seed_hi,
                                                               uint64_t step, const int64_t *__restrict__ step_dev,
                                                               int32_t *__restrict__ src_out, int32_t *__restrict__ rank_out,
                                                               int32_t *__restrict__ count_out) {
    __shared__ double f[kPbtBlock];
    __shared__ int part[kPbtBlock], by_rank[kPbtBlock];
    const int m = (int)threadIdx.x;
    double fm = 0.0;
    int pm = 0;
    if (m < members) {
        fm = fitness[(int64_t)m * stride];
        pm = (!ready || ready[m] != 0) && fm == fm;
    }
    f[m] = fm;
    part[m] = pm;
    __syncthreads();
    int r = 0, rank = 0;
    for (int j = 0; j < members; j++) {
        if (!part[j]) continue;  // (workgroup-uniform)
        r++;
        const double fj = f[j];
        rank += (fj > fm || (fj == fm && j < m)) ? 1 : 0;
    }
    if (pm) by_rank[rank] = m;
    __syncthreads();
    if (m >= members) return;
    const int k_eff = min(k, r / 2);
    int from = m;
    if (pm && rank >= r - k_eff) {  // (k_eff >= 1 here)
        if (step_dev) step += (uint64_t)step_dev[0];
        uint32_t o[4];
        philox4x32_10(seed_lo, seed_hi, (uint32_t)m, (uint32_t)step, (uint32_t)(step >> 32), kStreamPbtSelect, o);
        from = by_rank[__umulhi(o[0], (uint32_t)k_eff)];
    }
    src_out[m] = from;
    if (rank_out) rank_out[m] = pm ? rank : -1;
    if (count_out && m == 0) {
        count_out[0] = k_eff;  // copies: exactly the bottom k_eff members are destinations
        count_out[1] = k_eff;
    }
}

// Explore: for every member that adam_exploit_kernel's rule lets copy, every column takes the source's value, perturbed by its mode
// and clamped.  Sources are never destinations, so no element is read and written in one launch.
__global__ __launch_bounds__(kPbtBlock) void pbt_explore_kernel(int members, const int32_t *__restrict__ src, int n_columns, PbtColumns cols,
                                                                uint32_t seed_lo, uint32_t seed_hi, uint64_t step,
                                                                const int64_t *__restrict__ step_dev, int32_t *__restrict__ refused_out) {
    __shared__ int count[kPbtBlock];
    const int m = (int)threadIdx.x;
    int from = m;
    const bool copy = m < members && adam_exploit_source(src, members, m, from);
    if (refused_out) {  // (uniform) the refused copies, counted in a fixed order
        count[m] = (m < members && !copy && from != m) ? 1 : 0;
        __syncthreads();
        for (int s = kPbtBlock / 2; s > 0; s >>= 1) {
            if (m < s) count[m] += count[m + s];
            __syncthreads();
        }
        if (m == 0) refused_out[0] = count[0];
    }
    if (!copy) return;
    if (step_dev) step += (uint64_t)step_dev[0];
    for (int c = 0; c < n_columns; c++) {
        const sg_pbt_column &col = cols.c[c];
        const float v = col.data[(int64_t)from * col.stride];
        uint32_t o[4];
        philox4x32_10(seed_lo, seed_hi, ((uint32_t)c << 16) | (uint32_t)m, (uint32_t)step, (uint32_t)(step >> 32), kStreamPbtExplore, o);
        const float fac = (o[0] >> 31) ? col.up : col.down;
        float x = v;
        if (col.mode == SG_PBT_SCALE) x = __fmul_rn(v, fac);
        if (col.mode == SG_PBT_SCALE_COMPLEMENT) x = __fsub_rn(1.0f, __fmul_rn(__fsub_rn(1.0f, v), fac));
        col.data[(int64_t)m * col.stride] = fminf(fmaxf(x, col.lo), col.hi);
    }
}
