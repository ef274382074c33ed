// Device-resident replay ring with uniform n-step sampling (sg_replay_begin_device / sg_replay_commit_device /
// sg_replay_sample_device; DESIGN section 15).  The ring is caller-owned device memory in the rollout's own layout; slot p holds what
// the step stored there wrote, so the transition of (p, i) is
//     s = obs[(p - 1) mod T, i]   a = action[p, i]   r = reward[p, i]   s' = done ? term_obs[term_idx[p, i] mod C] : obs[p, i]
// Nothing of a handle is read but B, D and the action type (host side) and the status word: the kernels depend on their arguments
// and the ring only.  tests/replay_model.py is the same arithmetic in NumPy, bit for bit.
//
// Rows are D floats, 4-byte aligned only (15 floats = 60 B for Goal 3P): a row belongs to a group of 16 lanes, one dword per lane, so
// one wave instruction moves four rows and the wave's stores to a [n, D] batch are one contiguous run.  Per-draw scalars (index,
// walk, flags) are computed one draw per lane and handed to the lane groups with wave shuffles -- no LDS memory.
constexpr int kStatusReplay = 8;  // status word: a replay call refused its input on the device (the messages: status_error, sg_check_status)
constexpr uint32_t kReplayMagic = 0x52504c59u;  // "RPLY"
constexpr uint32_t kStreamReplay = 3u;  // Philox stream tag of the sampler (kStreamReset 0, kStreamGoal 1, kStreamAction 2)
constexpr int kReplayBlock = 256;
constexpr int kReplayGroup = 16;                  // lanes per row
constexpr int kReplayRowsPerWave = 64 / kReplayGroup;
constexpr uint32_t kReplayNoRow = 0xffffffffu;

struct ReplayHdr {  // 32 bytes, device memory
    uint32_t magic, T, B, D, head, filled, term_head, sample_calls;
};

struct ReplayRing {  // sg_replay as the kernels take it
    float *obs;
    void *action;
    float *reward;
    uint8_t *done, *trunc;
    uint32_t *term_idx;
    float *term_obs;
    uint32_t *slot_seq;
    ReplayHdr *hdr;
    uint32_t T, B, D, C;
};

__device__ __forceinline__ bool replay_hdr_ok(const ReplayHdr *h, const ReplayRing &r) {
    return h->magic == kReplayMagic && h->T == r.T && h->B == r.B && h->D == r.D;
}

// Writes the header and, if given, the observation the first action is taken from into obs[T - 1].
__global__ __launch_bounds__(kReplayBlock) void replay_begin_kernel(ReplayRing r, const float *__restrict__ obs0) {
    const size_t n = (size_t)r.B * r.D;
    const size_t k0 = (size_t)blockIdx.x * kReplayBlock + threadIdx.x;
    if (k0 == 0) {
        ReplayHdr *h = r.hdr;
        h->magic = kReplayMagic; h->T = r.T; h->B = r.B; h->D = r.D;
        h->head = 0u; h->filled = 0u; h->term_head = 0u; h->sample_calls = 0u;
    }
    if (!obs0) return;
    float *dst = r.obs + (size_t)(r.T - 1u) * n;
    for (size_t k = k0; k < n; k += (size_t)gridDim.x * kReplayBlock) dst[k] = obs0[k];
}

// Commit, list form, first launch: record k < min(count, capacity) gets seq = term_head + k; its row goes to term_obs[seq mod C]
// and term_idx[first_slot + t_k, i_k] = seq.  One 16-lane group per record.  term_head itself is advanced by replay_finish_kernel.
__global__ __launch_bounds__(kReplayBlock) void replay_commit_list_kernel(ReplayRing r, uint32_t first_slot, uint32_t n_steps,
                                                                         const uint32_t *__restrict__ count,
                                                                         const int32_t *__restrict__ step_env,
                                                                         const float *__restrict__ lobs, uint32_t capacity,
                                                                         int *__restrict__ status) {
    if (!replay_hdr_ok(r.hdr, r)) return;  // (reported by replay_finish_kernel)
    const uint32_t th = r.hdr->term_head;
    const uint32_t n = min(*count, capacity);
    const uint32_t sub = threadIdx.x & (kReplayGroup - 1);
    const uint32_t groups = gridDim.x * (kReplayBlock / kReplayGroup);
    for (uint32_t k = (blockIdx.x * kReplayBlock + threadIdx.x) / kReplayGroup; k < n; k += groups) {
        const int t = step_env[2 * (size_t)k], i = step_env[2 * (size_t)k + 1];
        if (t < 0 || (uint32_t)t >= n_steps || i < 0 || (uint32_t)i >= r.B) {
            if (sub == 0) *status = kStatusReplay;
            continue;
        }
        const uint32_t seq = th + k;
        const float *src = lobs + (size_t)k * r.D;
        float *dst = r.term_obs + (size_t)(seq % r.C) * r.D;
        for (uint32_t l = sub; l < r.D; l += kReplayGroup) dst[l] = src[l];
        if (sub == 0) r.term_idx[(size_t)(first_slot + (uint32_t)t) * r.B + (uint32_t)i] = seq;
    }
}

// Commit, dense form, first launch (one lane): slot_seq[first_slot] = term_head before the records are placed.
__global__ void replay_dense_mark_kernel(ReplayRing r, uint32_t first_slot) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || !replay_hdr_ok(r.hdr, r)) return;
    r.slot_seq[first_slot] = r.hdr->term_head;
}

// Commit, dense form, second launch: every env with done[first_slot, i] takes the next free sequence number (a ballot per wave, one
// reservation per workgroup; a workgroup without a finished env leaves after its one load) and its row of tobs [B, D] is copied.
__global__ __launch_bounds__(kReplayBlock) void replay_commit_dense_kernel(ReplayRing r, uint32_t first_slot,
                                                                          const float *__restrict__ tobs) {
    __shared__ uint32_t wave_n[kReplayBlock / 64 + 1];
    const uint32_t i = blockIdx.x * kReplayBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const size_t row = (size_t)first_slot * r.B;
    const bool hdr_ok = replay_hdr_ok(r.hdr, r);
    const bool fin = hdr_ok && i < r.B && r.done[row + min(i, r.B - 1u)] != 0;
    const unsigned long long m = __ballot(fin);
    if (lane == 0) wave_n[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int k = 0; k < kReplayBlock / 64; k++) tot += wave_n[k];
        wave_n[kReplayBlock / 64] = tot ? atomicAdd(&r.hdr->term_head, tot) : 0u;
    }
    __syncthreads();
    if (m == 0ull) return;  // (wave-uniform)
    uint32_t base = wave_n[kReplayBlock / 64];
    for (uint32_t k = 0; k < w; k++) base += wave_n[k];
    const uint32_t seq = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (fin) r.term_idx[row + i] = seq;
    // the rows of the wave's finished envs, one 16-lane group per row, four rows per pass
    const uint32_t sub = lane & (kReplayGroup - 1), g = lane / kReplayGroup;
    unsigned long long left = m;
    while (left) {  // (wave-uniform)
        // the g-th set bit of `left`, if there is one
        unsigned long long mine = left;
        for (uint32_t k = 0; k < g; k++) mine &= mine - 1ull;
        const bool have = mine != 0ull;
        const int src_lane = have ? __ffsll((long long)mine) - 1 : 0;
        const uint32_t s = (uint32_t)__shfl((int)seq, src_lane);
        if (have) {
            const uint32_t env = i - lane + (uint32_t)src_lane;
            const float *src = tobs + (size_t)env * r.D;
            float *dst = r.term_obs + (size_t)(s % r.C) * r.D;
            for (uint32_t l = sub; l < r.D; l += kReplayGroup) dst[l] = src[l];
        }
#pragma unroll
        for (int k = 0; k < kReplayRowsPerWave; k++) left &= left - 1ull;
    }
}

// Last launch of a commit (one wave): slot_seq of the committed slots, term_head (list form), head, filled, and the check that no
// record a valid transition still names can have been overwritten: term_head - slot_seq[oldest valid slot] <= C.
//   list form (count != NULL):  term_head_before = hdr.term_head, advanced here by min(count, capacity)
//   dense form:                 term_head_before = slot_seq[first_slot] (replay_dense_mark_kernel); hdr.term_head is already advanced
__global__ __launch_bounds__(64) void replay_finish_kernel(ReplayRing r, uint32_t first_slot, uint32_t filled_before, uint32_t n_steps,
                                                         const uint32_t *__restrict__ count, uint32_t capacity,
                                                         int *__restrict__ status) {
    ReplayHdr *h = r.hdr;
    if (!replay_hdr_ok(h, r)) {
        if (threadIdx.x == 0) *status = kStatusReplay;
        return;
    }
    uint32_t before, after;
    bool bad = false;
    if (count) {
        const uint32_t have = *count;
        bad = have > capacity;
        before = h->term_head;
        after = before + min(have, capacity);
        for (uint32_t k = threadIdx.x; k < n_steps; k += 64u) r.slot_seq[first_slot + k] = before;
    } else {
        before = r.slot_seq[first_slot];
        after = h->term_head;
    }
    if (threadIdx.x != 0) return;
    const uint32_t head = (first_slot + n_steps) % r.T;
    const uint32_t filled = min(filled_before + n_steps, r.T);
    const uint32_t v = min(filled, r.T - 1u);
    if (v) {
        const uint32_t oldest = (head + r.T - v) % r.T;
        const bool fresh = oldest >= first_slot && oldest < first_slot + n_steps;  // written above by another lane: known here
        const uint32_t seq0 = fresh ? before : r.slot_seq[oldest];
        bad |= after - seq0 > r.C;
    }
    h->term_head = after;
    h->head = head;
    h->filled = filled;
    if (bad) *status = kStatusReplay;
}

// sample_calls advances on the device, behind the sampler: a replayed captured call draws fresh indices.
__global__ void replay_tick_kernel(ReplayHdr *h) {
    if (threadIdx.x == 0 && blockIdx.x == 0) h->sample_calls += 1u;
}

struct ReplayBatch {
    float *obs;
    void *action;
    float *reward, *next_obs;
    uint8_t *terminated, *truncated;
    float *discount;
    uint8_t *steps;
    int64_t *index;
};

// One draw per lane for the scalars, one 16-lane group per row for the two gathers.  NMAX: the compiled length of the walk
// (n_step <= NMAX); steps past n_step load the draw's own first slot again and are not included.
template <int NMAX>
__global__ __launch_bounds__(kReplayBlock) void replay_sample_kernel(ReplayRing r, uint32_t seed_lo, uint32_t seed_hi, int n_step,
                                                                    double gamma, int discrete, uint64_t n,
                                                                    const int64_t *__restrict__ index_in, ReplayBatch out,
                                                                    int *__restrict__ status) {
    const ReplayHdr *h = r.hdr;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t j = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const uint64_t wave0 = j - lane;
    const bool hdr_ok = replay_hdr_ok(h, r);
    const uint32_t T = r.T, B = r.B, D = r.D;
    const uint32_t head = hdr_ok ? h->head % T : 0u, filled = hdr_ok ? h->filled : 0u;
    const uint32_t v = min(filled, T - 1u);
    const uint64_t cells = (uint64_t)v * B;  // < 2^31 (refused on the host otherwise)
    if (cells == 0ull) {  // (grid-uniform: a foreign or empty ring)
        if (j == 0) *status = kStatusReplay;
        return;
    }
    // ---- the draw
    int64_t u;
    if (index_in) {
        u = j < n ? index_in[j] : 0;
    } else {
        uint32_t w[4];
        philox4x32_10(seed_lo, seed_hi, (uint32_t)j, (uint32_t)(j >> 32), h->sample_calls, kStreamReplay, w);
        u = (int64_t)__umul64hi((uint64_t)w[0] | ((uint64_t)w[1] << 32), cells);
    }
    const bool in_range = u >= 0 && (uint64_t)u < cells;
    const bool valid = j < n && in_range;
    if (j < n && !in_range) *status = kStatusReplay;
    const uint32_t uu = valid ? (uint32_t)u : 0u;
    const uint32_t q = uu / B, i = uu - q * B;
    const uint32_t first = (head + T - v) % T;  // oldest valid slot
    uint32_t p0 = first + q;
    p0 = p0 >= T ? p0 - T : p0;
    const uint32_t pm = p0 ? p0 - 1u : T - 1u;
    // ---- the loads of the walk (independent of one another: every step's address is known from q)
    float rw[NMAX];
    uint32_t dn[NMAX];
    const uint32_t at0 = p0 * B + i;
#pragma unroll
    for (int k = 0; k < NMAX; k++) {
        const bool reach = k < n_step && q + (uint32_t)k < v;
        uint32_t p = p0 + (reach ? (uint32_t)k : 0u);
        p = p >= T ? p - T : p;
        const uint32_t at = p * B + i;
        rw[k] = r.reward[at];
        dn[k] = r.done[at];
    }
    // ---- s = obs[(p0 - 1) mod T, i] and the action: they do not depend on the walk
    const uint32_t srow = valid ? pm * B + i : kReplayNoRow;
    const uint32_t sub = lane & (kReplayGroup - 1), g = lane / kReplayGroup;
    for (uint32_t l0 = 0; l0 < D; l0 += kReplayGroup) {
        const uint32_t l = l0 + sub;
        float x[64 / kReplayRowsPerWave];
#pragma unroll
        for (int it = 0; it < 64 / kReplayRowsPerWave; it++) {
            const uint32_t row = (uint32_t)__shfl((int)srow, it * kReplayRowsPerWave + (int)g);
            const bool on = row != kReplayNoRow && l < D;
            x[it] = r.obs[on ? (size_t)row * D + l : (size_t)0];
        }
#pragma unroll
        for (int it = 0; it < 64 / kReplayRowsPerWave; it++) {
            const uint32_t row = (uint32_t)__shfl((int)srow, it * kReplayRowsPerWave + (int)g);
            if (row != kReplayNoRow && l < D) out.obs[(wave0 + (uint64_t)(it * kReplayRowsPerWave) + g) * D + l] = x[it];
        }
    }
    if (valid) {
        if (discrete) {
            static_cast<int32_t *>(out.action)[j] = static_cast<const int32_t *>(r.action)[at0];
        } else {
            const float *a = static_cast<const float *>(r.action) + 2 * (size_t)at0;
            float *o = static_cast<float *>(out.action) + 2 * j;
            o[0] = a[0]; o[1] = a[1];
        }
    }
    // ---- the walk: selects only, in float64, every operation rounded on its own
    double R = (double)rw[0], gpow = gamma;
    uint32_t last = 0u, d_last = dn[0];
    bool open = true;
#pragma unroll
    for (int k = 1; k < NMAX; k++) {
        open = open && dn[k - 1] == 0u && k < n_step && q + (uint32_t)k < v;
        const double R1 = __dadd_rn(R, __dmul_rn(gpow, (double)rw[k])), g1 = __dmul_rn(gpow, gamma);
        R = open ? R1 : R;
        gpow = open ? g1 : gpow;
        last = open ? (uint32_t)k : last;
        d_last = open ? dn[k] : d_last;
    }
    const bool fin = d_last != 0u;
    uint32_t p_last = p0 + last;
    p_last = p_last >= T ? p_last - T : p_last;
    const uint32_t at_last = p_last * B + i;
    const uint32_t tr = r.trunc[at_last];
    // term_idx is read only where done is set; the other lanes read a header word (a line every lane has touched)
    const uint32_t *sp = fin ? r.term_idx + at_last : &h->magic;
    const uint32_t seq = *sp;
    // bit 31: the row is in term_obs
    const uint32_t nrow = !valid ? kReplayNoRow : fin ? 0x80000000u | (seq % r.C) : at_last;
    if (valid) {
        out.reward[j] = __double2float_rn(R);
        out.terminated[j] = (uint8_t)(fin && tr == 0u);
        out.truncated[j] = (uint8_t)(tr != 0u);
        if (out.discount) out.discount[j] = __double2float_rn(gpow);
        if (out.steps) out.steps[j] = (uint8_t)(last + 1u);
        if (out.index) out.index[j] = u;
    }
    // ---- s' of the last step included
    for (uint32_t l0 = 0; l0 < D; l0 += kReplayGroup) {
        const uint32_t l = l0 + sub;
        float x[64 / kReplayRowsPerWave];
#pragma unroll
        for (int it = 0; it < 64 / kReplayRowsPerWave; it++) {
            const uint32_t row = (uint32_t)__shfl((int)nrow, it * kReplayRowsPerWave + (int)g);
            const bool on = row != kReplayNoRow && l < D;
            const float *base = (row & 0x80000000u) ? r.term_obs : r.obs;
            x[it] = base[on ? (size_t)(row & 0x7fffffffu) * D + l : (size_t)0];
        }
#pragma unroll
        for (int it = 0; it < 64 / kReplayRowsPerWave; it++) {
            const uint32_t row = (uint32_t)__shfl((int)nrow, it * kReplayRowsPerWave + (int)g);
            if (row != kReplayNoRow && l < D) out.next_obs[(wave0 + (uint64_t)(it * kReplayRowsPerWave) + g) * D + l] = x[it];
        }
    }
}
