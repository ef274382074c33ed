// Hindsight goal relabelling of a replay batch (sg_replay_relabel_device; DESIGN section 34): rows of a batch that the sampler has
// just gathered from the ring get, with probability her_ratio, the position the ship reached k* steps later in the same episode as
// their goal -- the two goal columns of obs and next_obs, and the goal-dependent part of the reward -- in place.  The ring, its
// header and the status code are sg_replay.inc's; tests/her_model.py is the same arithmetic in NumPy, bit for bit.
//
// One row per lane: the call reads and writes four of a row's D columns (0, 1, D - 2, D - 1), so moving whole rows through 16-lane
// groups, as the samplers do, would move four times the bytes to reach the same cache lines.  No LDS memory, no atomics.
//
// Philox stream tag 12, the next free one after sg_minibatch.inc's 11; written from kStreamSequence (8), as 9 .. 11 are
constexpr uint32_t kStreamHer = kStreamSequence + 4u;  // (relabel?, offset) of row j
static_assert(kStreamHer == 12u, "the header and tests/her_model.py state 12");
constexpr int kHerBatch = 8;  // done bytes of the window in flight per lane

struct HerOut {
    uint8_t *relabelled;
    int32_t *offset;
    float *goal;
};

// What the reward's goal term reads: the handle's values, and, with reward profiles on, the table and every env's index
struct HerReward {
    double goal_r2, goal_scale, sparse;
    const GoalRewardProfile *table;  // NULL: profiles are off
    const uint8_t *idx;
    float two_over_world, half_world;
};

// |v| and |v|^2 of a float64 vector, every operation rounded on its own
__device__ __forceinline__ double her_norm(double v0, double v1, double &n2) {
    n2 = __dadd_rn(__dmul_rn(v0, v0), __dmul_rn(v1, v1));
    return __dsqrt_rn(n2);
}

// goal_scale (|v0| - |v1|) + (|v1|^2 < goal_r2 ? sparse : 0): the goal term of goal_reward for the goal vectors before and after
__device__ __forceinline__ double her_term(double a0, double a1, double b0, double b1, double goal_scale, double sparse, double goal_r2) {
    double l2, c2;
    const double l = her_norm(a0, a1, l2), c = her_norm(b0, b1, c2);
    return __dadd_rn(__dmul_rn(goal_scale, __dadd_rn(l, -c)), c2 < goal_r2 ? sparse : 0.0);
}

__global__ __launch_bounds__(kReplayBlock) void her_relabel_kernel(ReplayRing r, uint32_t seed_lo, uint32_t seed_hi,
                                                                  unsigned long long thr, uint32_t H, int strategy, uint64_t n,
                                                                  ReplayBatch b, HerOut out, HerReward rw, int *__restrict__ status) {
    const ReplayHdr *h = r.hdr;
    const uint64_t j = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const bool hdr_ok = replay_hdr_ok(h, r);
    const uint32_t T = r.T, B = r.B, D = r.D;
    const uint32_t head = hdr_ok ? h->head % T : 0u, filled = hdr_ok ? h->filled : 0u;
    const uint32_t v = min(filled, T - 1u);
    const uint64_t cells = (uint64_t)v * B;  // < 2^31 (refused on the host otherwise)
    if (cells == 0ull) {  // (grid-uniform: a foreign or empty ring)
        if (j == 0) *status = kStatusReplay;
        return;
    }
    const bool live = j < n;
    const int64_t u = live ? b.index[j] : 0;
    const uint32_t st = live ? b.steps[j] : 0u;
    const bool in_range = u >= 0 && (uint64_t)u < cells;
    if (live && !in_range) *status = kStatusReplay;
    const bool valid = live && in_range;
    // ---- the draw (the call number is the header's as it stands: this call does not advance it)
    uint32_t w[4];
    philox4x32_10(seed_lo, seed_hi, (uint32_t)j, (uint32_t)(j >> 32), h->sample_calls, kStreamHer, w);
    const bool act = valid && st == 1u && (unsigned long long)w[2] < thr;
    if (valid && out.relabelled) out.relabelled[j] = st != 1u ? (uint8_t)2 : (uint8_t)act;
    const uint32_t uu = valid ? (uint32_t)u : 0u;
    const uint32_t q = uu / B, i = uu - q * B;
    const uint32_t first = (head + T - v) % T;  // oldest valid slot
    uint32_t p0 = first + q;
    p0 = p0 >= T ? p0 - T : p0;
    const uint32_t at0 = p0 * B + i;
    // ---- the window: m = min(H - 1, v - 1 - q, the first k with done[p_k, i]).  The addresses follow from q alone: kHerBatch loads
    // are issued together, and no more once every lane of the wave has met a done or its edge.  (Lanes past their window read the
    // draw's own slot again.)
    uint32_t m = act ? min(H - 1u, v - 1u - q) : 0u;
    for (uint32_t k0 = 0; __any(k0 < m); k0 += kHerBatch) {
        uint32_t dn[kHerBatch];
#pragma unroll
        for (int e = 0; e < kHerBatch; e++) {
            const uint32_t k = k0 + (uint32_t)e;
            uint32_t p = p0 + (k < m ? k : 0u);
            p = p >= T ? p - T : p;
            dn[e] = r.done[p * B + i];
        }
#pragma unroll
        for (int e = 0; e < kHerBatch; e++) {
            const uint32_t k = k0 + (uint32_t)e;
            m = k < m && dn[e] != 0u ? k : m;
        }
    }
    // ---- the offset and the achieved position: columns 0, 1 of s' of (p_k*, i)
    const uint32_t ks = strategy == 0 ? (uint32_t)__umul64hi((uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)m + 1ull) : m;
    uint32_t ps = p0 + ks;
    ps = ps >= T ? ps - T : ps;
    const uint32_t ats = act ? ps * B + i : at0;
    const bool fin = act && r.done[ats] != 0u;
    // term_idx is read only where done is set; the other lanes read a header word (a line every lane has touched)
    const uint32_t *sp = fin ? r.term_idx + ats : &h->magic;
    const uint32_t seq = *sp;
    const float *arow = fin ? r.term_obs + (size_t)(seq % r.C) * D : r.obs + (size_t)ats * D;
    const float a0 = arow[0], a1 = arow[1];
    if (!act) return;
    // ---- the row's own columns
    float *so = b.obs + j * D, *sn = b.next_obs + j * D;
    const float x00 = so[0], x01 = so[1], x10 = sn[0], x11 = sn[1];
    const float o0 = sn[D - 2u], o1 = sn[D - 1u];  // the goal the reward was formed under: s' carries it, s may predate a goal hit
    const float rew = b.reward[j];
    double goal_scale = rw.goal_scale, sparse = rw.sparse;
    if (rw.table) {
        const GoalRewardProfile &pr = rw.table[rw.idx[i]];
        goal_scale = pr.goal_scale; sparse = pr.sparse;
    }
    // ---- the new goal columns: goal_observe's formula, a float32 subtract and a float32 multiply
    so[D - 2u] = __fmul_rn(__fsub_rn(a0, x00), rw.two_over_world);
    so[D - 1u] = __fmul_rn(__fsub_rn(a1, x01), rw.two_over_world);
    sn[D - 2u] = __fmul_rn(__fsub_rn(a0, x10), rw.two_over_world);
    sn[D - 1u] = __fmul_rn(__fsub_rn(a1, x11), rw.two_over_world);
    // ---- the reward in delta form, float64, every operation rounded on its own
    const double hw = (double)rw.half_world;
    const double vo10 = __dmul_rn((double)o0, hw), vo11 = __dmul_rn((double)o1, hw);                  // old goal - x1
    const double vo00 = __dadd_rn(vo10, __dadd_rn((double)x10, -(double)x00));                       // old goal - x0
    const double vo01 = __dadd_rn(vo11, __dadd_rn((double)x11, -(double)x01));
    const double vn00 = __dadd_rn((double)a0, -(double)x00), vn01 = __dadd_rn((double)a1, -(double)x01);  // new goal - x0
    const double vn10 = __dadd_rn((double)a0, -(double)x10), vn11 = __dadd_rn((double)a1, -(double)x11);  // new goal - x1
    const double t_old = her_term(vo00, vo01, vo10, vo11, goal_scale, sparse, rw.goal_r2);
    const double t_new = her_term(vn00, vn01, vn10, vn11, goal_scale, sparse, rw.goal_r2);
    b.reward[j] = __double2float_rn(__dadd_rn(__dadd_rn((double)rew, -t_old), t_new));
    if (out.offset) out.offset[j] = (int32_t)ks;
    if (out.goal) {
        out.goal[2 * j] = a0;
        out.goal[2 * j + 1] = a1;
    }
}
