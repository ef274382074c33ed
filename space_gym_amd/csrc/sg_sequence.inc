// Fixed-length sequences from the replay ring (sg_replay_sequence_device; DESIGN section 28): column j of the time-major outputs is
// L consecutive steps of one env, its L + 1 observation rows and, where a step is done, its terminal observation.  The ring, its
// header, the status code and the row idiom are sg_replay.inc's: a row of D floats belongs to a group of 16 lanes, one dword per
// lane, a wave instruction moves four rows, and the per-row scalars are computed one row per lane and handed to the groups with wave
// shuffles -- no LDS memory.  tests/sequence_model.py is the same arithmetic in NumPy, bit for bit.
//
// One lane per observation row: row = kk n + j, kk = 0 .. L, is also the row's place in obs [L + 1, n, D], so a wave's 64 rows are one
// contiguous run of the output whatever kk they belong to.  The slot of row (kk, j) is (first + q + kk - 1) mod T; for kk >= 1 that
// is p_k of step k = kk - 1, so the same lane moves the step's scalars, and its place in the [L, n] outputs is row - n.
constexpr uint32_t kStreamSequence = 8u;  // Philox stream tag (0 .. 7: reset, goal, action, replay, priority and the net samplers)
constexpr int kSequenceExtras = 4;

struct SequenceBatch {
    float *obs;
    void *action;
    float *reward;
    uint8_t *done, *trunc;
    float *terminal_obs;
    int64_t *index;
    const float *extra_in[kSequenceExtras];
    float *extra_out[kSequenceExtras];
};

__global__ __launch_bounds__(kReplayBlock) void sequence_sample_kernel(ReplayRing r, uint32_t seed_lo, uint32_t seed_hi, uint32_t L,
                                                                      int discrete, int n_extra, uint32_t n,
                                                                      const int64_t *__restrict__ index_in, SequenceBatch out,
                                                                      int *__restrict__ status) {
    const ReplayHdr *h = r.hdr;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * kReplayBlock + threadIdx.x;  // (L + 1) n < 2^31 (refused on the host otherwise)
    const uint32_t wave0 = row - lane;
    const bool hdr_ok = replay_hdr_ok(h, r);
    const uint32_t T = r.T, B = r.B, D = r.D;
    const uint32_t head = hdr_ok ? h->head % T : 0u, filled = hdr_ok ? h->filled : 0u;
    const uint32_t v = min(filled, T - 1u);
    if (v < L) {  // (grid-uniform: a foreign ring, or one that holds fewer than L steps; L >= 1)
        if (row == 0u) *status = kStatusReplay;
        return;
    }
    const uint32_t starts = (v - L + 1u) * B;  // S <= v B < 2^31
    const bool live = row < (L + 1u) * n;
    const uint32_t kk = live ? row / n : 0u;
    const uint32_t j = live ? row - kk * n : 0u;
    // ---- the draw of column j (every row of the column forms it again: no lane waits for another)
    int64_t u;
    if (index_in) {
        u = index_in[j];
    } else {
        uint32_t w[4];
        philox4x32_10(seed_lo, seed_hi, j, 0u, h->sample_calls, kStreamSequence, w);
        u = (int64_t)__umul64hi((uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)starts);
    }
    const bool in_range = u >= 0 && (uint64_t)u < (uint64_t)starts;
    const bool valid = live && in_range;
    if (live && !in_range) *status = kStatusReplay;
    const uint32_t uu = valid ? (uint32_t)u : 0u;
    const uint32_t q = uu / B, i = uu - q * B;
    const uint32_t first = (head + T - v) % T;            // oldest valid slot
    uint32_t slot = first + q;  // (first + q + kk - 1) mod T, every term < T < 2^31: one conditional subtraction per sum
    slot = slot >= T ? slot - T : slot;
    slot += kk;
    slot = slot >= T ? slot - T : slot;
    slot = slot ? slot - 1u : T - 1u;
    const uint32_t at = slot * B + i;
    const bool step = valid && kk != 0u;
    // ---- the step's scalars: loads that do not depend on one another
    const uint32_t at_s = step ? at : 0u;
    const float rw = r.reward[at_s];
    const uint32_t dn = r.done[at_s], tr = r.trunc[at_s];
    int32_t a_id = 0;
    float a0 = 0.0f, a1 = 0.0f;
    if (discrete) {
        a_id = static_cast<const int32_t *>(r.action)[at_s];
    } else {
        const float *a = static_cast<const float *>(r.action) + 2 * (size_t)at_s;
        a0 = a[0]; a1 = a[1];
    }
    float ex[kSequenceExtras];
#pragma unroll
    for (int e = 0; e < kSequenceExtras; e++) ex[e] = e < n_extra ? out.extra_in[e][at_s] : 0.0f;
    // term_idx is read only where done is set; the other lanes read a header word (a line every lane has touched)
    const bool fin = step && dn != 0u && out.terminal_obs != nullptr;
    const uint32_t *sp = fin ? r.term_idx + at : &h->magic;
    const uint32_t seq = *sp;
    const uint32_t srow = valid ? at : kReplayNoRow;
    const uint32_t trow = fin ? seq % r.C : kReplayNoRow;
    // ---- obs[kk, j]
    const uint32_t sub = lane & (kReplayGroup - 1), g = lane / kReplayGroup;
    for (uint32_t l0 = 0; l0 < D; l0 += kReplayGroup) {
        const uint32_t l = l0 + sub;
        float x[64 / kReplayRowsPerWave];
#pragma unroll
        for (int it = 0; it < 64 / kReplayRowsPerWave; it++) {
            const uint32_t src = (uint32_t)__shfl((int)srow, it * kReplayRowsPerWave + (int)g);
            const bool on = src != kReplayNoRow && l < D;
            x[it] = r.obs[on ? (size_t)src * D + l : (size_t)0];
        }
#pragma unroll
        for (int it = 0; it < 64 / kReplayRowsPerWave; it++) {
            const uint32_t src = (uint32_t)__shfl((int)srow, it * kReplayRowsPerWave + (int)g);
            if (src != kReplayNoRow && l < D) out.obs[((size_t)wave0 + (size_t)(it * kReplayRowsPerWave) + g) * D + l] = x[it];
        }
    }
    // ---- the [L, n] members of step k = kk - 1, bits unchanged
    if (step) {
        const size_t o = (size_t)row - n;
        out.reward[o] = rw;
        out.done[o] = (uint8_t)dn;
        out.trunc[o] = (uint8_t)tr;
        if (discrete) {
            static_cast<int32_t *>(out.action)[o] = a_id;
        } else {
            float *a = static_cast<float *>(out.action) + 2 * o;
            a[0] = a0; a[1] = a1;
        }
#pragma unroll
        for (int e = 0; e < kSequenceExtras; e++)
            if (e < n_extra) out.extra_out[e][o] = ex[e];
    }
    if (valid && kk == 0u && out.index) out.index[j] = u;
    // ---- terminal_obs[k, j] where the step is done: few rows, so a group of four rows without one is skipped (wave-uniform)
    const unsigned long long want = __ballot(trow != kReplayNoRow);
    if (want == 0ull) return;
    for (uint32_t l0 = 0; l0 < D; l0 += kReplayGroup) {
        const uint32_t l = l0 + sub;
        for (int it = 0; it < 64 / kReplayRowsPerWave; it++) {
            if (((want >> (it * kReplayRowsPerWave)) & 0xfull) == 0ull) continue;
            const uint32_t src = (uint32_t)__shfl((int)trow, it * kReplayRowsPerWave + (int)g);
            if (src != kReplayNoRow && l < D)
                out.terminal_obs[((size_t)wave0 + (size_t)(it * kReplayRowsPerWave) + g - n) * D + l] = r.term_obs[(size_t)src * D + l];
        }
    }
}
