// Prioritized replay sampling with an exact integer sum tree (sg_priority_*_device; DESIGN section 16).  Priorities are unsigned
// fixed-point integers q (one uint32 leaf per cell c = slot * B + env of the ring, 0 = not samplable) and every sum over them is a
// uint64: integer addition is associative, so the contents do not depend on reduction order or on the arrival order of atomics, and
// the draw is defined without the tree: the cell chosen for r in [0, total) is the smallest c with q[0] + ... + q[c] > r.
// tests/priority_model.py is that definition in NumPy.
//
// The tree has fan-out 64: level 0 the leaves, level k node j the sum of level k - 1 nodes 64 j .. 64 j + 63, up to a level of one
// node (the total).  Every level of `node` is padded with zeros to a multiple of 64 entries, so a descent loads whole runs unguarded.
// Commit and update keep the leaves and level 1 exact (commit: one wave per level-1 node, plain stores; update: integer atomics);
// the levels above are rebuilt densely in the launches that follow (one wave per node, then one workgroup for the levels of at most
// 64 nodes and the header).  Nothing written by one workgroup is read by another within a launch except through those atomics.
constexpr int kStatusPriority = 9;  // status word: a priority call refused its input on the device (the messages: status_error, sg_check_status)
constexpr uint32_t kPriorityMagic = 0x5052494fu;  // "PRIO"
constexpr uint32_t kStreamPriority = 4u;  // Philox stream tag of the prioritized draw (kStreamReplay 3)
constexpr int kPrioBlock = 256;
constexpr int kPrioFan = 64;     // children per node
constexpr int kPrioGroup = 16;   // lanes per draw: four children per lane
constexpr int kPrioMaxLevels = 8;

struct PrioHdr {  // 64 bytes, device memory
    uint32_t magic, T, B, frac_bits, head, filled, max_q, sample_calls;
    unsigned long long total, reserved[3];
};

struct PrioTree {  // sg_priority as the kernels take it
    uint32_t *leaf;
    unsigned long long *node;
    PrioHdr *hdr;
    uint32_t T, B, frac_bits, levels;  // levels: L >= 1, level L has one node
    uint32_t n[kPrioMaxLevels];        // n[0] = T B cells, n[k] = ceil(n[k - 1] / 64)
    uint32_t off[kPrioMaxLevels];      // level k >= 1 starts at node[off[k]]
};

__device__ __forceinline__ bool prio_hdr_ok(const PrioHdr *h, const PrioTree &t) {
    return h->magic == kPriorityMagic && h->T == t.T && h->B == t.B && h->frac_bits == t.frac_bits;
}

__device__ __forceinline__ unsigned long long prio_wave_sum(unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// is slot p one of the v newest slots before head?
__device__ __forceinline__ bool prio_slot_valid(uint32_t p, uint32_t head, uint32_t v, uint32_t T) {
    const uint32_t age = head + T - 1u - p;  // (head - 1 - p) mod T, head and p < T
    return (age >= T ? age - T : age) < v;
}

// All leaves and nodes 0, total 0, max_q = priority 1.0.
__global__ __launch_bounds__(kPrioBlock) void priority_begin_kernel(PrioTree t, uint32_t n_node) {
    const size_t k0 = (size_t)blockIdx.x * kPrioBlock + threadIdx.x, stride = (size_t)gridDim.x * kPrioBlock;
    for (size_t k = k0; k < t.n[0]; k += stride) t.leaf[k] = 0u;
    for (size_t k = k0; k < n_node; k += stride) t.node[k] = 0ull;
    if (k0 == 0) {
        PrioHdr *h = t.hdr;
        h->magic = kPriorityMagic; h->T = t.T; h->B = t.B; h->frac_bits = t.frac_bits;
        h->head = 0u; h->filled = 0u; h->max_q = 1u << t.frac_bits; h->sample_calls = 0u;
        h->total = 0ull; h->reserved[0] = h->reserved[1] = h->reserved[2] = 0ull;
    }
}

// Commit, first launch: one wave per level-1 node that holds a cell of the committed slots [a0, a1) or of the hole slot [h0, h1):
// the node's 64 leaves become max_q (committed), 0 (hole; it wins where K = T makes it a committed slot too) or stay, and the
// node is their sum.  The host hands over two disjoint runs of nodes (the second one is the hole's when the commit ends at the
// end of the ring), so every node has one writer.
__global__ __launch_bounds__(kPrioBlock) void priority_commit_kernel(PrioTree t, uint32_t a0, uint32_t a1, uint32_t h0, uint32_t h1,
                                                                    uint32_t lo1, uint32_t cnt1, uint32_t lo2, uint32_t cnt2) {
    if (!prio_hdr_ok(t.hdr, t)) return;  // (reported by priority_top_kernel)
    const uint32_t w = (blockIdx.x * kPrioBlock + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= cnt1 + cnt2) return;  // (wave-uniform)
    const uint32_t nd = w < cnt1 ? lo1 + w : lo2 + (w - cnt1);
    const uint32_t c = nd * kPrioFan + lane;
    const uint32_t max_q = t.hdr->max_q;
    uint32_t q = 0u;
    if (c < t.n[0]) {
        const bool hole = c >= h0 && c < h1, fresh = c >= a0 && c < a1;
        q = hole ? 0u : fresh ? max_q : t.leaf[c];
        if (hole || fresh) t.leaf[c] = q;
    }
    const unsigned long long s = prio_wave_sum((unsigned long long)q);
    if (lane == 0) t.node[t.off[1] + nd] = s;
}

// q = clamp(rint((double) p 2^frac_bits), 1, 2^32 - 1); false for a p that is NaN, negative or infinite
__device__ __forceinline__ bool prio_quantise(float p, uint32_t frac_bits, uint32_t &q) {
    if (!(p >= 0.0f) || p > 3.402823466e38f) return false;
    const double x = rint(__dmul_rn((double)p, (double)(1ull << frac_bits)));  // (a power of two: exact)
    q = x < 1.0 ? 1u : x > 4294967295.0 ? 0xffffffffu : (uint32_t)x;
    return true;
}

// Update, first and second launch.  kPhase 0: every named cell of the valid window is exchanged to 0 and its old value leaves the
// level-1 node.  kPhase 1: atomicMax of the new q; whoever raises the leaf adds the difference to the node, so the leaf ends at
// the largest q named for it and the node at the matching sum, in any order.  max_q follows with one atomic per wave.
template <int kPhase>
__global__ __launch_bounds__(kPrioBlock) void priority_update_kernel(PrioTree t, uint64_t n, const int64_t *__restrict__ cell,
                                                                    const float *__restrict__ prio, int *__restrict__ status) {
    PrioHdr *h = t.hdr;
    if (!prio_hdr_ok(h, t)) return;  // (reported by priority_top_kernel)
    const uint64_t j = (uint64_t)blockIdx.x * kPrioBlock + threadIdx.x;
    const uint32_t head = h->head % t.T, v = min(h->filled, t.T - 1u);
    bool on = false;
    uint32_t q = 0u, c = 0u;
    if (j < n) {
        const int64_t cj = cell[j];
        const bool good = prio_quantise(prio[j], t.frac_bits, q) && cj >= 0 && cj < (int64_t)t.n[0];
        if (!good && kPhase == 0) *status = kStatusPriority;
        c = good ? (uint32_t)cj : 0u;
        on = good && prio_slot_valid(c / t.B, head, v, t.T);  // a stale cell (the hole, a never-filled slot) is skipped silently
    }
    unsigned long long *nd = t.node + t.off[1] + c / kPrioFan;
    if (kPhase == 0) {
        if (on) {
            const uint32_t old = atomicExch(t.leaf + c, 0u);
            if (old) atomicAdd(nd, 0ull - (unsigned long long)old);
        }
    } else {
        if (on) {
            const uint32_t prev = atomicMax(t.leaf + c, q);
            if (q > prev) atomicAdd(nd, (unsigned long long)(q - prev));
        }
        uint32_t m = on ? q : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
        if ((threadIdx.x & 63u) == 0 && m) atomicMax(&h->max_q, m);
    }
}

// One wave per node of level k > 1: the sum of its 64 children (the child level is padded with zeros).
__global__ __launch_bounds__(kPrioBlock) void priority_level_kernel(PrioTree t, uint32_t k) {
    if (!prio_hdr_ok(t.hdr, t)) return;  // (reported by priority_top_kernel; a foreign object is not written)
    const uint32_t w = (blockIdx.x * kPrioBlock + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= t.n[k]) return;  // (wave-uniform)
    const unsigned long long s = prio_wave_sum(t.node[t.off[k - 1u] + (size_t)w * kPrioFan + lane]);
    if (lane == 0) t.node[t.off[k] + w] = s;
}

// Last launch of a commit or an update (one workgroup): level k0 (at most 64 nodes) from its children in memory, the one-node
// level above it from LDS, then the header: total, and head / filled after a commit.  k0 > levels: level 1 is the top.
__global__ __launch_bounds__(1024) void priority_top_kernel(PrioTree t, uint32_t k0, int set_head, uint32_t head, uint32_t filled,
                                                           int *__restrict__ status) {
    __shared__ unsigned long long lv[kPrioFan];
    PrioHdr *h = t.hdr;
    if (!prio_hdr_ok(h, t)) {
        if (threadIdx.x == 0) *status = kStatusPriority;
        return;
    }
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned long long total;
    if (k0 > t.levels) {
        total = t.node[t.off[1]];
    } else {
        const unsigned long long *child = t.node + t.off[k0 - 1u];
        const uint32_t np = t.n[k0];
        for (uint32_t p = w; p < np; p += 1024u / 64u) {
            const unsigned long long s = prio_wave_sum(child[(size_t)p * kPrioFan + lane]);
            if (lane == 0) { lv[p] = s; t.node[t.off[k0] + p] = s; }
        }
        __syncthreads();
        if (w != 0) return;
        total = lv[0];
        if (np > 1u) {  // (then level k0 + 1 is the top)
            total = prio_wave_sum(lane < np ? lv[lane] : 0ull);
            if (lane == 0) t.node[t.off[k0 + 1u]] = total;
        }
    }
    if (threadIdx.x != 0) return;
    h->total = total;
    if (set_head) { h->head = head; h->filled = filled; }
}

// sample_calls advances on the device, behind the draw: a replayed captured call draws afresh.
__global__ void priority_tick_kernel(PrioHdr *h) {
    if (threadIdx.x == 0 && blockIdx.x == 0) h->sample_calls += 1u;
}

struct PrioDraw {
    int64_t *index, *cell;
    float *weight;
    uint32_t *leaf;
};

// One 16-lane group per draw.  At every level the group loads the 64 children of its node as one contiguous run (four per lane),
// scans them and steps to the first child whose inclusive prefix sum exceeds r.
__global__ __launch_bounds__(kPrioBlock) void priority_draw_kernel(PrioTree t, const uint32_t *__restrict__ ring_hdr, uint32_t seed_lo,
                                                                  uint32_t seed_hi, double beta, int stratified, uint64_t n, PrioDraw out,
                                                                  int *__restrict__ status) {
    const PrioHdr *h = t.hdr;
    const uint64_t j = ((uint64_t)blockIdx.x * kPrioBlock + threadIdx.x) / kPrioGroup;
    const uint32_t lane = threadIdx.x & 63u, sub = lane & (kPrioGroup - 1), g0 = lane - sub;
    const bool hdr_ok = prio_hdr_ok(h, t);
    const unsigned long long total = hdr_ok ? h->total : 0ull;
    const uint32_t head = hdr_ok ? h->head : 0u, filled = hdr_ok ? h->filled : 0u;
    // (grid-uniform) a foreign header, nothing to draw from, more strata than units, or priorities that lag the ring
    // (ring_hdr: the words of the ring's header -- magic, T, B, D, head, filled, ...)
    if (!hdr_ok || total == 0ull || (stratified && total < n) || ring_hdr[0] != kReplayMagic || ring_hdr[1] != t.T || ring_hdr[2] != t.B ||
        ring_hdr[4] != head || ring_hdr[5] != filled) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *status = kStatusPriority;
        return;
    }
    const uint32_t T = t.T, B = t.B, v = min(filled, T - 1u);
    const uint64_t jj = j < n ? j : 0ull;  // (groups past n walk draw 0 and store nothing)
    uint32_t w[4];
    philox4x32_10(seed_lo, seed_hi, (uint32_t)jj, (uint32_t)(jj >> 32), h->sample_calls, kStreamPriority, w);
    const unsigned long long x = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
    unsigned long long r;
    if (stratified) {
        const unsigned long long each = total / n, rest = total - each * n;
        r = jj * each + min((unsigned long long)jj, rest) + __umul64hi(x, each + (jj < rest ? 1ull : 0ull));
    } else {
        r = __umul64hi(x, total);
    }
    uint32_t nd = 0u;
    bool lost = false;
    for (uint32_t k = t.levels; k >= 1u; k--) {  // the children of node nd of level k
        unsigned long long a[4];
        if (k > 1u) {
            const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(t.node + t.off[k - 1u] + (size_t)nd * kPrioFan + 4u * sub);
            const ulonglong2 lo = src[0], hi = src[1];
            a[0] = lo.x; a[1] = lo.y; a[2] = hi.x; a[3] = hi.y;
        } else {
            const uint32_t c0 = nd * kPrioFan + 4u * sub;
            if (c0 + 3u < t.n[0]) {
                const uint4 q4 = *reinterpret_cast<const uint4 *>(t.leaf + c0);
                a[0] = q4.x; a[1] = q4.y; a[2] = q4.z; a[3] = q4.w;
            } else {
#pragma unroll
                for (uint32_t m = 0; m < 4u; m++) a[m] = c0 + m < t.n[0] ? t.leaf[c0 + m] : 0u;
            }
        }
        const unsigned long long s1 = a[0] + a[1], s2 = s1 + a[2], mine = s2 + a[3];
        unsigned long long inc = mine;  // inclusive scan over the group's 16 lanes
#pragma unroll
        for (int d = 1; d < kPrioGroup; d <<= 1) {
            const unsigned long long up = __shfl_up(inc, d, kPrioGroup);
            if ((int)sub >= d) inc += up;
        }
        const unsigned long long before = inc - mine;
        const uint32_t hits = (uint32_t)(__ballot(inc > r) >> g0) & 0xffffu;
        lost = lost || hits == 0u;
        const int src_lane = hits ? __ffs((int)hits) - 1 : 0;
        const unsigned long long rr = r - before;  // (meaningful in the hit lane)
        const uint32_t m = a[0] > rr ? 0u : s1 > rr ? 1u : s2 > rr ? 2u : 3u;
        const unsigned long long r_next = rr - (m == 0u ? 0ull : m == 1u ? a[0] : m == 2u ? s1 : s2);
        const uint32_t am = (uint32_t)(m == 0u ? a[0] : m == 1u ? a[1] : m == 2u ? a[2] : a[3]);
        nd = nd * kPrioFan + 4u * (uint32_t)src_lane + (uint32_t)__shfl((int)m, src_lane, kPrioGroup);
        lost = lost || nd >= t.n[k - 1u];
        nd = min(nd, t.n[k - 1u] - 1u);  // (a broken structure still reads inside its arrays)
        r = __shfl(r_next, src_lane, kPrioGroup);
        if (k == 1u) {
            const uint32_t q = (uint32_t)__shfl((int)am, src_lane, kPrioGroup);  // the leaf drawn
            const uint32_t c = lost ? 0u : nd;
            const uint32_t p = c / B, i = c - p * B;
            const bool good = !lost && c < t.n[0] && q != 0u && prio_slot_valid(p, head, v, T);
            if (j < n && sub == 0) {
                if (!good) {
                    *status = kStatusPriority;  // (the structure is broken: a check, not a path)
                } else {
                    uint32_t first = head + T - v;  // oldest valid slot
                    first = first >= T ? first - T : first;
                    const uint32_t age = p >= first ? p - first : p + T - first;
                    out.index[j] = (int64_t)((uint64_t)age * B + i);
                    if (out.cell) out.cell[j] = (int64_t)c;
                    if (out.leaf) out.leaf[j] = q;
                    const double share = __ddiv_rn(__dmul_rn((double)((uint64_t)v * B), (double)q), (double)total);
                    out.weight[j] = __double2float_rn(pow(share, -beta));
                }
            }
        }
    }
}
