// Shuffled PPO minibatch indices drawn on the device (sg_minibatch_index_device; DESIGN section 30).  tests/minibatch_model.py states
// the contract in NumPy with Python integers; the kernel follows it bit for bit.  Nothing of a handle's env state is read.
//
// For member m and epoch e, pi is a keyed bijection of [0, N): an 8-round unbalanced Feistel network over bits = max(2,
// bit_length(N - 1)) bits, round function fmix32(R + k[r]) >> (32 - a), walked along its cycle until the value is back below N.  The
// eight round keys are two Philox blocks, key = seed, counter = ((e << 16) | (blk << 8) | m, step lo, step hi, 11).  No sort, no
// workspace, and an index is a pure function of (seed, step + step_dev, e, m, position).
//
// One plain kernel, grid (ceil(M cnt / block), P, epochs), block up to 1 024 lanes: (e, m) is uniform per workgroup, so the step
// word and both Philox blocks are formed once per workgroup, not per lane -- by its first wave, on the scalar unit, and handed to the
// other waves through 32 bytes of LDS (formed by every wave they were a third of the time of a launch without walks).  Lane q of a member's M cnt positions
// (cnt = n for SG_MINIBATCH_ROW, c = E / M for SG_MINIBATCH_ENV) encrypts q: a wave's lanes are on consecutive q, so its stores are
// consecutive 8-byte words and its length is the longest of 64 walks of expectation < 2.  The divisions by cnt and E are a
// multiply-high by floor(2^32 / d), which the host passes, and one correction.  No atomics.
// Philox stream tag 11, the next free one after sg_pbt.inc's 9 and 10; written from kStreamSequence (8), as those are
constexpr uint32_t kStreamMinibatch = kStreamSequence + 3u;  // the round keys of (epoch, member)
static_assert(kStreamMinibatch == 11u, "the header and tests/minibatch_model.py state 11");
constexpr int kMinibatchMaxMembers = 256;
constexpr int kMinibatchMaxEpochs = 64;
constexpr int kMinibatchRounds = 8;
constexpr int kMinibatchBlock = 1024;  // lanes of a workgroup at most: sixteen waves share one pair of Philox blocks
// A walk returns below N with probability > 1/2 at every encryption; 64 is what tests/minibatch_model.py asserts nothing reaches.
// It bounds the loop should the network ever not be a bijection; the value past it is written as it stands.
constexpr int kMinibatchWalkCap = 64;

__device__ __forceinline__ uint32_t minibatch_fmix32(uint32_t x) {  // murmur3's finaliser
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// floor(x / d) and x mod d for x < 2^31, 1 <= d < 2^31, magic = min(floor(2^32 / d), 2^32 - 1): the product's high word is the
// quotient or one below it
__device__ __forceinline__ uint32_t minibatch_divmod(uint32_t x, uint32_t d, uint32_t magic, uint32_t &rem) {
    uint32_t q = __umulhi(x, magic);
    uint32_t r = x - q * d;
    if (r >= d) {
        q += 1u;
        r -= d;
    }
    rem = r;
    return q;
}

struct MinibatchShape {  // by value, as a kernel argument: all uniform
    uint32_t N;         // the domain of pi: K E (row) or E (env)
    uint32_t cnt;       // positions of one minibatch: n (row) or c (env)
    uint32_t total;     // M cnt <= N: positions of one (epoch, member)
    uint32_t E, B;      // envs per member, num_envs
    uint32_t T;         // stores per position: 1 (row) or K (env)
    uint32_t n;         // entries of one [n] block of the output
    uint32_t members, minibatches;
    uint32_t magic_cnt, magic_E;
    int32_t unit;
};

__global__ __launch_bounds__(kMinibatchBlock) void minibatch_index_kernel(MinibatchShape sh, uint32_t seed_lo, uint32_t seed_hi, uint64_t step,
                                                                          const int64_t *__restrict__ step_dev, int64_t *__restrict__ index_out) {
    __shared__ uint32_t keys[kMinibatchRounds];
    const uint32_t m = blockIdx.y, e = blockIdx.z;
    // ---- uniform: the keys, formed by the first wave alone (every input is uniform, so on the scalar unit), and the widths
    if (threadIdx.x < 64u) {
        if (step_dev) step += (uint64_t)step_dev[0];
#pragma unroll
        for (uint32_t blk = 0; blk < 2u; blk++) {
            uint32_t o[4];
            philox4x32_10(seed_lo, seed_hi, (e << 16) | (blk << 8) | m, (uint32_t)step, (uint32_t)(step >> 32), kStreamMinibatch, o);
            if (threadIdx.x == 0u) {
#pragma unroll
                for (int i = 0; i < 4; i++) keys[4 * blk + i] = o[i];
            }
        }
    }
    __syncthreads();
    uint32_t k[kMinibatchRounds];
#pragma unroll
    for (int i = 0; i < kMinibatchRounds; i++) k[i] = keys[i];
    const uint32_t N = sh.N;
    const int bits = max(2, 32 - __clz((int)(N - 1u)));  // (N = 1: clz(0) = 32)
    const int wa = bits / 2, wb = bits - wa;
    const uint32_t mask_b = (1u << wb) - 1u;
    // ---- per lane
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= sh.total) return;
    uint32_t x = q;
    for (int walk = 0; walk < kMinibatchWalkCap; walk++) {
        uint32_t L = x >> wb, R = x & mask_b;
#pragma unroll
        for (int r = 0; r < kMinibatchRounds; r += 2) {  // the widths (a, b) alternate: (wa, wb) in the even rounds
            const uint32_t t0 = minibatch_fmix32(R + k[r]) >> (32 - wa);
            const uint32_t L1 = R, R1 = L ^ t0;
            const uint32_t t1 = minibatch_fmix32(R1 + k[r + 1]) >> (32 - wb);
            L = R1;
            R = L1 ^ t1;
        }
        x = (L << wb) | R;
        if (x < N) break;
    }
    uint32_t i, b = minibatch_divmod(q, sh.cnt, sh.magic_cnt, i);
    uint32_t first = m * sh.E + x;  // env: the column; every row is < K B < 2^31
    if (sh.unit == SG_MINIBATCH_ROW) {  // (uniform)
        uint32_t col;
        const uint32_t t = minibatch_divmod(x, sh.E, sh.magic_E, col);
        first = t * sh.B + m * sh.E + col;
    }
    // index[e, b, m, t cnt + i]: the (e, m) part of the offset is uniform and 64-bit; the lane's part is below M P n <= K B < 2^31
    int64_t *out = index_out + ((uint64_t)e * sh.minibatches * sh.members + m) * sh.n;
    uint32_t at = b * (sh.members * sh.n) + i;
    for (uint32_t t = 0; t < sh.T; t++) {  // (uniform trip count)
        out[at] = (int64_t)first;
        at += sh.cnt;
        first += sh.B;
    }
}
