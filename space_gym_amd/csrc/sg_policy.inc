// Actor-critic forward, sampling and log-prob in one launch (sg_policy_act_device / sg_rollout_policy_device; DESIGN section 17):
// two small float32 MLPs (actor, optional critic) in torch.nn.Linear layout, read where the learner keeps them.
//     continuous: eps0, eps1 = box_muller(o0, o1);  action = mean + exp(log_std) * eps;  logp = sum(-eps^2 / 2 - log_std - ln(2 pi) / 2)
//     discrete:   p_j = exp(logit_j - max);  action = the first j whose running sum of p reaches u23(o0) * total;  logp = log_softmax[action]
// with o = philox4x32_10(key = seed, counter = (global env index, step lo, step hi, kStreamPolicy)).  tests/policy_model.py states
// the same in NumPy float64.
//
// One lane per env.  A layer's weights are staged once per workgroup in LDS, TRANSPOSED (wt[k][j] = W[j][k]) and zero-padded to J
// outputs, so that a lane reads the four weights of outputs j .. j + 3 for its current input k with one 16-byte broadcast read.
// The lane keeps all J outputs of the layer as accumulators in registers (J = 32 * NT for the hidden layers, NT the kernel's
// template argument; J = 8 for the heads) and walks the inputs k in ascending order: output j starts at its bias and receives
// fmaf(W[j][k], h[k], .) for k = 0, 1, ...: the order does not depend on the batch, the grid or the lane.  The lane's activations
// h live in its own LDS column (act[k][lane]: bank = lane, conflict-free); a layer reads every input before it writes its outputs
// over them, so one column serves all layers and no lane ever touches another lane's column.  Weights are the only LDS data the
// lanes share: two barriers per layer, around their staging.
constexpr uint32_t kStreamPolicy = 5u;  // Philox stream tag of the policy's noise (kStreamPriority 4)
constexpr int kPolicyMaxHidden = 128, kPolicyMaxHiddenLayers = 3, kPolicyTile = 32, kPolicyHeadPad = 8, kPolicyRowPad = 4;
constexpr int kPolicyDiscreteActions = 6, kPolicyActDim = 2;

struct PolicyNet {
    const float *w[kPolicyMaxHiddenLayers + 1];
    const float *b[kPolicyMaxHiddenLayers + 1];
};
struct PolicyDev {
    PolicyNet actor, critic;
    const float *log_std;
    int n_hidden, hidden, relu, head, obs_dim, discrete;
};
// The rows a launch evaluates: n of them, or (count given) the records a terminal list holds, min(*count, capacity)
struct PolicyRows {
    const uint32_t *count;
    uint32_t capacity;
    int n;
};

constexpr int policy_block(int nt) { return nt <= 2 ? 256 : 128; }  // lanes per workgroup: see policy_lds_bytes
// LDS of one workgroup: the widest staged layer (rows of J + pad floats), its bias, and one activation column per lane
static inline size_t policy_lds_bytes(int nt, int hidden, int obs_dim) {
    const int J = kPolicyTile * nt, in_max = std::max(hidden, obs_dim), rows = std::max(J, obs_dim);
    return sizeof(float) * ((size_t)in_max * (J + kPolicyRowPad) + J + (size_t)rows * policy_block(nt));
}

__device__ __forceinline__ float policy_tanh(float x) {
    // tanh |x| = (1 - e) / (1 + e), e = exp(-2 |x|) in (0, 1]: no overflow, absolute error ~1e-7 (the quotient of two values near 1)
    const float e = __expf(-2.0f * fabsf(x));
    return copysignf(__fdividef(1.0f - e, 1.0f + e), x);
}

// wt[k][j] = W[j][k] (j < out, else 0), bs[j] = b[j] (else 0).  Global reads run along k (coalesced); the row pad keeps the
// transposing stores on different banks for consecutive k.
template <int J>
__device__ __forceinline__ void policy_stage(float *__restrict__ wt, float *__restrict__ bs, const float *__restrict__ W,
                                             const float *__restrict__ b, int in, int out) {
    __syncthreads();  // every lane has finished reading the layer staged before
    const int sh = 32 - __clz(max(in - 1, 1)), n = J << sh;  // k runs over the next power of two: a shift instead of a division
    for (int idx = (int)threadIdx.x; idx < n; idx += (int)blockDim.x) {
        const int j = idx >> sh, k = idx & ((1 << sh) - 1);
        if (k < in) wt[k * (J + kPolicyRowPad) + j] = j < out ? W[(size_t)j * in + k] : 0.0f;
    }
    for (int j = (int)threadIdx.x; j < J; j += (int)blockDim.x) bs[j] = j < out ? b[j] : 0.0f;
    __syncthreads();
}

// acc[j] = b[j] + sum_k W[j][k] h[k], k ascending; h is this lane's activation column (stride: the lanes of the workgroup)
template <int J>
__device__ __forceinline__ void policy_layer(const float *__restrict__ wt, const float *__restrict__ bs, const float *__restrict__ h,
                                             int stride, int in, float (&acc)[J]) {
#pragma unroll
    for (int j = 0; j < J; j += 4) {
        const float4 b4 = *reinterpret_cast<const float4 *>(bs + j);
        acc[j] = b4.x; acc[j + 1] = b4.y; acc[j + 2] = b4.z; acc[j + 3] = b4.w;
    }
#pragma unroll 2
    for (int k = 0; k < in; k++) {
        const float hk = h[(size_t)k * stride];
        const float4 *row = reinterpret_cast<const float4 *>(wt + (size_t)k * (J + kPolicyRowPad));
#pragma unroll
        for (int j = 0; j < J; j += 4) {
            const float4 w4 = row[j >> 2];
            acc[j] = fmaf(w4.x, hk, acc[j]);
            acc[j + 1] = fmaf(w4.y, hk, acc[j + 1]);
            acc[j + 2] = fmaf(w4.z, hk, acc[j + 2]);
            acc[j + 3] = fmaf(w4.w, hk, acc[j + 3]);
        }
    }
}

// One net for this lane's observation row: head outputs 0 .. kPolicyHeadPad - 1 into `out`.  tail (the Q critics, sg_qnet.inc): the
// last kPolicyActDim of the p.obs_dim inputs are tail[0 .. 1], the row's action, and obs_row holds the others.  member (sg_population.inc):
// the net's tensors are stacked [members, ...] and this is member `member`'s slice of each, at member x numel(tensor)
template <int NT>
__device__ __forceinline__ void policy_net(const PolicyDev &p, const PolicyNet &net, int head, const float *__restrict__ obs_row,
                                           float *wt, float *bs, float *h, float (&out)[kPolicyHeadPad], const float *__restrict__ tail = nullptr,
                                           int member = 0) {
    constexpr int J = kPolicyTile * NT;
    const int stride = (int)blockDim.x;
    const size_t M = (size_t)member;
    const int from_obs = tail ? p.obs_dim - kPolicyActDim : p.obs_dim;
    for (int k = 0; k < from_obs; k++) h[(size_t)k * stride] = obs_row[k];
    if (tail) {
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) h[(size_t)(from_obs + d) * stride] = tail[d];
    }
    int in = p.obs_dim;
    for (int l = 0; l < p.n_hidden; l++) {  // (wave-uniform)
        policy_stage<J>(wt, bs, net.w[l] + M * p.hidden * in, net.b[l] + M * p.hidden, in, p.hidden);
        float acc[J];
        policy_layer<J>(wt, bs, h, stride, in, acc);
        // (the padded outputs are activation(0) = 0 and are never read: the next layer takes p.hidden inputs)
#pragma unroll
        for (int j = 0; j < J; j++) h[(size_t)j * stride] = p.relu ? (acc[j] < 0.0f ? 0.0f : acc[j]) : policy_tanh(acc[j]);  // (a NaN stays one)
        in = p.hidden;
    }
    policy_stage<kPolicyHeadPad>(wt, bs, net.w[p.n_hidden] + M * head * in, net.b[p.n_hidden] + M * head, in, head);
    policy_layer<kPolicyHeadPad>(wt, bs, h, stride, in, out);
}

// The act tail of a live row: draws (or not: flags & 4), the action and its log-prob from the actor's head outputs.  i is the env's index
// within the handle: it keys the noise (env_index_base + i) and addresses action_out / logp_out.  log_std: the row's policy's
__device__ __forceinline__ void policy_act_tail(const SgDev *__restrict__ cfg, const PolicyDev &p, const float *__restrict__ log_std,
                                                const float (&out)[kPolicyHeadPad], int i, uint32_t seed_lo, uint32_t seed_hi, uint64_t step,
                                                int flags, void *__restrict__ action_out, float *__restrict__ logp_out) {
    const bool det = (flags & 4) != 0;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    if (!det) philox4x32_10(seed_lo, seed_hi, cfg->env_index_base + (uint32_t)i, (uint32_t)step, (uint32_t)(step >> 32), kStreamPolicy, o);
    if (p.discrete) {
        float mx = out[0];
        int arg = 0;
#pragma unroll
        for (int j = 1; j < kPolicyDiscreteActions; j++)
            if (out[j] > mx) { mx = out[j]; arg = j; }  // the first maximum
        float pr[kPolicyDiscreteActions], total = 0.0f;
#pragma unroll
        for (int j = 0; j < kPolicyDiscreteActions; j++) { pr[j] = expf(out[j] - mx); total += pr[j]; }
        int a = arg;
        if (!det) {
            const float want = u23(o[0]) * total;
            float run = 0.0f;  // the same ascending sum as `total`: its last value is total >= want, so some j is found
            bool found = false;
            a = kPolicyDiscreteActions - 1;
#pragma unroll
            for (int j = 0; j < kPolicyDiscreteActions; j++) {
                run += pr[j];
                if (!found && run >= want) { a = j; found = true; }
            }
        }
        float la = out[0];
#pragma unroll
        for (int j = 1; j < kPolicyDiscreteActions; j++) la = a == j ? out[j] : la;
        static_cast<int32_t *>(action_out)[i] = a;
        if (logp_out) logp_out[i] = (la - mx) - logf(total);
    } else {
        float eps[kPolicyActDim] = {0.0f, 0.0f};
        if (!det) box_muller(o[0], o[1], eps[0], eps[1]);
        float lp = 0.0f, act[kPolicyActDim];
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) {
            const float ls = log_std[d];
            act[d] = fmaf(expf(ls), eps[d], out[d]);
            lp += (-0.5f * eps[d] * eps[d] - ls) - 0.9189385332046727f;
        }
        reinterpret_cast<float2 *>(action_out)[i] = make_float2(act[0], act[1]);
        if (logp_out) logp_out[i] = lp;
    }
}

// flags: 1 actor (action, logp), 2 critic (value), 4 deterministic
template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void policy_act_kernel(const SgDev *__restrict__ cfg, PolicyDev p, PolicyRows rows,
                                                                      const float *__restrict__ obs, uint32_t seed_lo, uint32_t seed_hi,
                                                                      uint64_t step, int flags, void *__restrict__ action_out,
                                                                      float *__restrict__ logp_out, float *__restrict__ value_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int n = rows.count ? (int)min(*rows.count, rows.capacity) : rows.n;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;  // (the whole workgroup: no barrier is left waiting)
    const int i = first + (int)threadIdx.x;
    const bool live = i < n;
    const float *obs_row = obs + (size_t)(live ? i : n - 1) * p.obs_dim;  // idle lanes of the last workgroup redo its last row
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(p.hidden, p.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    if (flags & 2) {
        policy_net<NT>(p, p.critic, 1, obs_row, wt, bs, h, out);
        if (live) value_out[i] = out[0];
    }
    if (!(flags & 1)) return;
    policy_net<NT>(p, p.actor, p.head, obs_row, wt, bs, h, out);
    if (!live) return;
    policy_act_tail(cfg, p, p.log_std, out, i, seed_lo, seed_hi, step, flags, action_out, logp_out);
}
