// The DQN head of the discrete ids (sg_dqn_act_device / sg_dqn_evaluate_device / sg_dqn_grad_device / sg_rollout_dqn_device; DESIGN
// section 22): one MLP Q(obs) -> 6, epsilon-greedy acting, the Q values a TD target and a TD loss need, and the gradients of a loss on
// them by the net's parameters.  Per row, Q = head outputs 0 .. 5:
//     argmax  = the first j with Q_j = max_j Q_j                   (policy_act_kernel's deterministic comparison loop)
//     act     explore = u23(o0) < eps_i;  action = explore ? umulhi(o1, 6) : argmax;  q = Q[action]
//     grad    dz_j = g_all[j] + [j = action] g_taken
// with o = philox4x32_10(key = seed, counter = (global env index, step lo, step hi, kStreamDqn)).  tests/dqn_model.py states the
// same in NumPy.
//
// Nothing here is a net of its own: the net is a PolicyNet with a head of 6, as the discrete actor's; the forward is policy_net, the
// backward policy_grad_net with the dz above (no extra rows, no tail, no dx), section 18's workspace of per-workgroup partial sums,
// grid cap and policy_grad_reduce_kernel.  The act and the evaluate kernel share dqn_argmax and dqn_select, so that for the same rows
// argmax, q_max and q_taken of the one are the other's bits.
constexpr uint32_t kStreamDqn = 7u;  // Philox stream tag of the epsilon-greedy draw (kStreamSquashed 6)
constexpr int kDqnHead = kPolicyDiscreteActions;

// the first maximum of the six Q values and its index
__device__ __forceinline__ int dqn_argmax(const float (&out)[kPolicyHeadPad], float &mx) {
    mx = out[0];
    int arg = 0;
#pragma unroll
    for (int j = 1; j < kDqnHead; j++)
        if (out[j] > mx) { mx = out[j]; arg = j; }
    return arg;
}
// Q[a], selected by comparison: an action outside 0 .. 5 indexes nothing (it reads Q_0).  The six values are named one by one: written
// as a loop over out[j], the selects of loads become one load at a selected address, and `out` goes to scratch
__device__ __forceinline__ float dqn_select(const float (&out)[kPolicyHeadPad], int a) {
    static_assert(kDqnHead == 6, "dqn_select names the six values");
    const float q0 = out[0], q1 = out[1], q2 = out[2], q3 = out[3], q4 = out[4], q5 = out[5];
    return a == 5 ? q5 : a == 4 ? q4 : a == 3 ? q3 : a == 2 ? q2 : a == 1 ? q1 : q0;
}

// epsilon_dev NULL: every env takes `epsilon`; then epsilon == 0 draws nothing
template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void dqn_act_kernel(const SgDev *__restrict__ cfg, PolicyDev p, int n, const float *__restrict__ obs,
                                                                   uint32_t seed_lo, uint32_t seed_hi, uint64_t step, float epsilon,
                                                                   const float *__restrict__ epsilon_dev, int32_t *__restrict__ action_out,
                                                                   float *__restrict__ q_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;  // (the whole workgroup: no barrier is left waiting)
    const bool live = (int64_t)first + (int)threadIdx.x < n;  // (the sum may pass 2^31 - 1 in the last workgroup)
    const int i = live ? first + (int)threadIdx.x : n - 1;  // idle lanes of the last workgroup redo its last row
    const float *obs_row = obs + (size_t)i * p.obs_dim;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(p.hidden, p.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    policy_net<NT>(p, p.actor, kDqnHead, obs_row, wt, bs, h, out);
    if (!live) return;
    float mx;
    int a = dqn_argmax(out, mx);
    if (epsilon_dev || epsilon > 0.0f) {
        const float eps_i = epsilon_dev ? epsilon_dev[i] : epsilon;
        uint32_t o[4];
        philox4x32_10(seed_lo, seed_hi, cfg->env_index_base + (uint32_t)i, (uint32_t)step, (uint32_t)(step >> 32), kStreamDqn, o);
        if (u23(o[0]) < eps_i) a = (int)__umulhi(o[1], (uint32_t)kDqnHead);  // (a NaN eps_i never explores)
    }
    action_out[i] = a;
    if (q_out) q_out[i] = dqn_select(out, a);
}

template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void dqn_evaluate_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                        const int32_t *__restrict__ action, float *__restrict__ q_all_out,
                                                                        float *__restrict__ q_taken_out, float *__restrict__ q_max_out,
                                                                        int32_t *__restrict__ argmax_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;
    const bool live = (int64_t)first + (int)threadIdx.x < n;
    const int i = live ? first + (int)threadIdx.x : n - 1;
    const float *obs_row = obs + (size_t)i * p.obs_dim;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(p.hidden, p.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    policy_net<NT>(p, p.actor, kDqnHead, obs_row, wt, bs, h, out);
    if (!live) return;
    if (q_all_out) {
        float2 *row = reinterpret_cast<float2 *>(q_all_out + (size_t)i * kDqnHead);  // (24-byte rows: 8-byte aligned)
#pragma unroll
        for (int j = 0; j < kDqnHead; j += 2) row[j >> 1] = make_float2(out[j], out[j + 1]);
    }
    if (q_taken_out) q_taken_out[i] = dqn_select(out, action[i]);
    if (q_max_out || argmax_out) {
        float mx;
        const int arg = dqn_argmax(out, mx);
        if (q_max_out) q_max_out[i] = mx;
        if (argmax_out) argmax_out[i] = arg;
    }
}

// sum_i sum_j (g_all[i][j] + [j = action[i]] g_taken[i]) d Q_j[i] / d theta: policy_grad_net with that dz at the head
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void dqn_grad_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                         const int32_t *__restrict__ action, const float *__restrict__ g_taken,
                                                                         const float *__restrict__ g_all, PolicyGradLayout lay,
                                                                         float *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, tiles = (int)(((int64_t)n + R - 1) / R);  // (n may be 2^31 - 1)
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + (size_t)blockIdx.x * lay.total;
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int64_t at = (int64_t)tile * R + (int)threadIdx.x;  // (past n in the last tile: may not fit an int)
        const bool live = at < n;
        const int i = live ? (int)at : n - 1;
        const size_t row = (size_t)i;  // idle lanes of the last tile redo its last row with zero loss gradients
        float ga[kDqnHead] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, gt = 0.0f, no_dx[kPolicyActDim];
        int a = -1;  // (no j: g_taken reaches nothing)
        if (live) {
            if (g_all) {
                const float2 *g2 = reinterpret_cast<const float2 *>(g_all + row * kDqnHead);
#pragma unroll
                for (int j = 0; j < kDqnHead; j += 2) {
                    const float2 g = g2[j >> 1];
                    ga[j] = g.x; ga[j + 1] = g.y;
                }
            }
            if (g_taken) { gt = g_taken[i]; a = action[i]; }
        }
        policy_grad_net<NT>(p, 0, kDqnHead, 0, obs + row * p.obs_dim, nullptr,
                            [&](const float (&)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
#pragma unroll
            for (int j = 0; j < kDqnHead; j++) dz[j] = ga[j] + (a == j ? gt : 0.0f);  // (selected by comparison, as dqn_select)
        }, lay, part, first, true, false, no_dx, wt, bs, store);
        first = false;
    }
}
