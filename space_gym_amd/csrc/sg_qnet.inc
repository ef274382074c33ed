// The off-policy learner's nets (sg_q_evaluate_device / sg_q_grad_device / sg_policy_action_device / sg_policy_action_grad_device;
// DESIGN section 19): one or two Q critics on the row x = [obs | action], their parameter gradients and d Q / d action, and the
// actor's reparametrised action a = mean(obs) + exp(log_std) eps with its parameter gradients, so that d Q / d a reaches the actor.
//     Q_c(x) = MLP_c(x), head width 1;  grads = sum_i g_qc[i] d Q_c[i] / d theta;  g_action[i] = sum_c g_qc[i] d Q_c[i] / d a[i]
//     a_d = mean_d + exp(log_std_d) eps_d;  d a_d / d mean_d = 1,  d a_d / d log_std_d = exp(log_std_d) eps_d
// tests/q_model.py states the same in NumPy.
//
// Nothing here is a net of its own: a critic is a PolicyNet whose input width p.obs_dim is obs_dim + 2 and whose last two inputs
// come from the action row (the `tail` of policy_net / policy_grad_net); the two critics sit in a PolicyDev's actor and critic
// slots, both with head 1.  The forward is policy_net, the backward policy_grad_net with the head's dz = g_qc[i]; at layer 0 the
// walk goes one step further for the two action columns of W0 (policy_grad_net's dx).  The workspace of per-workgroup partial sums,
// the grid cap and policy_grad_reduce_kernel are section 18's.  d Q / d a never leaves the lane: it is a function of the row, its g
// values and the parameters, whatever n is.

template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void q_evaluate_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                      const float *__restrict__ action, float *__restrict__ q1_out,
                                                                      float *__restrict__ q2_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;
    const int i = first + (int)threadIdx.x;
    const bool live = i < n;
    const size_t row = (size_t)(live ? i : n - 1);  // idle lanes of the last workgroup redo its last row
    const float *obs_row = obs + row * (p.obs_dim - kPolicyActDim), *act_row = action + row * kPolicyActDim;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(p.hidden, p.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    if (q1_out) {
        policy_net<NT>(p, p.actor, 1, obs_row, wt, bs, h, out, act_row);
        if (live) q1_out[i] = out[0];
    }
    if (q2_out) {
        policy_net<NT>(p, p.critic, 1, obs_row, wt, bs, h, out, act_row);
        if (live) q2_out[i] = out[0];
    }
}

// ws NULL: the critics are frozen (no MFMA, no partial sums); g_action_out NULL: no action gradient
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void q_grad_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                       const float *__restrict__ action, const float *__restrict__ g_q1,
                                                                       const float *__restrict__ g_q2, PolicyGradLayout lay,
                                                                       float *__restrict__ ws, float *__restrict__ g_action_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, tiles = (n + R - 1) / R;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws ? ws + (size_t)blockIdx.x * lay.total : nullptr;
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int i = tile * R + (int)threadIdx.x;
        const bool live = i < n;
        const size_t row = (size_t)(live ? i : n - 1);  // idle lanes of the last tile redo its last row with zero loss gradients
        const float *obs_row = obs + row * (p.obs_dim - kPolicyActDim), *act_row = action + row * kPolicyActDim;
        float da[kPolicyActDim] = {0.0f, 0.0f};
        for (int c = 0; c < 2; c++) {  // the first critic's contribution before the second's
            const float *g = c ? g_q2 : g_q1;
            if (!g) continue;  // (uniform)
            const float gq = live ? g[i] : 0.0f;
            float dx[kPolicyActDim] = {0.0f, 0.0f};
            policy_grad_net<NT>(p, c, 1, 0, obs_row, act_row, [&](const float (&)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
#pragma unroll
                for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
                dz[0] = gq;
            }, lay, part, first, ws != nullptr, g_action_out != nullptr, dx, wt, bs, store);
#pragma unroll
            for (int d = 0; d < kPolicyActDim; d++) da[d] += dx[d];
        }
        if (g_action_out && live) reinterpret_cast<float2 *>(g_action_out)[i] = make_float2(da[0], da[1]);
        first = false;
    }
}

// a = mean + exp(log_std) eps: policy_act_kernel's expression (eps NULL: zeros, its deterministic action bit for bit)
template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void policy_action_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                         const float *__restrict__ eps, float *__restrict__ action_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;
    const int i = first + (int)threadIdx.x;
    const bool live = i < n;
    const float *obs_row = obs + (size_t)(live ? i : n - 1) * p.obs_dim;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(p.hidden, p.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    policy_net<NT>(p, p.actor, p.head, obs_row, wt, bs, h, out);
    if (!live) return;
    float e[kPolicyActDim] = {0.0f, 0.0f}, act[kPolicyActDim];
    if (eps) {
        const float2 e2 = reinterpret_cast<const float2 *>(eps)[i];
        e[0] = e2.x; e[1] = e2.y;
    }
#pragma unroll
    for (int d = 0; d < kPolicyActDim; d++) {
        const float ls = p.log_std[d];
        act[d] = fmaf(expf(ls), e[d], out[d]);
    }
    reinterpret_cast<float2 *>(action_out)[i] = make_float2(act[0], act[1]);
}

// sum_i g_action[i] d a[i] / d theta for the actor and log_std: policy_grad_net with the score dz[d] = g_action[i][d] and the two
// log_std rows g_action[i][d] exp(log_std_d) eps[i][d]
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void policy_action_grad_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                                   const float *__restrict__ eps,
                                                                                   const float *__restrict__ g_action, PolicyGradLayout lay,
                                                                                   float *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, tiles = (n + R - 1) / R;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + (size_t)blockIdx.x * lay.total;
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int i = tile * R + (int)threadIdx.x;
        const bool live = i < n;
        const size_t row = (size_t)(live ? i : n - 1);
        float ga[kPolicyActDim] = {0.0f, 0.0f}, e[kPolicyActDim] = {0.0f, 0.0f}, no_dx[kPolicyActDim];
        if (live) {
            const float2 g2 = reinterpret_cast<const float2 *>(g_action)[i];
            ga[0] = g2.x; ga[1] = g2.y;
            if (eps) {
                const float2 e2 = reinterpret_cast<const float2 *>(eps)[i];
                e[0] = e2.x; e[1] = e2.y;
            }
        }
        policy_grad_net<NT>(p, 0, p.head, kPolicyActDim, obs + row * p.obs_dim, nullptr,
                            [&](const float (&)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
#pragma unroll
            for (int d = 0; d < kPolicyActDim; d++) {
                dz[d] = ga[d];
                dz[kPolicyActDim + d] = live && eps ? ga[d] * (expf(p.log_std[d]) * e[d]) : 0.0f;
            }
        }, lay, part, first, true, false, no_dx, wt, bs, store);
        first = false;
    }
}
