// Policy populations (sg_policy_population_* / sg_rollout_policy_population_device; DESIGN section 23): P actor-critics of one
// architecture, their parameters stacked along a leading dimension (weight [P, out, in], bias [P, out], log_std [P, 2], the layout of
// torch.func.stack_module_state), each on its own block of rows, in ONE launch.
//
// Nothing here is arithmetic of its own.  A workgroup serves one member m = blockIdx.y.  It hands m to the device functions the
// single-policy kernels run -- policy_net and policy_act_tail (sg_policy.inc), policy_score and policy_grad_net (sg_policy_grad.inc),
// policy_grad_reduce_element -- which move every PolicyNet pointer by m x numel(layer) where they read it; log_std moves by 2 m and
// the rows by m x rows-per-member here.  (The stacked PolicyDev stays the kernel's argument, read through scalar loads: a copy with
// moved pointers, indexed by the layer, would live in scratch.)  A member's block is tiled on its own, blockIdx.x over ITS rows: a
// block of 80 rows is one workgroup with 80 live lanes, whose idle lanes redo that member's last row, so no workgroup ever stages
// two members' weights.  Member m's rows are therefore the bits the single-policy kernels give with member m's parameters; the
// gradients are, too, whenever the member's rows group into workgroups as the single call's do (population_grad_kernel).
//
// Row indices are ints: the host refuses members x rows-per-member above 2^31 - 1.

// policy_act_kernel for member blockIdx.y on rows [m x rows, (m + 1) x rows) of the handle's envs; flags as policy_act_kernel's.  The
// row index i is the env's index within the handle, so the noise stays keyed by env_index_base + i
template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void population_act_kernel(const SgDev *__restrict__ cfg, PolicyDev p, int rows,
                                                                          const float *__restrict__ obs, uint32_t seed_lo, uint32_t seed_hi,
                                                                          uint64_t step, int flags, void *__restrict__ action_out,
                                                                          float *__restrict__ logp_out, float *__restrict__ value_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= rows) return;  // (the whole workgroup: no barrier is left waiting)
    const int m = (int)blockIdx.y, local = first + (int)threadIdx.x;
    const bool live = local < rows;
    const int i = m * rows + (live ? local : rows - 1);  // idle lanes of a member's last workgroup redo the member's last row
    const float *obs_row = obs + (size_t)i * p.obs_dim;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(p.hidden, p.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    if (flags & 2) {
        policy_net<NT>(p, p.critic, 1, obs_row, wt, bs, h, out, nullptr, m);
        if (live) value_out[i] = out[0];
    }
    if (!(flags & 1)) return;
    policy_net<NT>(p, p.actor, p.head, obs_row, wt, bs, h, out, nullptr, m);
    if (!live) return;
    policy_act_tail(cfg, p, p.log_std + (size_t)m * kPolicyActDim, out, i, seed_lo, seed_hi, step, flags, action_out, logp_out);
}

// policy_evaluate_kernel for member blockIdx.y on rows [m x n, (m + 1) x n) of obs [P, n, D] / action [P, n(, 2)] / outputs [P, n]
template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void population_evaluate_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                               const void *__restrict__ action, float *__restrict__ logp_out,
                                                                               float *__restrict__ entropy_out, float *__restrict__ value_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;
    const int m = (int)blockIdx.y, local = first + (int)threadIdx.x;
    const bool live = local < n;
    const int i = m * n + (live ? local : n - 1);
    const float *obs_row = obs + (size_t)i * p.obs_dim;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(p.hidden, p.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    if (value_out) {
        policy_net<NT>(p, p.critic, 1, obs_row, wt, bs, h, out, nullptr, m);
        if (live) value_out[i] = out[0];
    }
    if (!logp_out && !entropy_out) return;
    policy_net<NT>(p, p.actor, p.head, obs_row, wt, bs, h, out, nullptr, m);
    if (!live) return;
    PolicyScore s;
    policy_score(p, p.log_std + (size_t)m * kPolicyActDim, out, action, i, 0.0f, 0.0f, false, s);
    if (logp_out) logp_out[i] = s.logp;
    if (entropy_out) entropy_out[i] = s.entropy;
}

// policy_grad_kernel for member blockIdx.y: gridDim.x workgroups take the member's row tiles blockIdx.x, + gridDim.x, ... and leave
// their partial sums in ws[m][blockIdx.x][parameter].  With gridDim.x = min(ceil(n / R), 256) this is policy_grad_kernel's grouping of
// n rows, bit for bit; the host gives a member fewer workgroups when members x that would pass 256 (the same sums, grouped otherwise)
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void population_grad_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                                const void *__restrict__ action,
                                                                                const float *__restrict__ g_logp,
                                                                                const float *__restrict__ g_entropy,
                                                                                const float *__restrict__ g_value, PolicyGradLayout lay,
                                                                                float *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, tiles = (int)(((int64_t)n + R - 1) / R), m = (int)blockIdx.y;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + ((size_t)m * gridDim.x + blockIdx.x) * lay.total;
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int64_t at = (int64_t)tile * R + (int)threadIdx.x;  // (past n in the last tile: may not fit an int)
        const bool live = at < n;
        const int i = m * n + (live ? (int)at : n - 1);  // idle lanes of the member's last tile redo its last row with zero loss gradients
        const float *obs_row = obs + (size_t)i * p.obs_dim;
        const float gl = live && g_logp ? g_logp[i] : 0.0f, ge = live && g_entropy ? g_entropy[i] : 0.0f;
        float no_dx[kPolicyActDim];  // (no gradient by the input row here)
        if (g_value) {
            const float gv = live ? g_value[i] : 0.0f;
            policy_grad_net<NT>(p, 1, 1, 0, obs_row, nullptr, [&](const float (&)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
#pragma unroll
                for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
                dz[0] = gv;
            }, lay, part, first, true, false, no_dx, wt, bs, store, m);
        }
        policy_grad_net<NT>(p, 0, p.head, p.discrete ? 0 : kPolicyActDim, obs_row, nullptr,
                            [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
            PolicyScore s;
            policy_score(p, p.log_std + (size_t)m * kPolicyActDim, out, action, i, gl, ge, true, s);
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = s.dz[j];
        }, lay, part, first, true, false, no_dx, wt, bs, store, m);
        first = false;
    }
}

// Member blockIdx.y's partials ws[m][0 .. parts) added in workgroup order into slice m of the stacked gradient tensors
__global__ __launch_bounds__(256) void population_grad_reduce_kernel(const float *__restrict__ ws, int parts, int total, PolicyGradOut o) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= total) return;
    const int m = (int)blockIdx.y;
    policy_grad_reduce_element(ws + (size_t)m * parts * total, parts, total, o, e, m);
}
