// The SAC actor (sg_squashed_act_device / sg_squashed_sample_device / sg_squashed_grad_device / sg_rollout_squashed_device; DESIGN
// section 20): a Gaussian with a state-dependent log_std, squashed by tanh, its log-prob with the Jacobian term, and the
// reparametrised gradients of (action, logp) by the actor's parameters.  Per row, d = 0, 1, head outputs (mean_0, mean_1, raw_0, raw_1):
//     ls_d  = min(max(raw_d, log_std_min), log_std_max)
//     u_d   = mean_d + exp(ls_d) eps_d;  e_d = exp(-2 |u_d|);  a_d = sign(u_d) (1 - e_d) / (1 + e_d)
//     ldj_d = 2 (ln 2 - |u_d| - log1p(e_d))                       = log(1 - a_d^2), finite when a_d rounds to +-1
//     logp  = sum_d(-eps_d^2 / 2 - ls_d - ln(2 pi) / 2 - ldj_d)
//     gu_d  = g_action_d 4 e_d / (1 + e_d)^2 + g_logp 2 a_d;  dz_mean_d = gu_d
//     dz_raw_d = (gu_d exp(ls_d) eps_d - g_logp) [log_std_min <= raw_d <= log_std_max]
// tests/squashed_model.py states the same in NumPy.
//
// Nothing here is a net of its own: the actor is a PolicyNet with a head of 4; the forward is policy_net, the backward policy_grad_net
// with the score above as the head's dz (no extra rows: log_std is the head's own outputs 2, 3), section 18's workspace of
// per-workgroup partial sums, grid cap and policy_grad_reduce_kernel.  The act and the sample kernel share squashed_tail, so the
// deterministic act and a sample without eps give the same bits.
constexpr uint32_t kStreamSquashed = 6u;  // Philox stream tag of the squashed actor's noise (kStreamPolicy 5)
constexpr int kSquashedHead = 2 * kPolicyActDim;

struct SquashedBounds {
    float lo, hi;
};

// What the tail and the score share of one component: ls, sigma = exp(ls), e, a and whether raw lies inside the clamp (bounds inclusive)
struct SquashedPart {
    float ls, sigma, e, a, absu;
    bool inside;
};
__device__ __forceinline__ SquashedPart squashed_part(float mean, float raw, float eps, SquashedBounds b) {
    SquashedPart s;
    s.ls = raw < b.lo ? b.lo : (raw > b.hi ? b.hi : raw);  // (a NaN stays one, as torch.clamp)
    s.inside = b.lo <= raw && raw <= b.hi;
    s.sigma = expf(s.ls);
    const float u = fmaf(s.sigma, eps, mean);
    s.absu = fabsf(u);
    s.e = __expf(-2.0f * s.absu);  // policy_tanh's path
    s.a = copysignf(__fdividef(1.0f - s.e, 1.0f + s.e), u);
    return s;
}

// (action, logp) of one row from its head outputs and its noise
__device__ __forceinline__ void squashed_tail(const float (&out)[kPolicyHeadPad], const float (&eps)[kPolicyActDim], SquashedBounds b,
                                              float (&act)[kPolicyActDim], float &logp) {
    float lp = 0.0f;
#pragma unroll
    for (int d = 0; d < kPolicyActDim; d++) {
        const SquashedPart s = squashed_part(out[d], out[kPolicyActDim + d], eps[d], b);
        const float ldj = 2.0f * ((0.6931471805599453f - s.absu) - log1pf(s.e));
        act[d] = s.a;
        lp += ((-0.5f * eps[d] * eps[d] - s.ls) - 0.9189385332046727f) - ldj;
    }
    logp = lp;
}

template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void squashed_act_kernel(const SgDev *__restrict__ cfg, PolicyDev p, SquashedBounds b, int n,
                                                                        const float *__restrict__ obs, uint32_t seed_lo, uint32_t seed_hi,
                                                                        uint64_t step, int deterministic, float *__restrict__ action_out,
                                                                        float *__restrict__ logp_out) {
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
    policy_net<NT>(p, p.actor, kSquashedHead, obs_row, wt, bs, h, out);
    if (!live) return;
    float eps[kPolicyActDim] = {0.0f, 0.0f}, act[kPolicyActDim], lp;
    if (!deterministic) {
        uint32_t o[4];
        philox4x32_10(seed_lo, seed_hi, cfg->env_index_base + (uint32_t)i, (uint32_t)step, (uint32_t)(step >> 32), kStreamSquashed, o);
        box_muller(o[0], o[1], eps[0], eps[1]);
    }
    squashed_tail(out, eps, b, act, lp);
    reinterpret_cast<float2 *>(action_out)[i] = make_float2(act[0], act[1]);
    if (logp_out) logp_out[i] = lp;
}

// the same tail with the caller's noise (eps NULL: zeros, the deterministic act bit for bit)
template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void squashed_sample_kernel(PolicyDev p, SquashedBounds b, int n, const float *__restrict__ obs,
                                                                           const float *__restrict__ eps_in, float *__restrict__ action_out,
                                                                           float *__restrict__ logp_out) {
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
    policy_net<NT>(p, p.actor, kSquashedHead, obs_row, wt, bs, h, out);
    if (!live) return;
    float eps[kPolicyActDim] = {0.0f, 0.0f}, act[kPolicyActDim], lp;
    if (eps_in) {
        const float2 e2 = reinterpret_cast<const float2 *>(eps_in)[i];
        eps[0] = e2.x; eps[1] = e2.y;
    }
    squashed_tail(out, eps, b, act, lp);
    reinterpret_cast<float2 *>(action_out)[i] = make_float2(act[0], act[1]);
    if (logp_out) logp_out[i] = lp;
}

// sum_i (g_action[i] . d a[i] + g_logp[i] d logp[i]) / d theta: policy_grad_net with the head's dz from the score above
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void squashed_grad_kernel(PolicyDev p, SquashedBounds b, int n, const float *__restrict__ obs,
                                                                              const float *__restrict__ eps_in, const float *__restrict__ g_action,
                                                                              const float *__restrict__ g_logp, PolicyGradLayout lay,
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
        float ga[kPolicyActDim] = {0.0f, 0.0f}, eps[kPolicyActDim] = {0.0f, 0.0f}, gl = 0.0f, no_dx[kPolicyActDim];
        if (live) {
            if (g_action) {
                const float2 g2 = reinterpret_cast<const float2 *>(g_action)[i];
                ga[0] = g2.x; ga[1] = g2.y;
            }
            if (g_logp) gl = g_logp[i];
            if (eps_in) {
                const float2 e2 = reinterpret_cast<const float2 *>(eps_in)[i];
                eps[0] = e2.x; eps[1] = e2.y;
            }
        }
        policy_grad_net<NT>(p, 0, kSquashedHead, 0, obs + row * p.obs_dim, nullptr,
                            [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
            if (!live) return;
#pragma unroll
            for (int d = 0; d < kPolicyActDim; d++) {
                const SquashedPart s = squashed_part(out[d], out[kPolicyActDim + d], eps[d], b);
                const float ope = 1.0f + s.e;
                const float gu = fmaf(ga[d], 4.0f * s.e / (ope * ope), gl * (2.0f * s.a));
                dz[d] = gu;
                dz[kPolicyActDim + d] = s.inside ? gu * (s.sigma * eps[d]) - gl : 0.0f;
            }
        }, lay, part, first, true, false, no_dx, wt, bs, store);
        first = false;
    }
}
