// The actor update of SAC, TD3 and DDPG through the twin Q critics in one call (sg_q_actor_squashed_grad_device /
// sg_q_actor_gaussian_grad_device; DESIGN section 33): from a batch of observations, the actor and an sg_qnet to the action, the critics'
// values and action gradients, the loss alpha logp - Q, its statistics and the ACTOR's parameter gradients.  For row i:
//     head     = actor MLP(obs[i])                                      exactly as policy_net runs it
//     squashed: (a, logp) = squashed_tail(head, eps[i])                 (eps NULL: zeros)
//     gaussian: a_d = fmaf(expf(log_std_d), eps[i][d], head_d);  logp = 0  (alpha is 0)
//     critic c: q_c = Qc(obs[i], a);  dq_c[d] = 0.0f + d Qc / d a_d     policy_grad_net with the head's dz = 1, no weights, want_dx
//     q_select = 1 (both critics run): sel2 = q2 < q1 || q2 != q2 (q_td_min's rule, ties to critic 1);  q_select = 0: critic 1 alone
//     q_sel = sel2 ? q2 : q1;  loss_i = fsub(fmul(alpha, logp), q_sel)  (alpha = *alpha_dev when given, else cfg.alpha)
//     g_action[d] = (-dq_sel[d]) / (float)n;  g_logp = alpha / (float)n
//     the actor's head dz: squashed_grad_kernel's score of (g_action, g_logp); gaussian: policy_action_grad_kernel's of g_action
// d Q / d a is linear in the head's dz, so one pass per critic with dz = 1 gives both q_c and dq_c: the critics run once, and the
// selection needs no walk of its own.  The critics' parameters get no gradient.  tests/q_actor_model.py states the same in NumPy.
//
// Launches: q_actor_*_grad_kernel (q_grad_kernel's frame -- the tile loop, the grid cap, the ACTOR's PolicyGradLayout and per-workgroup
// partial sums -- with both nets' PolicyDev; NT is the larger of the two nets' width classes, the staging area and the store are sized
// for the larger of the two nets; per tile: the actor's forward and the tail (a policy_grad_net call with no weights and a zero dz),
// critic 0's policy_grad_net, critic 1's, then the actor's policy_grad_net with weights, whose forward is recomputed because the store
// holds one net at a time; then q_td_grad_kernel's statistics fold), q_actor_reduce_kernel (q_td_reduce_kernel's shape).  Given the
// per-row g_action the kernel formed, the gradients are squashed_grad_kernel's / policy_action_grad_kernel's bit for bit wherever the
// tile of NT holds as many rows as the actor's own class's.  Every sum has a fixed order: the same inputs and the same n give the same bits.
constexpr int kQActorStats = 9, kQActorSums = 8;  // floats of stats_out; per-workgroup sums: loss, logp, q1, q2, q_sel, sel2, |a|, max |dq|
constexpr int kQActorMaxSlot = 7;                 // the one sum that is a maximum
// workspace: the parameter partials float [groups][total], then float [groups][kQActorSums]

struct QActorDev {
    const float *eps, *alpha_dev;
    float *row_action, *row_logp, *row_q1, *row_q2, *row_q_sel, *row_dq1, *row_dq2, *row_g_action;
    float alpha;
    int two;  // q_select: both critics run and the smaller one is taken
};

// the maximum that hands a NaN on, whichever side it is on (fmaxf would drop it): section 32's rule for every min, max and clamp
__device__ __forceinline__ float q_actor_max(float a, float b) { return b > a || b != b ? b : a; }

// LDS of one workgroup: policy_grad_lds_bytes for the larger staging area and the larger store of the two nets
static inline size_t q_actor_lds_bytes(int nt, const PolicyDev &a, const PolicyDev &q) {
    const int wt_rows = std::max(policy_grad_wt_rows(a.hidden, a.obs_dim), policy_grad_wt_rows(q.hidden, q.obs_dim));
    const int rows = std::max(policy_grad_store_rows(a.n_hidden, a.hidden, a.obs_dim), policy_grad_store_rows(q.n_hidden, q.hidden, q.obs_dim));
    return sizeof(float) * ((size_t)wt_rows * (kPolicyGradChunk + kPolicyRowPad) + kPolicyGradChunk + (size_t)rows * (policy_grad_block(nt) + 2));
}

//   tail   (head outputs, eps, act, logp): the row's action and log-prob
//   score  (head outputs, eps, g_action, g_logp, live, dz): the actor's head dz of the row, zeros for an idle lane
template <int NT, typename Tail, typename Score>
__device__ __forceinline__ void q_actor_grad_body(const PolicyDev &a, int head, int extra, const PolicyDev &q, const QActorDev &r, int n,
                                                  const float *__restrict__ obs, const PolicyGradLayout &lay, float *__restrict__ ws,
                                                  float *__restrict__ sums, float *lds, Tail tail, Score score) {
    const int R = (int)blockDim.x, S = R + 2, tid = (int)threadIdx.x, tiles = (int)(((int64_t)n + R - 1) / R);  // (n may be 2^31 - 1)
    float *wt = lds;
    float *bs = wt + (size_t)max(max(max(a.hidden, a.obs_dim), max(q.hidden, q.obs_dim)), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + (size_t)blockIdx.x * lay.total;
    const float nf = (float)n;
    const float alpha = r.alpha_dev ? *r.alpha_dev : r.alpha;
    const float gl = alpha / nf;
    float acc = 0.0f;  // lane s < kQActorSums: this workgroup's sum (s = 7: maximum) s over its rows, in row order
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int64_t at = (int64_t)tile * R + tid;  // (past n in the last tile: may not fit an int)
        const bool live = at < n;
        const int i = live ? (int)at : n - 1;
        const float *obs_row = obs + (size_t)i * a.obs_dim;  // idle lanes of the last tile redo its last row with zero loss gradients
        float e[kPolicyActDim] = {0.0f, 0.0f};
        if (r.eps) {
            const float2 e2 = reinterpret_cast<const float2 *>(r.eps)[i];
            e[0] = e2.x; e[1] = e2.y;
        }
        // 1. the actor's forward and the tail: policy_grad_net with no weights and a zero dz, whose walk down moves zeros (its forward
        // half as a function of its own changed the registers of the existing grad kernels, so policy_grad_net stays whole)
        float act[kPolicyActDim] = {0.0f, 0.0f}, logp = 0.0f, no_dx[kPolicyActDim];
        policy_grad_net<NT>(a, 0, head, 0, obs_row, nullptr, [&](const float (&o)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
            tail(o, e, act, logp);
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
        }, lay, part, first, false, false, no_dx, wt, bs, store);
        // 2., 3. the critics at (obs, a): the head's dz = 1 gives q_c and d q_c / d a in one pass
        float q1 = 0.0f, q2 = 0.0f, dq1[kPolicyActDim] = {0.0f, 0.0f}, dq2[kPolicyActDim] = {0.0f, 0.0f};
        for (int c = 0; c < 2; c++) {
            if (c && !r.two) break;  // (uniform)
            float qc = 0.0f, dx[kPolicyActDim] = {0.0f, 0.0f};
            policy_grad_net<NT>(q, c, 1, 0, obs_row, act, [&](const float (&o)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
                qc = o[0];
#pragma unroll
                for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
                dz[0] = live ? 1.0f : 0.0f;
            }, lay, part, first, false, true, dx, wt, bs, store);
            if (c) { q2 = qc; dq2[0] = 0.0f + dx[0]; dq2[1] = 0.0f + dx[1]; }  // (selected, not indexed: everything stays in registers)
            else { q1 = qc; dq1[0] = 0.0f + dx[0]; dq1[1] = 0.0f + dx[1]; }
        }
        const bool sel2 = r.two && (q2 < q1 || q2 != q2);
        const float q_sel = sel2 ? q2 : q1;
        const float loss = __fsub_rn(__fmul_rn(alpha, logp), q_sel);
        float ga[kPolicyActDim];
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) ga[d] = (-(sel2 ? dq2[d] : dq1[d])) / nf;
        if (live) {
            if (r.row_action) reinterpret_cast<float2 *>(r.row_action)[i] = make_float2(act[0], act[1]);
            if (r.row_logp) r.row_logp[i] = logp;
            if (r.row_q1) r.row_q1[i] = q1;
            if (r.row_q2) r.row_q2[i] = q2;
            if (r.row_q_sel) r.row_q_sel[i] = q_sel;
            if (r.row_dq1) reinterpret_cast<float2 *>(r.row_dq1)[i] = make_float2(dq1[0], dq1[1]);
            if (r.row_dq2) reinterpret_cast<float2 *>(r.row_dq2)[i] = make_float2(dq2[0], dq2[1]);
            if (r.row_g_action) reinterpret_cast<float2 *>(r.row_g_action)[i] = make_float2(ga[0], ga[1]);
        }
        float c_sum[kQActorSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            c_sum[0] = loss; c_sum[1] = logp; c_sum[2] = q1; c_sum[3] = q2; c_sum[4] = q_sel; c_sum[5] = sel2 ? 1.0f : 0.0f;
            c_sum[6] = 0.5f * (fabsf(act[0]) + fabsf(act[1]));
            c_sum[7] = q_actor_max(q_actor_max(fabsf(dq1[0]), fabsf(dq1[1])), q_actor_max(fabsf(dq2[0]), fabsf(dq2[1])));  // (critic 2 not run: zeros)
        }
        // 4. the actor's backward: its forward again, the score of (g_action, g_logp) as the head's dz
        policy_grad_net<NT>(a, 0, head, extra, obs_row, nullptr, [&](const float (&o)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
            score(o, e, ga, gl, live, dz);
        }, lay, part, first, true, false, no_dx, wt, bs, store);
        first = false;
        // the statistics of the tile: each row's terms to the store (free once every wave has left the walk), lane s folds column s
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kQActorSums; s++) store[(size_t)s * S + tid] = c_sum[s];
        __syncthreads();
        if (tid < kQActorSums) {
            // (the trip count as a constant and one body for the sum and the maximum, as q_td_grad_kernel)
            const float *col = store + (size_t)tid * S;
            const bool is_max = tid == kQActorMaxSlot;
#pragma unroll 16
            for (int k = 0; k < policy_grad_block(NT); k++) {
                const float v = col[k];
                acc = is_max ? q_actor_max(acc, v) : acc + v;
            }
        }
    }
    if (tid < kQActorSums) sums[(size_t)blockIdx.x * kQActorSums + tid] = acc;
}

// The SAC actor (sg_squashed.inc): squashed_tail, and squashed_grad_kernel's score
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void q_actor_squashed_grad_kernel(PolicyDev a, SquashedBounds b, PolicyDev q, QActorDev r, int n,
                                                                                      const float *__restrict__ obs, PolicyGradLayout lay,
                                                                                      float *__restrict__ ws, float *__restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    q_actor_grad_body<NT>(a, kSquashedHead, 0, q, r, n, obs, lay, ws, sums, sg_policy_lds,
                          [&](const float (&out)[kPolicyHeadPad], const float (&eps)[kPolicyActDim], float (&act)[kPolicyActDim], float &logp) {
        squashed_tail(out, eps, b, act, logp);
    }, [&](const float (&out)[kPolicyHeadPad], const float (&eps)[kPolicyActDim], const float (&ga)[kPolicyActDim], float gl, bool live,
           float (&dz)[kPolicyHeadPad]) {
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
    });
}

// The Gaussian actor of policy_action_kernel (sg_qnet.inc): its action, and policy_action_grad_kernel's score with the two log_std rows
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void q_actor_gaussian_grad_kernel(PolicyDev a, PolicyDev q, QActorDev r, int n,
                                                                                      const float *__restrict__ obs, PolicyGradLayout lay,
                                                                                      float *__restrict__ ws, float *__restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const bool noisy = r.eps != nullptr;
    q_actor_grad_body<NT>(a, a.head, kPolicyActDim, q, r, n, obs, lay, ws, sums, sg_policy_lds,
                          [&](const float (&out)[kPolicyHeadPad], const float (&eps)[kPolicyActDim], float (&act)[kPolicyActDim], float &logp) {
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) {
            const float ls = a.log_std[d];
            act[d] = fmaf(expf(ls), eps[d], out[d]);
        }
        logp = 0.0f;
    }, [&](const float (&)[kPolicyHeadPad], const float (&eps)[kPolicyActDim], const float (&ga)[kPolicyActDim], float, bool live,
           float (&dz)[kPolicyHeadPad]) {
#pragma unroll
        for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
        if (!live) return;
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) {
            dz[d] = ga[d];
            dz[kPolicyActDim + d] = noisy ? ga[d] * (expf(a.log_std[d]) * eps[d]) : 0.0f;
        }
    });
}

// policy_grad_reduce_kernel, and one workgroup more: the statistics partials folded in workgroup order by lanes 0 .. 7, then stats_out
// [kQActorStats] by lane 0: loss, logp_mean, q1_mean, q2_mean, q_sel_mean, critic2_fraction, action_abs_mean, dq_da_abs_max,
// log_alpha_grad = -(logp_mean + target_entropy) (temperature 0, the Gaussian form: 0)
__global__ __launch_bounds__(256) void q_actor_reduce_kernel(const float *__restrict__ ws, int parts, int total, PolicyGradOut o,
                                                             const float *__restrict__ sums, int n, int temperature, float target_entropy,
                                                             float *__restrict__ stats) {
    if (blockIdx.x + 1 < gridDim.x) {
        const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        if (e < total) policy_grad_reduce_element(ws, parts, total, o, e, 0);
        return;
    }
    __shared__ float tot[kQActorSums];
    const int t = (int)threadIdx.x;
    if (t < kQActorSums) {
        float sum = sums[t];
        for (int g = 1; g < parts; g++) {
            const float v = sums[(size_t)g * kQActorSums + t];
            sum = t == kQActorMaxSlot ? q_actor_max(sum, v) : sum + v;
        }
        tot[t] = sum;
    }
    __syncthreads();
    if (t != 0) return;
    const float nf = (float)n;
    const float logp_mean = tot[1] / nf;
    stats[0] = tot[0] / nf;
    stats[1] = logp_mean;
    stats[2] = tot[2] / nf;
    stats[3] = tot[3] / nf;  // (critic 2 not run: its sum is 0)
    stats[4] = tot[4] / nf;
    stats[5] = tot[5] / nf;
    stats[6] = tot[6] / nf;
    stats[7] = tot[7];
    stats[8] = temperature ? -(logp_mean + target_entropy) : 0.0f;
}
