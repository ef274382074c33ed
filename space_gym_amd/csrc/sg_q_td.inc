// The TD critic update of SAC, TD3 and DDPG in one call (sg_q_td_grad_device; DESIGN section 32): from a replay batch, the target action
// the caller formed, an online and a target sg_qnet to the TD target, the Huber loss, its statistics and the ONLINE critics' parameter
// gradients.  For row i of the batch, with Qc = policy_net on [obs | action] with head 1, exactly as sg_q_evaluate_device runs it:
//     a'_d    = next_action[i][d]
//               noise given:  e = min(max(fmul(noise_std, noise[i][d]), -noise_clip), noise_clip)
//                             a'_d = min(max(fadd(a'_d, e), -action_clip), action_clip)      (noise NULL: a' used as given, never clamped)
//     q_next  = min(Q1_target(next_obs[i], a'), Q2_target(next_obs[i], a'))                  (one critic: Q1_target)
//               next_logp given:  q_next = fsub(q_next, fmul(alpha, next_logp[i]))           (alpha = *alpha_dev when given, else cfg.alpha)
//     y       = terminated[i] ? reward[i] : fadd(reward[i], fmul(discount[i], q_next))       (a select: two roundings, never an fma)
//     per critic c of the online handle:  q_c = Qc(obs[i], action[i]);  td_c = q_c - y
//               cl_c = min(max(td_c, -delta), delta);  w = weight ? weight[i] : 1;  g_c = (w * cl_c) / (float)n
//               l_c  = w * (|td_c| <= delta ? 0.5 * (td_c * td_c) : delta * (|td_c| - 0.5 * delta))
//     loss    = (1 / n) sum_i (l_1 + l_2);  dz of critic c's head = g_c
// delta = +inf gives 0.5 td^2 per critic: half of the sum of the two mean squared errors that CleanRL's and SB3's TD3 minimise.  A
// terminated row never multiplies its q_next: an infinite one leaves y = reward.  Every min, max and clamp above hands a NaN on, as
// torch.minimum and torch.clamp do (q_td_min / q_td_clamp): non-finite inputs propagate as they do in torch, and there is no bad-row
// rule, because no action is an index.  tests/q_td_model.py states the same in NumPy.
//
// Launches: q_td_target_kernel (q_evaluate_kernel's frame on the TARGET critics, one row of next_obs per lane; a' lives in two
// registers and is policy_net's `tail`; critic 0, then critic 1 in the same LDS), q_td_grad_kernel (q_grad_kernel's frame on the ONLINE
// critics with no action gradient -- the same tiles, grid cap, workspace layout and order: critic 0's policy_grad_net, then critic 1's,
// per tile -- with the loss gradient formed from the head output, and dqn_td_grad_kernel's per-workgroup statistics sums),
// q_td_reduce_kernel (policy_grad_reduce_element per parameter, and one workgroup more that folds the statistics in workgroup order).
// Given the per-row g_1 / g_2 the kernel formed, the parameter gradients are q_grad_kernel's bit for bit at the same n.  Every sum has a
// fixed order: the same inputs and the same n give the same bits.
constexpr int kQTdStats = 9, kQTdSums = 9;  // floats of stats_out; per-workgroup sums: loss, |td1|, |td2|, max |td|, q1, q2, y, clipped, weight
constexpr int kQTdMaxSlot = 3;              // the one sum that is a maximum
// workspace: the parameter partials float [groups][total], then float [groups][kQTdSums], then y float [n]

struct QTdDev {
    const float *next_obs, *next_action, *noise, *next_logp, *alpha_dev, *reward, *discount, *weight;
    const uint8_t *terminated;
    float *row_td1, *row_td2, *row_q1, *row_q2, *row_g1, *row_g2, *row_target, *row_q_next, *row_td_abs;
    float delta, alpha, noise_std, noise_clip, action_clip;
};

// torch.minimum / torch.clamp: a NaN operand gives NaN (fminf / fmaxf would drop it); the same values as fminf / fmaxf otherwise
__device__ __forceinline__ float q_td_min(float a, float b) { return b < a || b != b ? b : a; }
__device__ __forceinline__ float q_td_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void q_td_target_kernel(PolicyDev target, QTdDev q, int n, float *__restrict__ y_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;  // (the whole workgroup: no barrier is left waiting)
    const bool live = (int64_t)first + (int)threadIdx.x < n;  // (the sum may pass 2^31 - 1 in the last workgroup)
    const int i = live ? first + (int)threadIdx.x : n - 1;  // idle lanes of the last workgroup redo its last row
    const float *obs_row = q.next_obs + (size_t)i * (target.obs_dim - kPolicyActDim);
    const float2 a2 = reinterpret_cast<const float2 *>(q.next_action)[i];
    float a[kPolicyActDim] = {a2.x, a2.y};  // a': the critics' tail
    if (q.noise) {  // (uniform over the grid) TD3's target smoothing
        const float2 e2 = reinterpret_cast<const float2 *>(q.noise)[i];
        const float e[kPolicyActDim] = {e2.x, e2.y};
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) {
            const float ed = q_td_clamp(__fmul_rn(q.noise_std, e[d]), -q.noise_clip, q.noise_clip);
            a[d] = q_td_clamp(__fadd_rn(a[d], ed), -q.action_clip, q.action_clip);
        }
    }
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(target.hidden, target.obs_dim) * (J + kPolicyRowPad);
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad];
    policy_net<NT>(target, target.actor, 1, obs_row, wt, bs, h, out, a);
    float qn = out[0];
    if (target.critic.w[0]) {  // (uniform) its first barrier: every lane has left critic 0's head
        policy_net<NT>(target, target.critic, 1, obs_row, wt, bs, h, out, a);
        qn = q_td_min(qn, out[0]);
    }
    if (!live) return;
    if (q.next_logp) {  // SAC's entropy term
        const float alpha = q.alpha_dev ? *q.alpha_dev : q.alpha;
        qn = __fsub_rn(qn, __fmul_rn(alpha, q.next_logp[i]));
    }
    const float r = q.reward[i];
    const float y = q.terminated[i] ? r : __fadd_rn(r, __fmul_rn(q.discount[i], qn));
    y_out[i] = y;
    if (q.row_target) q.row_target[i] = y;
    if (q.row_q_next) q.row_q_next[i] = qn;
}

template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void q_td_grad_kernel(PolicyDev p, QTdDev q, int n, const float *__restrict__ obs,
                                                                          const float *__restrict__ action, const float *__restrict__ y,
                                                                          PolicyGradLayout lay, float *__restrict__ ws,
                                                                          float *__restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, S = R + 2, tid = (int)threadIdx.x, tiles = (int)(((int64_t)n + R - 1) / R);  // (n may be 2^31 - 1)
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + (size_t)blockIdx.x * lay.total;
    const float nf = (float)n;
    const bool two = p.critic.w[0] != nullptr;
    float acc = 0.0f;  // lane s < kQTdSums: this workgroup's sum (s = 3: maximum) s over its rows, in row order
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int64_t at = (int64_t)tile * R + tid;  // (past n in the last tile: may not fit an int)
        const bool live = at < n;
        const int i = live ? (int)at : n - 1;
        const size_t row = (size_t)i;  // idle lanes of the last tile redo its last row with zero loss gradients
        const float *obs_row = obs + row * (p.obs_dim - kPolicyActDim), *act_row = action + row * kPolicyActDim;
        const float yi = y[i], w = q.weight ? q.weight[i] : 1.0f;
        float c_sum[kQTdSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, live ? yi : 0.0f, 0.0f, live ? w : 0.0f};
        float no_dx[kPolicyActDim];  // (no gradient by the action here)
        for (int c = 0; c < 2; c++) {  // the first critic's contribution before the second's, as q_grad_kernel
            if (c && !two) break;  // (uniform)
            policy_grad_net<NT>(p, c, 1, 0, obs_row, act_row, [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
                const float qc = out[0], td = qc - yi;
                const float cl = q_td_clamp(td, -q.delta, q.delta);
                const float g = live ? (w * cl) / nf : 0.0f;
                if (live) {
                    const float ad = fabsf(td);
                    c_sum[0] += w * (ad <= q.delta ? 0.5f * (td * td) : q.delta * (ad - 0.5f * q.delta));
                    if (c) { c_sum[2] = ad; c_sum[5] = qc; }  // (selected, not indexed: the sums stay in registers)
                    else { c_sum[1] = ad; c_sum[4] = qc; }
                    c_sum[3] = fmaxf(c_sum[3], ad);
                    c_sum[7] += ad > q.delta ? 1.0f : 0.0f;
                    float *row_td = c ? q.row_td2 : q.row_td1, *row_q = c ? q.row_q2 : q.row_q1, *row_g = c ? q.row_g2 : q.row_g1;
                    if (row_td) row_td[i] = td;
                    if (row_q) row_q[i] = qc;
                    if (row_g) row_g[i] = g;
                }
#pragma unroll
                for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
                dz[0] = g;
            }, lay, part, first, true, false, no_dx, wt, bs, store);
        }
        first = false;
        if (live && q.row_td_abs) q.row_td_abs[i] = two ? 0.5f * (c_sum[1] + c_sum[2]) : c_sum[1];
        // the statistics of the tile: each row's terms to the store (free once every wave has left the walk), lane s folds column s
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kQTdSums; s++) store[(size_t)s * S + tid] = c_sum[s];
        __syncthreads();
        if (tid < kQTdSums) {
            // (the trip count as a constant and one body for the sum and the maximum, as dqn_td_grad_kernel: the loads of 16 rows are
            // in flight together, the additions stay in row order)
            const float *col = store + (size_t)tid * S;
            const bool is_max = tid == kQTdMaxSlot;
#pragma unroll 16
            for (int k = 0; k < policy_grad_block(NT); k++) {
                const float v = col[k];
                acc = is_max ? fmaxf(acc, v) : acc + v;
            }
        }
    }
    if (tid < kQTdSums) sums[(size_t)blockIdx.x * kQTdSums + tid] = acc;
}

// policy_grad_reduce_kernel, and one workgroup more: the statistics partials folded in workgroup order by lanes 0 .. 8, then stats_out
// [kQTdStats] by lane 0: loss, td1_abs_mean, td2_abs_mean, td_abs_max, q1_mean, q2_mean, target_mean, clip_fraction, weight_mean
__global__ __launch_bounds__(256) void q_td_reduce_kernel(const float *__restrict__ ws, int parts, int total, PolicyGradOut o,
                                                          const float *__restrict__ sums, int n, int critics, float *__restrict__ stats) {
    if (blockIdx.x + 1 < gridDim.x) {
        const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        if (e < total) policy_grad_reduce_element(ws, parts, total, o, e, 0);
        return;
    }
    __shared__ float tot[kQTdSums];
    const int t = (int)threadIdx.x;
    if (t < kQTdSums) {
        float sum = sums[t];
        for (int g = 1; g < parts; g++) {
            const float v = sums[(size_t)g * kQTdSums + t];
            sum = t == kQTdMaxSlot ? fmaxf(sum, v) : sum + v;
        }
        tot[t] = sum;
    }
    __syncthreads();
    if (t != 0) return;
    const float nf = (float)n;
    stats[0] = tot[0] / nf;
    stats[1] = tot[1] / nf;
    stats[2] = tot[2] / nf;  // (one critic: its sums are 0)
    stats[3] = tot[3];
    stats[4] = tot[4] / nf;
    stats[5] = tot[5] / nf;
    stats[6] = tot[6] / nf;
    stats[7] = tot[7] / ((float)critics * nf);
    stats[8] = tot[8] / nf;
}
