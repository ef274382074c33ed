// The Double-DQN TD update in one call (sg_dqn_td_grad_device; DESIGN section 31): from a replay batch, an online and a target net to
// the TD target, the Huber loss, its statistics and the online net's parameter gradients.  For row i of the batch, with Q = policy_net's
// six head outputs and dqn_argmax / dqn_select exactly as sg_dqn_evaluate_device uses them:
//     a*      = dqn_argmax(Q_online(next_obs[i]))                           (double_q; the first maximum)
//     q_next  = dqn_select(Q_target(next_obs[i]), a*)                       (double_q; else the maximum of Q_target(next_obs[i]))
//     y       = terminated[i] ? reward[i] : fadd(reward[i], fmul(discount[i], q_next))      two roundings, never an fma
//     q_taken = dqn_select(Q_online(obs[i]), action[i]);  td = q_taken - y
//     c       = min(max(td, -delta), +delta);  w = weight ? weight[i] : 1
//     g       = (w * c) / (float)n                                          the product rounded, then the quotient
//     loss_i  = w * (|td| <= delta ? 0.5 * (td * td) : delta * (|td| - 0.5 * delta));  dz_j = (action[i] == j) ? g : 0
// delta = +inf gives the squared loss 0.5 td^2.  A terminated row never multiplies its q_next: an infinite one leaves y = reward.
// tests/dqn_td_model.py states the same in NumPy.
//
// Launches: dqn_td_target_kernel (dqn_evaluate_kernel's frame: one row per lane, policy_net; with double_q the online net, then the
// target net re-staged into the same LDS), dqn_td_grad_kernel (dqn_grad_kernel's frame -- the same tiles, grid cap, workspace layout and
// policy_grad_net with a head of 6 -- with the loss gradient formed from the head outputs, and ppo_grad_kernel's per-workgroup
// statistics sums), dqn_td_reduce_kernel (policy_grad_reduce_element per parameter, and one workgroup more that folds the statistics in
// workgroup order).  Given the per-row g the kernel formed, the parameter gradients are dqn_grad_kernel's bit for bit at the same n.
// An action outside 0 .. 5 is never an index (the selections compare); such a row contributes zero to every gradient and statistic,
// reports g = 0 and td_error = 0, is counted in bad_rows, and the means still divide by n.  No atomics: the same inputs and the same n
// give the same bits.
constexpr int kDqnTdStats = 8, kDqnTdSums = 8;  // floats of stats_out; per-workgroup sums: loss, |td|, max |td|, q_taken, y, clipped, weight, bad
constexpr int kDqnTdMaxSlot = 2;                // the one sum that is a maximum
// workspace: the parameter partials float [groups][total], then float [groups][kDqnTdSums], then y float [n]

struct DqnTdDev {
    const float *next_obs, *reward, *discount, *weight;
    const uint8_t *terminated;
    float *row_td, *row_q_taken, *row_target, *row_q_next, *row_g;
    float delta;
    int double_q;
};

template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void dqn_td_target_kernel(PolicyDev online, PolicyDev target, DqnTdDev q, int n,
                                                                         float *__restrict__ y_out) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    constexpr int J = kPolicyTile * NT;
    const int first = (int)blockIdx.x * (int)blockDim.x;
    if (first >= n) return;  // (the whole workgroup: no barrier is left waiting)
    const bool live = (int64_t)first + (int)threadIdx.x < n;  // (the sum may pass 2^31 - 1 in the last workgroup)
    const int i = live ? first + (int)threadIdx.x : n - 1;  // idle lanes of the last workgroup redo its last row
    const float *obs_row = q.next_obs + (size_t)i * target.obs_dim;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(target.hidden, target.obs_dim) * (J + kPolicyRowPad);  // (both nets have one shape: the host refuses otherwise)
    float *h = bs + J + threadIdx.x;
    float out[kPolicyHeadPad], mx;
    int a = 0;
    if (q.double_q) {  // (uniform over the grid)
        policy_net<NT>(online, online.actor, kDqnHead, obs_row, wt, bs, h, out);
        a = dqn_argmax(out, mx);
    }
    policy_net<NT>(target, target.actor, kDqnHead, obs_row, wt, bs, h, out);  // (its first barrier: every lane has left the online head)
    if (!live) return;
    if (q.double_q) mx = dqn_select(out, a);
    else dqn_argmax(out, mx);
    const float r = q.reward[i];
    const float y = q.terminated[i] ? r : __fadd_rn(r, __fmul_rn(q.discount[i], mx));
    y_out[i] = y;
    if (q.row_target) q.row_target[i] = y;
    if (q.row_q_next) q.row_q_next[i] = mx;
}

template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void dqn_td_grad_kernel(PolicyDev p, DqnTdDev q, int n, const float *__restrict__ obs,
                                                                            const int32_t *__restrict__ action, const float *__restrict__ y,
                                                                            PolicyGradLayout lay, float *__restrict__ ws,
                                                                            float *__restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, S = R + 2, tid = (int)threadIdx.x, tiles = (int)(((int64_t)n + R - 1) / R);  // (n may be 2^31 - 1)
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + (size_t)blockIdx.x * lay.total;
    const float nf = (float)n;
    float acc = 0.0f;  // lane s < kDqnTdSums: this workgroup's sum (s = 2: maximum) s over its rows, in row order
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int64_t at = (int64_t)tile * R + tid;  // (past n in the last tile: may not fit an int)
        const bool live = at < n;
        const int i = live ? (int)at : n - 1;
        const size_t row = (size_t)i;  // idle lanes of the last tile redo its last row with zero loss gradients
        const int a = action[i];
        const bool on = live && a >= 0 && a < kDqnHead;
        float c_sum[kDqnTdSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, live && !on ? 1.0f : 0.0f};
        float no_dx[kPolicyActDim];  // (no gradient by the input row here)
        policy_grad_net<NT>(p, 0, kDqnHead, 0, obs + row * p.obs_dim, nullptr,
                            [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
            const float qt = dqn_select(out, a), yi = y[i], td = qt - yi;
            const float cl = fminf(fmaxf(td, -q.delta), q.delta);
            const float w = q.weight ? q.weight[i] : 1.0f;
            const float g = on ? (w * cl) / nf : 0.0f;
            if (on) {
                const float ad = fabsf(td);
                c_sum[0] = w * (ad <= q.delta ? 0.5f * (td * td) : q.delta * (ad - 0.5f * q.delta));
                c_sum[1] = ad;
                c_sum[2] = ad;
                c_sum[3] = qt;
                c_sum[4] = yi;
                c_sum[5] = ad > q.delta ? 1.0f : 0.0f;
                c_sum[6] = w;
            }
            if (live) {
                if (q.row_td) q.row_td[i] = on ? td : 0.0f;
                if (q.row_q_taken) q.row_q_taken[i] = qt;
                if (q.row_g) q.row_g[i] = g;
            }
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
#pragma unroll
            for (int j = 0; j < kDqnHead; j++) dz[j] = a == j ? g : 0.0f;  // (selected by comparison, as dqn_select)
        }, lay, part, first, true, false, no_dx, wt, bs, store);
        first = false;
        // the statistics of the tile: each row's terms to the store (free once every wave has left the walk), lane s folds column s
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kDqnTdSums; s++) store[(size_t)s * S + tid] = c_sum[s];
        __syncthreads();
        if (tid < kDqnTdSums) {
            // (the trip count as a constant and one body for the sum and the maximum: the loads of 16 rows are in flight together,
            // the additions stay in row order; with the run-time count every row waited for its own LDS read)
            const float *col = store + (size_t)tid * S;
            const bool is_max = tid == kDqnTdMaxSlot;
#pragma unroll 16
            for (int k = 0; k < policy_grad_block(NT); k++) {
                const float v = col[k];
                acc = is_max ? fmaxf(acc, v) : acc + v;
            }
        }
    }
    if (tid < kDqnTdSums) sums[(size_t)blockIdx.x * kDqnTdSums + tid] = acc;
}

// policy_grad_reduce_kernel, and one workgroup more: the statistics partials folded in workgroup order by lanes 0 .. 7, then stats_out
// [kDqnTdStats] by lane 0: loss, td_abs_mean, td_abs_max, q_mean, target_mean, clip_fraction, weight_mean, bad_rows
__global__ __launch_bounds__(256) void dqn_td_reduce_kernel(const float *__restrict__ ws, int parts, int total, PolicyGradOut o,
                                                            const float *__restrict__ sums, int n, float *__restrict__ stats) {
    if (blockIdx.x + 1 < gridDim.x) {
        const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        if (e < total) policy_grad_reduce_element(ws, parts, total, o, e, 0);
        return;
    }
    __shared__ float tot[kDqnTdSums];
    const int t = (int)threadIdx.x;
    if (t < kDqnTdSums) {
        float sum = sums[t];
        for (int g = 1; g < parts; g++) {
            const float v = sums[(size_t)g * kDqnTdSums + t];
            sum = t == kDqnTdMaxSlot ? fmaxf(sum, v) : sum + v;
        }
        tot[t] = sum;
    }
    __syncthreads();
    if (t != 0) return;
    const float nf = (float)n;
    stats[0] = tot[0] / nf;
    stats[1] = tot[1] / nf;
    stats[2] = tot[2];
    stats[3] = tot[3] / nf;
    stats[4] = tot[4] / nf;
    stats[5] = tot[5] / nf;
    stats[6] = tot[6] / nf;
    stats[7] = tot[7];
}
