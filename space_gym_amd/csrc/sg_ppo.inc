// The PPO minibatch update in one call (sg_ppo_grad_device; DESIGN section 24): from stored rollout rows and a minibatch index to the
// parameter gradients and the loss statistics.  The objective is the CleanRL / SB3 form.  For row i of the minibatch, r = index[i]
// (r = i without an index), with logp, entropy, value exactly policy_score / policy_net's values:
//     lr = logp - old_logp[r];  ratio = exp(lr);  A = (adv[r] - mean) * rstd when normalising, else adv[r]
//     pg = max(-A ratio, -A clamp(ratio, 1 - c, 1 + c))
//     vl = 0.5 max((value - ret)^2, (vclip - ret)^2),  vclip = old_value + clamp(value - old_value, -cv, cv)   (cv > 0; else 0.5 (value - ret)^2)
//     loss = mean(pg) - ent_coef mean(entropy) + vf_coef mean(vl)
//     g_logp = -A ratio / n where the unclipped term is >= the clipped one, else 0;  g_entropy = -ent_coef / n
//     g_value = vf_coef (value - ret) / n where the unclipped square is >= the clipped one, else vf_coef (vclip - ret) / n inside the
//               clamp (bounds included) and 0 outside it
// torch's subgradients: clamp passes the gradient at its bounds, a tie of the two branches takes the unclipped one (there both give the
// same derivative, or A = 0).  c = +inf gives the unclipped policy gradient (A2C).  tests/ppo_model.py states the same in NumPy.
//
// Launches: ppo_adv_stats_kernel (normalising only; ppo_adv_finish turns its partials into mean and rstd where they are used),
// ppo_grad_kernel, ppo_reduce_kernel.  ppo_grad_kernel is policy_grad_kernel's frame -- the same tiles, grid cap, workspace layout and
// policy_grad_net -- with the row gathered through the index, the critic first (its callback forms g_value from the head output) and
// the actor's callback forming g_logp before it calls policy_score.  Given the per-row g_logp / g_value the kernel formed, the
// parameter gradients are policy_grad_kernel's bit for bit at the same n.
// An index outside [0, rows) is clamped before ANY address is formed from it; such a row contributes zero to every gradient and
// statistic, is counted in bad_rows, and the means still divide by n.  No atomics: the same inputs and the same n give the same bits.
//
// Populations (sg_ppo_population_grad_device; DESIGN section 25): the same three launches with the member in blockIdx.y.  Member m's
// minibatch entries are m n + i of index / the per-row outputs [P, n], its parameters policy_grad_net's and policy_score's member m,
// its partial sums ws[m][group][parameter], its statistics sums [m][group][8], its advantage partials [m][Gadv][2], and its four
// coefficients row m of member_coef [P, 4] when that is given.  The advantage pass and the statistics are one body each for both
// forms (`member` 0, folded away, in the single-policy kernels); the backward has a frame of its own (see ppo_population_grad_kernel).
constexpr int kPpoStats = 12, kPpoSums = 8;  // floats of stats_out; per-workgroup sums: pg, vl, entropy, kl, old kl, clipped, bad, (pad)
// workspace after the parameter partials (rounded up to 8 bytes): double [kPpoAdvMaxGroups][2] advantage partials, then float [groups][kPpoSums]
constexpr int kPpoAdvBlock = 1024, kPpoAdvMaxGroups = 256;

struct PpoDev {
    const float *old_logp, *adv, *ret, *old_value;
    const int64_t *index;
    float *row_logp, *row_value, *row_g_logp, *row_g_value;
    int64_t rows;
    float clip, clip_vf, ent_coef, vf_coef;  // clip_vf <= 0: the value term is not clipped
    float adv_eps;
    int normalize, adv_groups;  // normalize: the advantage partials of adv_groups workgroups are in the workspace
};

// Row r of the rollout for entry i of the minibatch: the index clamped to [0, rows); good: it was inside
__device__ __forceinline__ int64_t ppo_row(const PpoDev &q, int64_t i, bool &good) {
    const int64_t r = q.index ? q.index[i] : i;
    good = r >= 0 && r < q.rows;
    return r < 0 ? 0 : r >= q.rows ? q.rows - 1 : r;
}

// The sum and the sum of squares, in float64, of adv[index[i]], i < n: workgroup g of G takes entries g 1024 + t, + G 1024, ... (lane t in
// ascending order), then a fixed tree over its lanes; part[g] = (sum, sum of squares).  A bad index counts as advantage 0.  One
// workgroup alone would walk n / 1024 dependent gathers per lane; G = min(ceil(n / 1024), 256) of them walk at most a few
__device__ __forceinline__ void ppo_adv_stats(const PpoDev &q, int64_t n, double *__restrict__ part, int member = 0) {
    __shared__ double sum[kPpoAdvBlock], sq[kPpoAdvBlock];
    const int t = (int)threadIdx.x;
    const int64_t base = (int64_t)member * n;  // the member's entries of the minibatch: base + i, i < n
    double s = 0.0, s2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kPpoAdvBlock + t; i < n; i += (int64_t)gridDim.x * kPpoAdvBlock) {
        bool good;
        const float a = q.adv[ppo_row(q, base + i, good)];
        const double v = good ? (double)a : 0.0;
        s += v;
        s2 += v * v;
    }
    sum[t] = s;
    sq[t] = s2;
    __syncthreads();
    for (int w = kPpoAdvBlock / 2; w > 0; w >>= 1) {
        if (t < w) { sum[t] += sum[t + w]; sq[t] += sq[t + w]; }
        __syncthreads();
    }
    if (t == 0) { part[2 * blockIdx.x] = sum[0]; part[2 * blockIdx.x + 1] = sq[0]; }
}
__global__ __launch_bounds__(kPpoAdvBlock) void ppo_adv_stats_kernel(PpoDev q, int64_t n, double *__restrict__ part) {
    ppo_adv_stats(q, n, part);
}
// Member blockIdx.y's entries by gridDim.x = Gadv = min(ceil(n / 1024), max(1, 256 / P)) workgroups: part [P][Gadv][2]
__global__ __launch_bounds__(kPpoAdvBlock) void ppo_population_adv_stats_kernel(PpoDev q, int64_t n, double *__restrict__ part) {
    const int m = (int)blockIdx.y;
    ppo_adv_stats(q, n, part + 2 * (size_t)m * gridDim.x, m);
}

// mean, 1 / (std + eps) and std from the partials, added in workgroup order: std unbiased (torch's .std()), all in float64, rounded once.
// Every lane that needs them runs this on the same values (n >= 2: the host refuses n = 1 when normalising)
__device__ __forceinline__ void ppo_adv_finish(const PpoDev &q, const double *__restrict__ part, int n, float &mean, float &rstd, float &sd) {
    double s = 0.0, s2 = 0.0;
    for (int g = 0; g < q.adv_groups; g++) { s += part[2 * g]; s2 += part[2 * g + 1]; }
    const double m = s / (double)n, d = sqrt(fmax(0.0, (s2 - s * m) / (double)(n - 1)));
    mean = (float)m;
    rstd = (float)(1.0 / (d + (double)q.adv_eps));
    sd = (float)d;
}

template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void ppo_grad_kernel(PolicyDev p, PpoDev q, int n, const float *__restrict__ obs,
                                                                         const void *__restrict__ action, PolicyGradLayout lay,
                                                                         float *__restrict__ ws, const double *__restrict__ adv_part,
                                                                         float *__restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, S = R + 2, tid = (int)threadIdx.x, tiles = (int)(((int64_t)n + R - 1) / R);
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + (size_t)blockIdx.x * lay.total;
    const bool critic = p.critic.w[0] != nullptr;
    const float nf = (float)n, ge_row = -q.ent_coef / nf;
    float mean = 0.0f, rstd = 1.0f, sd = 0.0f;
    if (q.normalize) ppo_adv_finish(q, adv_part, n, mean, rstd, sd);
    const float lo = 1.0f - q.clip, hi = 1.0f + q.clip;
    float acc = 0.0f;  // lane s < kPpoSums: this workgroup's sum s over its rows, in row order
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int64_t at = (int64_t)tile * R + tid;
        const bool live = at < n;
        bool good;
        const int64_t r = ppo_row(q, live ? at : n - 1, good);  // idle lanes of the last tile redo its last row with zero loss gradients
        const bool on = live && good;
        const float *obs_row = obs + (size_t)r * p.obs_dim;
        float c_sum[kPpoSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, live && !good ? 1.0f : 0.0f, 0.0f};
        float no_dx[kPolicyActDim];  // (no gradient by the input row here)
        if (critic) {
            policy_grad_net<NT>(p, 1, 1, 0, obs_row, nullptr, [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
                const float value = out[0], d = value - q.ret[r];
                float vl = 0.5f * (d * d), gv = q.vf_coef * d / nf;
                if (q.clip_vf > 0.0f) {
                    const float ov = q.old_value[r], dv = value - ov;
                    const float e2 = (ov + fminf(fmaxf(dv, -q.clip_vf), q.clip_vf)) - q.ret[r];
                    if (!(d * d >= e2 * e2)) {
                        vl = 0.5f * (e2 * e2);
                        gv = dv >= -q.clip_vf && dv <= q.clip_vf ? q.vf_coef * e2 / nf : 0.0f;
                    }
                }
                if (!on) gv = 0.0f;
                c_sum[1] = on ? vl : 0.0f;
                if (live && q.row_value) q.row_value[at] = value;
                if (live && q.row_g_value) q.row_g_value[at] = gv;
#pragma unroll
                for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
                dz[0] = gv;
            }, lay, part, first, true, false, no_dx, wt, bs, store);
        }
        policy_grad_net<NT>(p, 0, p.head, p.discrete ? 0 : kPolicyActDim, obs_row, nullptr,
                            [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
            PolicyScore s;
            policy_score(p, p.log_std, out, action, (int)r, 0.0f, 0.0f, false, s);
            const float lr = s.logp - q.old_logp[r], ratio = expf(lr);
            const float A = q.normalize ? (q.adv[r] - mean) * rstd : q.adv[r];
            const float t1 = -A * ratio, t2 = -A * fminf(fmaxf(ratio, lo), hi);
            const float gl = on && t1 >= t2 ? t1 / nf : 0.0f;
            if (on) {
                c_sum[0] = t1 >= t2 ? t1 : t2;
                c_sum[2] = s.entropy;
                c_sum[3] = (ratio - 1.0f) - lr;
                c_sum[4] = -lr;
                c_sum[5] = fabsf(ratio - 1.0f) > q.clip ? 1.0f : 0.0f;
            }
            if (live && q.row_logp) q.row_logp[at] = s.logp;
            if (live && q.row_g_logp) q.row_g_logp[at] = gl;
            policy_score(p, p.log_std, out, action, (int)r, gl, on ? ge_row : 0.0f, true, s);
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = s.dz[j];
        }, lay, part, first, true, false, no_dx, wt, bs, store);
        first = false;
        // the statistics of the tile: each row's terms to the store (free once every wave has left the actor's walk), lane s adds sum s
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kPpoSums; s++) store[(size_t)s * S + tid] = c_sum[s];
        __syncthreads();
        if (tid < kPpoSums) {
            const float *col = store + (size_t)tid * S;
            for (int k = 0; k < R; k++) acc += col[k];
        }
    }
    if (tid < kPpoSums) sums[(size_t)blockIdx.x * kPpoSums + tid] = acc;
}

// The four coefficients of one update: the call's (PpoDev), or a member's row of member_coef [P, 4], read where the kernels use them
struct PpoCoef {
    float clip, clip_vf, ent_coef, vf_coef;
};
__device__ __forceinline__ PpoCoef ppo_coef(const PpoDev &q) { return PpoCoef{q.clip, q.clip_vf, q.ent_coef, q.vf_coef}; }
// (uniform over the workgroup: four scalar loads.)  The values are not checked: NaN or <= 0 in clip_vf turns value clipping off by the comparison
__device__ __forceinline__ PpoCoef ppo_member_coef(const PpoDev &q, const float *__restrict__ member_coef, int m) {
    if (!member_coef) return ppo_coef(q);
    const float *c = member_coef + 4 * (size_t)m;
    return PpoCoef{c[0], c[1], c[2], c[3]};
}

// ppo_grad_kernel for member blockIdx.y: gridDim.x workgroups (population_grad_plan's) take the tiles blockIdx.x, + gridDim.x, ... of
// the member's n minibatch entries -- entries member x n + local of index and of the per-row outputs -- and leave their partial sums in
// ws[m][blockIdx.x][parameter], their statistics sums in sums[m][blockIdx.x][8].  With gridDim.x = min(ceil(n / R), 256) and
// q.adv_groups = min(ceil(n / 1024), 256) this is ppo_grad_kernel's grouping of the member's n entries, bit for bit.
// The frame is ppo_grad_kernel's, line by line, over the same device functions with the member handed on, and the four coefficients
// taken from c.  (One body shared by both kernels, `member` defaulting to 0, was built first: it changed ppo_grad_kernel's register
// allocation, so that kernel keeps its text: DESIGN section 25.)
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void ppo_population_grad_kernel(PolicyDev p, PpoDev q, const float *__restrict__ member_coef,
                                                                                    int n, const float *__restrict__ obs,
                                                                                    const void *__restrict__ action, PolicyGradLayout lay,
                                                                                    float *__restrict__ ws, const double *__restrict__ adv_all,
                                                                                    float *__restrict__ sums_all) {
    extern __shared__ __attribute__((aligned(16))) float sg_policy_lds[];
    const int R = (int)blockDim.x, S = R + 2, tid = (int)threadIdx.x, tiles = (int)(((int64_t)n + R - 1) / R), member = (int)blockIdx.y;
    const size_t group = (size_t)member * gridDim.x + blockIdx.x;
    float *wt = sg_policy_lds;
    float *bs = wt + (size_t)max(max(p.hidden, p.obs_dim), kPolicyHeadPad) * (kPolicyGradChunk + kPolicyRowPad);
    float *store = bs + kPolicyGradChunk;
    float *part = ws + group * lay.total;
    float *sums = sums_all + group * kPpoSums;
    const double *adv_part = adv_all + 2 * (size_t)member * q.adv_groups;
    const PpoCoef c = ppo_member_coef(q, member_coef, member);
    const bool critic = p.critic.w[0] != nullptr;
    const int64_t base = (int64_t)member * n;
    const float *log_std = p.log_std + (size_t)member * kPolicyActDim;
    const float nf = (float)n, ge_row = -c.ent_coef / nf;
    float mean = 0.0f, rstd = 1.0f, sd = 0.0f;
    if (q.normalize) ppo_adv_finish(q, adv_part, n, mean, rstd, sd);
    const float lo = 1.0f - c.clip, hi = 1.0f + c.clip;
    float acc = 0.0f;  // lane s < kPpoSums: this workgroup's sum s over its rows, in row order
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {  // (uniform over the workgroup)
        const int64_t local = (int64_t)tile * R + tid;
        const bool live = local < n;
        const int64_t at = base + local;
        bool good;
        const int64_t r = ppo_row(q, live ? at : base + n - 1, good);  // idle lanes of the last tile redo its last row with zero loss gradients
        const bool on = live && good;
        const float *obs_row = obs + (size_t)r * p.obs_dim;
        float c_sum[kPpoSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, live && !good ? 1.0f : 0.0f, 0.0f};
        float no_dx[kPolicyActDim];  // (no gradient by the input row here)
        if (critic) {
            policy_grad_net<NT>(p, 1, 1, 0, obs_row, nullptr, [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
                const float value = out[0], d = value - q.ret[r];
                float vl = 0.5f * (d * d), gv = c.vf_coef * d / nf;
                if (c.clip_vf > 0.0f) {
                    const float ov = q.old_value[r], dv = value - ov;
                    const float e2 = (ov + fminf(fmaxf(dv, -c.clip_vf), c.clip_vf)) - q.ret[r];
                    if (!(d * d >= e2 * e2)) {
                        vl = 0.5f * (e2 * e2);
                        gv = dv >= -c.clip_vf && dv <= c.clip_vf ? c.vf_coef * e2 / nf : 0.0f;
                    }
                }
                if (!on) gv = 0.0f;
                c_sum[1] = on ? vl : 0.0f;
                if (live && q.row_value) q.row_value[at] = value;
                if (live && q.row_g_value) q.row_g_value[at] = gv;
#pragma unroll
                for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
                dz[0] = gv;
            }, lay, part, first, true, false, no_dx, wt, bs, store, member);
        }
        policy_grad_net<NT>(p, 0, p.head, p.discrete ? 0 : kPolicyActDim, obs_row, nullptr,
                            [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
            PolicyScore s;
            policy_score(p, log_std, out, action, (int)r, 0.0f, 0.0f, false, s);
            const float lr = s.logp - q.old_logp[r], ratio = expf(lr);
            const float A = q.normalize ? (q.adv[r] - mean) * rstd : q.adv[r];
            const float t1 = -A * ratio, t2 = -A * fminf(fmaxf(ratio, lo), hi);
            const float gl = on && t1 >= t2 ? t1 / nf : 0.0f;
            if (on) {
                c_sum[0] = t1 >= t2 ? t1 : t2;
                c_sum[2] = s.entropy;
                c_sum[3] = (ratio - 1.0f) - lr;
                c_sum[4] = -lr;
                c_sum[5] = fabsf(ratio - 1.0f) > c.clip ? 1.0f : 0.0f;
            }
            if (live && q.row_logp) q.row_logp[at] = s.logp;
            if (live && q.row_g_logp) q.row_g_logp[at] = gl;
            policy_score(p, log_std, out, action, (int)r, gl, on ? ge_row : 0.0f, true, s);
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = s.dz[j];
        }, lay, part, first, true, false, no_dx, wt, bs, store, member);
        first = false;
        // the statistics of the tile: each row's terms to the store (free once every wave has left the actor's walk), lane s adds sum s
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kPpoSums; s++) store[(size_t)s * S + tid] = c_sum[s];
        __syncthreads();
        if (tid < kPpoSums) {
            const float *col = store + (size_t)tid * S;
            for (int k = 0; k < R; k++) acc += col[k];
        }
    }
    if (tid < kPpoSums) sums[tid] = acc;
}

// One net's statistics: the workgroups' sums added in workgroup order by lanes 0 .. 7, then stats [kPpoStats] by lane 0 (the whole
// workgroup calls this)
__device__ __forceinline__ void ppo_stats_finish(const PpoDev &q, const PpoCoef c, const float *__restrict__ sums, int parts,
                                                 const double *__restrict__ adv_part, int n, int critic, float *__restrict__ stats) {
    __shared__ float tot[kPpoSums];
    const int t = (int)threadIdx.x;
    if (t < kPpoSums) {
        float sum = sums[t];
        for (int g = 1; g < parts; g++) sum += sums[(size_t)g * kPpoSums + t];
        tot[t] = sum;
    }
    __syncthreads();
    if (t != 0) return;
    const float nf = (float)n, ent_coef = c.ent_coef, vf_coef = c.vf_coef;
    float mean = 0.0f, rstd = 1.0f, sd = 0.0f;
    if (q.normalize) ppo_adv_finish(q, adv_part, n, mean, rstd, sd);
    const float pg = tot[0] / nf, vl = critic ? tot[1] / nf : 0.0f, ent = tot[2] / nf;
    stats[0] = critic ? (pg - ent_coef * ent) + vf_coef * vl : pg - ent_coef * ent;
    stats[1] = pg;
    stats[2] = vl;
    stats[3] = ent;
    stats[4] = tot[3] / nf;
    stats[5] = tot[4] / nf;
    stats[6] = tot[5] / nf;
    stats[7] = mean;
    stats[8] = sd;
    stats[9] = tot[6];
    stats[10] = 0.0f;
    stats[11] = 0.0f;
}

// policy_grad_reduce_kernel, and one workgroup more: the statistics partials added in workgroup order, then stats_out [kPpoStats]
__global__ __launch_bounds__(256) void ppo_reduce_kernel(const float *__restrict__ ws, int parts, int total, PolicyGradOut o,
                                                         PpoDev q, const float *__restrict__ sums, const double *__restrict__ adv_part, int n,
                                                         int critic, float *__restrict__ stats) {
    if (blockIdx.x + 1 < gridDim.x) {
        const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        if (e < total) policy_grad_reduce_element(ws, parts, total, o, e, 0);
        return;
    }
    ppo_stats_finish(q, ppo_coef(q), sums, parts, adv_part, n, critic, stats);
}

// ppo_reduce_kernel for member blockIdx.y: its partials ws[m][0 .. parts) into slice m of the stacked gradient tensors, and the one
// statistics workgroup of the member, which writes stats[m][0 .. 12)
__global__ __launch_bounds__(256) void ppo_population_reduce_kernel(const float *__restrict__ ws, int parts, int total, PolicyGradOut o,
                                                                    PpoDev q, const float *__restrict__ member_coef,
                                                                    const float *__restrict__ sums, const double *__restrict__ adv_part, int n,
                                                                    int critic, float *__restrict__ stats) {
    const int m = (int)blockIdx.y;
    if (blockIdx.x + 1 < gridDim.x) {
        const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        if (e < total) policy_grad_reduce_element(ws + (size_t)m * parts * total, parts, total, o, e, m);
        return;
    }
    ppo_stats_finish(q, ppo_member_coef(q, member_coef, m), sums + (size_t)m * parts * kPpoSums, parts, adv_part + 2 * (size_t)m * q.adv_groups, n,
                     critic, stats + (size_t)m * kPpoStats);
}

