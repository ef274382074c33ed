// Log-prob, entropy and value of GIVEN actions, and their gradients with respect to the parameters (sg_policy_evaluate_device /
// sg_policy_grad_device; DESIGN section 18): what a PPO / A2C learner's minibatch update needs around its own loss.
//     continuous: z_d = (a_d - mean_d) exp(-log_std_d);  logp = sum_d(-z_d^2 / 2 - log_std_d - ln(2 pi) / 2);  entropy = sum_d log_std_d + 1 + ln(2 pi)
//                 d logp / d mean_d = z_d / sigma_d,  d logp / d log_std_d = z_d^2 - 1,  d entropy / d log_std_d = 1
//     discrete:   logp = (logit_a - max) - log(total), as policy_act_kernel;  entropy H = -sum_j p_j log p_j
//                 d logp / d logit_j = [j = a] - p_j,  d entropy / d logit_j = -p_j (log p_j + H)
//     tanh' = 1 - h^2 of the stored activation; relu' = [pre-activation > 0] = [h > 0]: 0 at 0, as torch.
// tests/policy_grad_model.py states the same in NumPy.
//
// The evaluate kernel is policy_act_kernel's forward (policy_net) with another tail: value and the discrete logp are the act
// kernel's own arithmetic, bit for bit.
//
// The grad kernel: a workgroup of R lanes takes row tiles of R rows, tile = blockIdx.x, + gridDim.x, ... (the grid is capped, so a
// row's workgroup and position are a function of n alone), one lane per row.  Per net it
//   1. recomputes the forward pass with policy_stage / policy_layer in chunks of 32 outputs, keeping every layer's activations in the
//      lane's LDS column (store[row k][lane], row stride S = R + 2);
//   2. walks the layers from the head down: dz of the layer's outputs goes to LDS (for the hidden layers IN PLACE of the layer's
//      activations, which are not needed once dz = dh * f'(h) is formed); dW[j][k] = sum_rows dz[j] h[k] and db[j] = sum_rows dz[j]
//      are one [J x R] . [R x (in + 1)] product with the rows as the contraction dimension, done with v_mfma_f32_32x32x2_f32
//      (exact float32, rows in ascending order; the bias is column `in`, whose operand is the constant 1); then dh = W^T dz is
//      policy_layer again over the untransposed weights.
// The MFMA operands are read across the lanes' columns: lane l takes store[j0 + (l & 31)][r + (l >> 5)]; with S = 2 (mod 64)
// the 64 addresses fall on 64 different banks.  A 32 x 32 accumulator tile starts from the workgroup's partial sums of its earlier row
// tiles (zero for the first) and goes back to them: ws[blockIdx.x][parameter], loaded and stored by the same lane, so no
// accumulator has to live across the forward pass of the next tile.  The continuous head carries two more rows, 2 and 3, whose
// "dz" is the row's d loss / d log_std_d: their bias column is the log_std gradient.
// policy_grad_reduce_kernel then adds the partials of a parameter in workgroup order.  No atomics anywhere: the same inputs and the
// same n give the same bits; another n groups the rows differently.
constexpr int kPolicyGradMaxGroups = 256;  // the grid cap: one workgroup per CU of an MI355X; bounds the workspace
constexpr int kPolicyGradChunk = 32, kPolicyGradSegs = 2 * 2 * (kPolicyMaxHiddenLayers + 1) + 1;

constexpr int policy_grad_block(int nt) { return nt <= 1 ? 256 : nt == 2 ? 128 : 64; }  // rows per tile: see policy_grad_lds_bytes

// Offsets (floats) of every parameter in a workgroup's partial sums: actor w0 b0 w1 b1 ..., critic the same, log_std [2]
struct PolicyGradLayout {
    int w[2][kPolicyMaxHiddenLayers + 1], b[2][kPolicyMaxHiddenLayers + 1];
    int log_std, total;
};
// Where the sums go: segment s covers partial offsets [off[s], off[s + 1]); dst NULL: not wanted; zero: written with 0 (not computed)
struct PolicyGradOut {
    float *dst[kPolicyGradSegs];
    int off[kPolicyGradSegs + 1];
    int zero[kPolicyGradSegs];
    int count;
};

static inline int policy_grad_store_rows(int n_hidden, int hidden, int obs_dim) { return obs_dim + n_hidden * hidden + kPolicyHeadPad; }
static inline int policy_grad_wt_rows(int hidden, int obs_dim) { return std::max(std::max(hidden, obs_dim), kPolicyHeadPad); }
// LDS of one workgroup: a staged chunk (rows of 32 + pad floats), its bias, and per lane the observation, every hidden layer and the head's dz
static inline size_t policy_grad_lds_bytes(int nt, int n_hidden, int hidden, int obs_dim) {
    return sizeof(float) * ((size_t)policy_grad_wt_rows(hidden, obs_dim) * (kPolicyGradChunk + kPolicyRowPad) + kPolicyGradChunk +
                            (size_t)policy_grad_store_rows(n_hidden, hidden, obs_dim) * (policy_grad_block(nt) + 2));
}

// The scores of one row from its head outputs.  Discrete: exactly policy_act_kernel's expressions.
struct PolicyScore {
    float logp, entropy;
    float dz[kPolicyHeadPad];  // d (g_logp logp + g_entropy entropy) / d head output j; continuous: [2 + d] = the same by log_std_d
};
// log_std: the row's policy's (a population member's slice)
__device__ __forceinline__ void policy_score(const PolicyDev &p, const float *__restrict__ log_std, const float (&out)[kPolicyHeadPad],
                                             const void *__restrict__ action, int i, float gl, float ge, bool want_grad, PolicyScore &s) {
#pragma unroll
    for (int j = 0; j < kPolicyHeadPad; j++) s.dz[j] = 0.0f;
    if (p.discrete) {
        const int a = static_cast<const int32_t *>(action)[i];
        float mx = out[0];
#pragma unroll
        for (int j = 1; j < kPolicyDiscreteActions; j++)
            if (out[j] > mx) mx = out[j];
        float pr[kPolicyDiscreteActions], total = 0.0f;
#pragma unroll
        for (int j = 0; j < kPolicyDiscreteActions; j++) { pr[j] = expf(out[j] - mx); total += pr[j]; }
        float la = out[0];
#pragma unroll
        for (int j = 1; j < kPolicyDiscreteActions; j++) la = a == j ? out[j] : la;  // selected by comparison: a bad action indexes nothing
        const float lt = logf(total);
        s.logp = (la - mx) - lt;
        float H = 0.0f, lpj[kPolicyDiscreteActions], pj[kPolicyDiscreteActions];
#pragma unroll
        for (int j = 0; j < kPolicyDiscreteActions; j++) {
            pj[j] = pr[j] / total;
            lpj[j] = (out[j] - mx) - lt;
            H -= pj[j] * lpj[j];
        }
        s.entropy = H;
        if (want_grad) {
#pragma unroll
            for (int j = 0; j < kPolicyDiscreteActions; j++)
                s.dz[j] = gl * ((a == j ? 1.0f : 0.0f) - pj[j]) - ge * pj[j] * (lpj[j] + H);
        }
    } else {
        const float2 a2 = reinterpret_cast<const float2 *>(action)[i];
        const float a[kPolicyActDim] = {a2.x, a2.y};
        float lp = 0.0f, ent = 2.8378770664093453f;  // 1 + ln(2 pi)
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) {
            const float ls = log_std[d], inv = expf(-ls), z = (a[d] - out[d]) * inv;
            lp += (-0.5f * z * z - ls) - 0.9189385332046727f;
            ent += ls;
            if (want_grad) {
                s.dz[d] = gl * z * inv;
                s.dz[kPolicyActDim + d] = gl * (z * z - 1.0f) + ge;
            }
        }
        s.logp = lp;
        s.entropy = ent;
    }
}

template <int NT>
__global__ __launch_bounds__(policy_block(NT)) void policy_evaluate_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                           const void *__restrict__ action, float *__restrict__ logp_out,
                                                                           float *__restrict__ entropy_out, float *__restrict__ value_out) {
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
    if (value_out) {
        policy_net<NT>(p, p.critic, 1, obs_row, wt, bs, h, out);
        if (live) value_out[i] = out[0];
    }
    if (!logp_out && !entropy_out) return;
    policy_net<NT>(p, p.actor, p.head, obs_row, wt, bs, h, out);
    if (!live) return;
    PolicyScore s;
    policy_score(p, p.log_std, out, action, i, 0.0f, 0.0f, false, s);
    if (logp_out) logp_out[i] = s.logp;
    if (entropy_out) entropy_out[i] = s.entropy;
}

// ws[j][k] = W[j][k0 + k] (k0 + k < in, j < out; else 0) for k < J, bs = 0: the weights as policy_layer<J> wants them for dh = W^T dz
template <int J>
__device__ __forceinline__ void policy_stage_plain(float *__restrict__ ws, float *__restrict__ bs, const float *__restrict__ W, int in, int out,
                                                   int k0) {
    __syncthreads();
    for (int idx = (int)threadIdx.x; idx < out * J; idx += (int)blockDim.x) {
        const int j = idx / J, k = idx % J;  // (J is a power of two)
        ws[j * (J + kPolicyRowPad) + k] = k0 + k < in ? W[(size_t)j * in + k0 + k] : 0.0f;
    }
    if (threadIdx.x < J) bs[threadIdx.x] = 0.0f;
    __syncthreads();
}

typedef float policy_f32x16 __attribute__((ext_vector_type(16)));

// part[w .. ] += dz^T [h | 1] over the R rows of the tile: dz rows j < n_j at dz[j * S + row], h rows k < in at h[k * S + row].
// Tile t of the (n_j / 32) x ((in + 1) / 32) tiles (rounded up) belongs to wave t mod waves, the same in every pass, and its
// element (j, k) to one lane: k < in the weight, k = in the bias, and for extra rows (j >= out, continuous head) the bias alone.
__device__ __forceinline__ void policy_grad_weights(const float *__restrict__ dz, const float *__restrict__ h, int S, int R, int out, int n_j,
                                                    int in, float *__restrict__ pw, float *__restrict__ pb, float *__restrict__ pextra,
                                                    bool first) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, waves = R >> 6;
    const int KT = (in + 1 + 31) >> 5, JT = (n_j + 31) >> 5;
    const int half = lane >> 5, l31 = lane & 31;
    for (int t = wave; t < JT * KT; t += waves) {
        const int j0 = (t / KT) << 5, k0 = (t % KT) << 5;
        const int k = k0 + l31;
        policy_f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float v = 0.0f;
            if (!first) {
                if (j < out) { if (k < in) v = pw[(size_t)j * in + k]; else if (k == in) v = pb[j]; }
                else if (j < n_j && k == in) v = pextra[j - out];
            }
            c[r] = v;
        }
        const int ja = j0 + l31;
        const bool a_on = ja < n_j, b_on = k < in;
        const float *ap = dz + (size_t)(a_on ? ja : 0) * S + half;
        const float *bp = h + (size_t)(b_on ? k : 0) * S + half;
        const float b_const = k == in ? 1.0f : 0.0f;
#pragma unroll 4
        for (int r = 0; r < R; r += 2) {
            const float a = a_on ? ap[r] : 0.0f;
            const float b = b_on ? bp[r] : b_const;
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (j < out) { if (k < in) pw[(size_t)j * in + k] = c[r]; else if (k == in) pb[j] = c[r]; }
            else if (j < n_j && k == in) pextra[j - out] = c[r];
        }
    }
}

// One net of a row tile: forward into the store, then the walk down.
//   which    0 the actor, 1 the critic (sg_qnet.inc: critic 0 / 1): the net and its offsets in `lay`;  head: its outputs
//   extra    rows of the head's dz past `head` whose bias column is a sum of its own (the continuous actor: 2, d loss / d log_std_d)
//   tail     NULL, or the row's action: the last kPolicyActDim of the p.obs_dim inputs (obs_row holds the others)
//   head_dz  (head outputs, dz [kPolicyHeadPad]): fills this row's dz of the head's outputs and extra rows, zeros elsewhere (zeros
//            altogether for the idle lanes of the last tile)
//   weights  false: the parameters' sums are not wanted, no MFMA runs and `part` is not touched
//   want_dx  dx receives W0[:, in - 2 .. in)^T dz0, this row's gradient by the tail (else dx is left as it is)
//   member   (sg_population.inc) the net's tensors are stacked [members, ...]: member `member`'s slice of each, at member x numel(tensor)
template <int NT, typename HeadDz>
__device__ __forceinline__ void policy_grad_net(const PolicyDev &p, int which, int head, int extra, const float *__restrict__ obs_row,
                                                const float *__restrict__ tail, HeadDz head_dz, const PolicyGradLayout &lay,
                                                float *__restrict__ part, bool first, bool weights, bool want_dx, float (&dx)[kPolicyActDim], float *wt,
                                                float *bs, float *store, int member = 0) {
    constexpr int C = kPolicyGradChunk;
    const PolicyNet &net = which ? p.critic : p.actor;
    const int R = (int)blockDim.x, S = R + 2, tid = (int)threadIdx.x, D = p.obs_dim, H = p.hidden, L = p.n_hidden;
    const size_t M = (size_t)member;
    const auto w_of = [&](int l) { return net.w[l] + M * (l == L ? head : H) * (l == 0 ? D : H); };
    const auto b_of = [&](int l) { return net.b[l] + M * (l == L ? head : H); };
    const int from_obs = tail ? D - kPolicyActDim : D;
    __syncthreads();  // the store is free: every wave has finished the net before
    for (int k = 0; k < from_obs; k++) store[(size_t)k * S + tid] = obs_row[k];
    if (tail) {
#pragma unroll
        for (int d = 0; d < kPolicyActDim; d++) store[(size_t)(from_obs + d) * S + tid] = tail[d];
    }
    // rows of the store: [0, D) the input row, [D + l H, D + (l + 1) H) hidden layer l, then kPolicyHeadPad rows for the head's dz
    int in = D;
    const float *hin = store + tid;
    for (int l = 0; l < L; l++) {
        float *hout = store + (size_t)(D + l * H) * S + tid;
#pragma unroll
        for (int c = 0; c < NT; c++) {
            if (c * C >= H) break;  // (uniform)
            policy_stage<C>(wt, bs, w_of(l) + (size_t)c * C * in, b_of(l) + c * C, in, H - c * C);
            float acc[C];
            policy_layer<C>(wt, bs, hin, S, in, acc);
#pragma unroll
            for (int j = 0; j < C; j++)
                if (c * C + j < H) hout[(size_t)(c * C + j) * S] = p.relu ? (acc[j] < 0.0f ? 0.0f : acc[j]) : policy_tanh(acc[j]);
        }
        hin = hout;
        in = H;
    }
    float out[kPolicyHeadPad], dz_head[kPolicyHeadPad];
    policy_stage<kPolicyHeadPad>(wt, bs, w_of(L), b_of(L), in, head);
    policy_layer<kPolicyHeadPad>(wt, bs, hin, S, in, out);
    head_dz(out, dz_head);
    float *hd = store + (size_t)(D + L * H) * S;
#pragma unroll
    for (int j = 0; j < kPolicyHeadPad; j++) hd[(size_t)j * S + tid] = dz_head[j];
    for (int l = L; l >= 0; l--) {
        const int out_l = l == L ? head : H, in_l = l == 0 ? D : H;
        const float *dz = l == L ? hd : store + (size_t)(D + l * H) * S;
        float *hprev = l == 0 ? store : store + (size_t)(D + (l - 1) * H) * S;
        __syncthreads();  // dz of every row of the tile is in LDS
        if (weights)
            policy_grad_weights(dz, hprev, S, R, out_l, out_l + (l == L ? extra : 0), in_l, part + lay.w[which][l], part + lay.b[which][l],
                                part + lay.log_std, first);
        if (l == 0) {
            if (want_dx) {  // one step further, for the tail's two columns of W0 only (out_l = H rows of the staging area: it holds max(H, D))
                constexpr int A = 4;  // kPolicyActDim padded to policy_layer's four outputs
                policy_stage_plain<A>(wt, bs, w_of(0), in_l, out_l, in_l - kPolicyActDim);
                float acc[A];
                policy_layer<A>(wt, bs, dz + tid, S, out_l, acc);
#pragma unroll
                for (int d = 0; d < kPolicyActDim; d++) dx[d] = acc[d];
            }
            break;
        }
#pragma unroll
        for (int c = 0; c < NT; c++) {
            if (c * C >= in_l) break;  // (uniform)
            policy_stage_plain<C>(wt, bs, w_of(l), in_l, out_l, c * C);  // (its first barrier: every wave is past the MFMA reads of hprev)
            float acc[C];
            policy_layer<C>(wt, bs, dz + tid, S, out_l, acc);
#pragma unroll
            for (int k = 0; k < C; k++) {
                if (c * C + k < in_l) {
                    float *hp = hprev + (size_t)(c * C + k) * S + tid;
                    const float hv = *hp;
                    *hp = acc[k] * (p.relu ? (hv > 0.0f ? 1.0f : 0.0f) : 1.0f - hv * hv);
                }
            }
        }
    }
}

// flags: 2 the critic (g_value given)
template <int NT>
__global__ __launch_bounds__(policy_grad_block(NT)) void policy_grad_kernel(PolicyDev p, int n, const float *__restrict__ obs,
                                                                            const void *__restrict__ action, const float *__restrict__ g_logp,
                                                                            const float *__restrict__ g_entropy, const float *__restrict__ g_value,
                                                                            PolicyGradLayout lay, float *__restrict__ ws) {
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
        const int row = live ? i : n - 1;  // idle lanes of the last tile redo its last row with zero loss gradients
        const float *obs_row = obs + (size_t)row * p.obs_dim;
        const float gl = live && g_logp ? g_logp[i] : 0.0f, ge = live && g_entropy ? g_entropy[i] : 0.0f;
        float no_dx[kPolicyActDim];  // (no gradient by the input row here)
        if (g_value) {
            const float gv = live ? g_value[i] : 0.0f;
            policy_grad_net<NT>(p, 1, 1, 0, obs_row, nullptr, [&](const float (&)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
#pragma unroll
                for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = 0.0f;
                dz[0] = gv;
            }, lay, part, first, true, false, no_dx, wt, bs, store);
        }
        policy_grad_net<NT>(p, 0, p.head, p.discrete ? 0 : kPolicyActDim, obs_row, nullptr,
                            [&](const float (&out)[kPolicyHeadPad], float (&dz)[kPolicyHeadPad]) {
            PolicyScore s;
            policy_score(p, p.log_std, out, action, row, gl, ge, true, s);
#pragma unroll
            for (int j = 0; j < kPolicyHeadPad; j++) dz[j] = s.dz[j];
        }, lay, part, first, true, false, no_dx, wt, bs, store);
        first = false;
    }
}

// Element e of the partial sums ws[parts][total], added in workgroup order, to its place in the segment's tensor; member (sg_population.inc):
// the tensors are stacked [members, ...] and this is member `member`'s slice
__device__ __forceinline__ void policy_grad_reduce_element(const float *__restrict__ ws, int parts, int total, const PolicyGradOut &o, int e,
                                                           int member) {
    int s = 0;
    while (s + 1 < o.count && e >= o.off[s + 1]) s++;
    if (!o.dst[s]) return;
    float sum = 0.0f;
    if (!o.zero[s]) {
        sum = ws[e];
        for (int g = 1; g < parts; g++) sum += ws[(size_t)g * total + e];
    }
    o.dst[s][(size_t)member * (o.off[s + 1] - o.off[s]) + (e - o.off[s])] = sum;
}

// grads[e] = ws[0][e] + ws[1][e] + ... in workgroup order
__global__ __launch_bounds__(256) void policy_grad_reduce_kernel(const float *__restrict__ ws, int parts, int total, PolicyGradOut o) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= total) return;
    policy_grad_reduce_element(ws, parts, total, o, e, 0);
}
