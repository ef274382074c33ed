// Per-member Adam / AdamW step with global-norm gradient clipping, and the PBT exploit copy (sg_adam_step_device /
// sg_adam_exploit_device; DESIGN section 26).  tests/adam_model.py states every operation and its order in NumPy; the kernels follow
// it so that parameters, moments and the state row come out with the same bits.
//
// Two launches.  adam_prepare_kernel, one workgroup per member: lane l accumulates the float64 squares of elements l, l + 1024, ...
// of the member's slice of table entry 0, then of entry 1, ...; a fixed LDS tree (part[i] += part[i + s], s = 512 .. 1) finishes the
// sum; lane 0 forms the norm, the clip scale, the skip decision, the new beta powers and step_size and writes the member's state row.
// adam_update_kernel, grid (element blocks, table entry, member): reads the member's state and hyper rows -- nothing that its own
// launch writes -- returns at once for a skipped member, and updates its elements.  Every float32 operation is rounded on its own
// (__fmul_rn / __fadd_rn / __fsub_rn: nothing contracts); sqrtf and / are the correctly rounded sequences.  No atomics.
//
// Member slices of small tensors (log_std [P, 2], head biases of 1, 2 or 6) are not 16-byte aligned: a table entry takes the
// four-wide path only when numel % 4 == 0 and all four bases are 16-byte aligned (wave-uniform), else one element per access.
constexpr int kAdamMaxTensors = 32;
constexpr int kAdamPrepareBlock = 1024;
constexpr int kAdamBlock = 256;
constexpr int kAdamPerLane = 4;                                  // elements per lane of the update and exploit kernels
constexpr int kAdamTile = kAdamBlock * kAdamPerLane;            // elements per workgroup
enum AdamHyper { kAdamLr = 0, kAdamBeta1, kAdamBeta2, kAdamEps, kAdamWeightDecay, kAdamMaxGradNorm, kAdamHyperCols = 8 };
enum AdamStateCol { kAdamSteps = 0, kAdamBeta1Pow, kAdamBeta2Pow, kAdamSkipped, kAdamGradNorm, kAdamClipScale, kAdamStepSize, kAdamApplied,
                    kAdamStateCols = 8 };

struct AdamTable {  // by value, as a kernel argument
    sg_adam_tensor t[kAdamMaxTensors];
};

__global__ __launch_bounds__(kAdamPrepareBlock) void adam_prepare_kernel(int n_tensors, AdamTable tab, const float *__restrict__ hyper,
                                                                         double *__restrict__ state) {
    __shared__ double part[kAdamPrepareBlock];
    const int m = (int)blockIdx.x, lane = (int)threadIdx.x;
    double acc = 0.0;
    for (int k = 0; k < n_tensors; k++) {
        const size_t n = (size_t)tab.t[k].numel;
        const float *g = tab.t[k].grad + (size_t)m * n;
        for (size_t i = (size_t)lane; i < n; i += kAdamPrepareBlock) {
            const double x = (double)g[i];
            acc = __dadd_rn(acc, __dmul_rn(x, x));  // (the square of a float32 is exact in float64)
        }
    }
    part[lane] = acc;
    __syncthreads();
    for (int s = kAdamPrepareBlock / 2; s > 0; s >>= 1) {
        if (lane < s) part[lane] = __dadd_rn(part[lane], part[lane + s]);
        __syncthreads();
    }
    if (lane != 0) return;
    const float *h = hyper + (size_t)m * kAdamHyperCols;
    double *st = state + (size_t)m * kAdamStateCols;
    const float norm = (float)sqrt(part[0]);
    st[kAdamGradNorm] = (double)norm;
    if (!(fabsf(norm) < INFINITY)) {  // an inf or NaN anywhere in the member's gradient: the step is skipped
        st[kAdamSkipped] = __dadd_rn(st[kAdamSkipped], 1.0);
        st[kAdamClipScale] = 0.0;
        st[kAdamStepSize] = 0.0;
        st[kAdamApplied] = 0.0;
        return;
    }
    const float max_norm = h[kAdamMaxGradNorm];
    float scale = 1.0f;  // 0, negative, inf, NaN: no clipping, by the comparison
    if (max_norm > 0.0f && max_norm < INFINITY) {
        const double coef = (double)max_norm / __dadd_rn((double)norm, 1e-6);
        scale = (float)(coef < 1.0 ? coef : 1.0);
    }
    const double b1p = __dmul_rn(st[kAdamBeta1Pow], (double)h[kAdamBeta1]);
    const double b2p = __dmul_rn(st[kAdamBeta2Pow], (double)h[kAdamBeta2]);
    const double bc1 = __dsub_rn(1.0, b1p);
    const float step_size = (float)((double)h[kAdamLr] / bc1);
    st[kAdamSteps] = __dadd_rn(st[kAdamSteps], 1.0);
    st[kAdamBeta1Pow] = b1p;
    st[kAdamBeta2Pow] = b2p;
    st[kAdamClipScale] = (double)scale;
    st[kAdamStepSize] = (double)step_size;
    st[kAdamApplied] = 1.0;
}

struct AdamMember {  // what the update needs of a member: wave-uniform
    float scale, b1, omb1, b2, omb2, eps, lrwd, step_size, bc2s;
};

__device__ __forceinline__ void adam_element(float g, float &p, float &m, float &v, const AdamMember &c) {
    const float g1 = __fmul_rn(g, c.scale);
    m = __fadd_rn(__fmul_rn(c.b1, m), __fmul_rn(c.omb1, g1));
    v = __fadd_rn(__fmul_rn(c.b2, v), __fmul_rn(__fmul_rn(c.omb2, g1), g1));
    const float root = sqrtf(v);
    const float scaled = root / c.bc2s;
    const float den = __fadd_rn(scaled, c.eps);
    const float decayed = __fsub_rn(p, __fmul_rn(c.lrwd, p));
    const float num = __fmul_rn(c.step_size, m);
    const float delta = num / den;
    p = __fsub_rn(decayed, delta);
}

__global__ __launch_bounds__(kAdamBlock) void adam_update_kernel(AdamTable tab, const float *__restrict__ hyper,
                                                                 const double *__restrict__ state) {
    const int k = (int)blockIdx.y, mem = (int)blockIdx.z;
    const size_t n = (size_t)tab.t[k].numel;
    const size_t first = (size_t)blockIdx.x * kAdamTile;
    if (first >= n) return;
    const double *st = state + (size_t)mem * kAdamStateCols;
    if (st[kAdamApplied] == 0.0) return;
    const float *h = hyper + (size_t)mem * kAdamHyperCols;
    AdamMember c;
    c.scale = (float)st[kAdamClipScale];
    c.step_size = (float)st[kAdamStepSize];
    const double bc2 = __dsub_rn(1.0, st[kAdamBeta2Pow]);
    c.bc2s = (float)sqrt(bc2);
    c.b1 = h[kAdamBeta1];
    c.b2 = h[kAdamBeta2];
    c.omb1 = __fsub_rn(1.0f, c.b1);
    c.omb2 = __fsub_rn(1.0f, c.b2);
    c.eps = h[kAdamEps];
    c.lrwd = __fmul_rn(h[kAdamLr], h[kAdamWeightDecay]);
    const size_t base = (size_t)mem * n;
    float *p = tab.t[k].param + base, *ea = tab.t[k].exp_avg + base, *es = tab.t[k].exp_avg_sq + base;
    const float *g = tab.t[k].grad + base;
    const bool wide = n % 4 == 0 && (((uintptr_t)tab.t[k].param | (uintptr_t)tab.t[k].grad | (uintptr_t)tab.t[k].exp_avg |
                                      (uintptr_t)tab.t[k].exp_avg_sq) & 15u) == 0;
    if (wide) {  // (then every member's slice is 16-byte aligned too)
        const size_t i = first + (size_t)threadIdx.x * kAdamPerLane;
        if (i >= n) return;
        const float4 g4 = *reinterpret_cast<const float4 *>(g + i);
        float4 p4 = *reinterpret_cast<float4 *>(p + i), m4 = *reinterpret_cast<float4 *>(ea + i), v4 = *reinterpret_cast<float4 *>(es + i);
        adam_element(g4.x, p4.x, m4.x, v4.x, c);
        adam_element(g4.y, p4.y, m4.y, v4.y, c);
        adam_element(g4.z, p4.z, m4.z, v4.z, c);
        adam_element(g4.w, p4.w, m4.w, v4.w, c);
        *reinterpret_cast<float4 *>(p + i) = p4;
        *reinterpret_cast<float4 *>(ea + i) = m4;
        *reinterpret_cast<float4 *>(es + i) = v4;
        return;
    }
#pragma unroll
    for (int j = 0; j < kAdamPerLane; j++) {
        const size_t i = first + (size_t)j * kAdamBlock + threadIdx.x;
        if (i < n) {
            float pv = p[i], mv = ea[i], vv = es[i];
            adam_element(g[i], pv, mv, vv, c);
            p[i] = pv;
            ea[i] = mv;
            es[i] = vv;
        }
    }
}

// PBT exploit: member m's parameter and moment slices and columns 0 .. 3 of its state row become member src[m]'s.  A copy is
// performed only if src[m] is in [0, members), differs from m and is not itself a destination (src[src[m]] == src[m]): then no
// workgroup of the launch reads what another writes.  The test comes before any address is formed from src[m].
__device__ __forceinline__ bool adam_exploit_source(const int32_t *__restrict__ src, int members, int m, int &from) {
    const int s = src[m];
    from = s;
    if (s == m) return false;
    if (s < 0 || s >= members) return false;
    return src[s] == s;
}

__global__ __launch_bounds__(kAdamBlock) void adam_exploit_kernel(int members, AdamTable tab, double *__restrict__ state,
                                                                  const int32_t *__restrict__ src, int32_t *__restrict__ refused_out) {
    const int k = (int)blockIdx.y, mem = (int)blockIdx.z;
    if (refused_out && blockIdx.x == 0 && k == 0 && mem == 0) {  // one workgroup counts the refused copies, in a fixed order
        __shared__ int count[kAdamBlock];
        int c = 0;
        for (int m = (int)threadIdx.x; m < members; m += kAdamBlock) {
            int from;
            if (!adam_exploit_source(src, members, m, from) && from != m) c++;
        }
        count[threadIdx.x] = c;
        __syncthreads();
        for (int s = kAdamBlock / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) count[threadIdx.x] += count[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) refused_out[0] = count[0];
    }
    int from;
    if (!adam_exploit_source(src, members, mem, from)) return;  // (workgroup-uniform)
    if (blockIdx.x == 0 && k == 0 && threadIdx.x <= kAdamSkipped)
        state[(size_t)mem * kAdamStateCols + threadIdx.x] = state[(size_t)from * kAdamStateCols + threadIdx.x];
    const size_t n = (size_t)tab.t[k].numel;
    const size_t first = (size_t)blockIdx.x * kAdamTile;
    if (first >= n) return;
    const size_t to = (size_t)mem * n, fr = (size_t)from * n;
    float *p = tab.t[k].param, *ea = tab.t[k].exp_avg, *es = tab.t[k].exp_avg_sq;
#pragma unroll
    for (int j = 0; j < kAdamPerLane; j++) {
        const size_t i = first + (size_t)j * kAdamBlock + threadIdx.x;
        if (i < n) {
            p[to + i] = p[fr + i];
            ea[to + i] = ea[fr + i];
            es[to + i] = es[fr + i];
        }
    }
}
