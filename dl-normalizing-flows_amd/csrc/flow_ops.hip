// Flow-level kernels: index maps, logit transform, scoring, prior log-prob,
// regulariser, BN running stats, fused Adam.  All HBM-bound elementwise / reduction work.
#include <math.h>

#include "coupling_common.h"

extern "C" int rnvp_version(void) { return 114; }

extern "C" int rnvp_struct_size(int which) {
    switch (which) {
        case 0: return (int)sizeof(rnvp_bn_src);
        case 1: return (int)sizeof(rnvp_bn_running);
        case 2: return (int)sizeof(rnvp_conv_args);
        case 3: return (int)sizeof(rnvp_wgrad_conv);
        case 4: return (int)sizeof(rnvp_wgrad_group);
        case 5: return (int)sizeof(rnvp_bn_bwd_args);
        case 6: return (int)sizeof(rnvp_wn_desc);
        case 7: return (int)sizeof(rnvp_adam_args);
        case 8: return (int)sizeof(rnvp_coupling_args);
        case 9: return (int)sizeof(rnvp_net_step);
        case 10: return (int)sizeof(rnvp_range);
        case 11: return (int)sizeof(rnvp_link_args);
        case 12: return (int)sizeof(rnvp_step_ctl);
    }
    return -1;
}

extern "C" const char* rnvp_status_string(int s) {
    if (s == RNVP_OK) return "ok";
    if (s == RNVP_E_INVALID) return "invalid argument";
    if (s == RNVP_E_UNSUPPORTED) return "unsupported configuration";
    return hipGetErrorString((hipError_t)s);
}

// Profiling marker: an empty one-lane dispatch.  bench.py brackets each engine
// launch of its instrumented step with one so that per-dispatch PMC records
// (rocprofv3 --pmc) can be attributed to kernel families (tools/pmc_traffic.py).
__global__ void k_marker(int tag) { (void)tag; }

extern "C" int rnvp_marker(int tag, void* stream) {
    k_marker<<<1, 1, 0, (hipStream_t)stream>>>(tag);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// index maps  (modules_realnvp.py:211-226, flow_realnvp.py:121-193)
// ---------------------------------------------------------------------------
__global__ void k_mask(float* m, int S, int cfg) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S * S) m[i] = (float)((cfg + i / S + i % S) & 1);
}

extern "C" int rnvp_checkerboard_mask(float* mask, int size, int config, void* stream) {
    if (!mask || size <= 0) return RNVP_E_INVALID;
    k_mask<<<rnvp_grid((long long)size * size, 256, 1 << 20), 256, 0, (hipStream_t)stream>>>(mask, size, config & 1);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// squeeze: y[b, 4c+2i+j, h, w] = x[b, c, 2h+i, 2w+j].  One thread per x element
// (coalesced read), indices in 64-bit.
__global__ void k_squeeze(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W, long long n) {
    const int h2 = H >> 1, w2 = W >> 1;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        int xx = (int)(e % W);
        long long t = e / W;
        int yy = (int)(t % H);
        t /= H;
        int c = (int)(t % C);
        long long b = t / C;
        int i = yy & 1, j = xx & 1;
        long long o = (((b * 4 * C + 4 * c + 2 * i + j) * h2 + (yy >> 1)) * w2 + (xx >> 1));
        y[o] = x[e];
    }
}
// undo: x[b, c, 2h+i, 2w+j] = y[b, 4c+2i+j, h, w]  (gather, one thread per x element)
__global__ void k_undo_squeeze(const float* __restrict__ y, float* __restrict__ x, int C, int H, int W, long long n) {
    const int h2 = H >> 1, w2 = W >> 1;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        int xx = (int)(e % W);
        long long t = e / W;
        int yy = (int)(t % H);
        t /= H;
        int c = (int)(t % C);
        long long b = t / C;
        int i = yy & 1, j = xx & 1;
        x[e] = y[(((b * 4 * C + 4 * c + 2 * i + j) * h2 + (yy >> 1)) * w2 + (xx >> 1))];
    }
}

extern "C" int rnvp_squeeze(const float* x, float* y, int B, int C, int H, int W, void* stream) {
    if (!x || !y || B < 0 || C <= 0 || (H & 1) || (W & 1)) return RNVP_E_INVALID;
    long long n = (long long)B * C * H * W;
    if (n == 0) return RNVP_OK;
    k_squeeze<<<rnvp_grid(n, 256), 256, 0, (hipStream_t)stream>>>(x, y, C, H, W, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_undo_squeeze(const float* y, float* x, int B, int C, int H, int W, void* stream) {
    if (!x || !y || B < 0 || C <= 0 || (H & 1) || (W & 1)) return RNVP_E_INVALID;
    long long n = (long long)B * C * H * W;
    if (n == 0) return RNVP_OK;
    k_undo_squeeze<<<rnvp_grid(n, 256), 256, 0, (hipStream_t)stream>>>(y, x, C, H, W, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// factor_out: (y&1, x&1) = (0,0) -> on[c], (1,1) -> on[C+c], (0,1) -> off[c], (1,0) -> off[C+c]
__global__ void k_factor_out(const float* __restrict__ x, float* __restrict__ on, float* __restrict__ off,
                             int C, int H, int W, long long n) {
    const int h2 = H >> 1, w2 = W >> 1;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        int xx = (int)(e % W);
        long long t = e / W;
        int yy = (int)(t % H);
        t /= H;
        int c = (int)(t % C);
        long long b = t / C;
        int i = yy & 1, j = xx & 1;
        float* dst = (i == j) ? on : off;
        int cc = (i == 0) ? c : C + c;
        dst[((b * 2 * C + cc) * h2 + (yy >> 1)) * w2 + (xx >> 1)] = x[e];
    }
}
__global__ void k_restore(const float* __restrict__ on, const float* __restrict__ off, float* __restrict__ x,
                          int C, int H, int W, long long n) {
    const int h2 = H >> 1, w2 = W >> 1;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        int xx = (int)(e % W);
        long long t = e / W;
        int yy = (int)(t % H);
        t /= H;
        int c = (int)(t % C);
        long long b = t / C;
        int i = yy & 1, j = xx & 1;
        const float* src = (i == j) ? on : off;
        int cc = (i == 0) ? c : C + c;
        x[e] = src[((b * 2 * C + cc) * h2 + (yy >> 1)) * w2 + (xx >> 1)];
    }
}

extern "C" int rnvp_factor_out(const float* x, float* on, float* off, int B, int C, int H, int W, void* stream) {
    if (!x || !on || !off || B < 0 || C <= 0 || (H & 1) || (W & 1)) return RNVP_E_INVALID;
    long long n = (long long)B * C * H * W;
    if (n == 0) return RNVP_OK;
    k_factor_out<<<rnvp_grid(n, 256), 256, 0, (hipStream_t)stream>>>(x, on, off, C, H, W, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_restore(const float* on, const float* off, float* x, int B, int C, int H, int W, void* stream) {
    if (!x || !on || !off || B < 0 || C <= 0 || (H & 1) || (W & 1)) return RNVP_E_INVALID;
    long long n = (long long)B * C * H * W;
    if (n == 0) return RNVP_OK;
    k_restore<<<rnvp_grid(n, 256), 256, 0, (hipStream_t)stream>>>(on, off, x, C, H, W, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// logit transform (utils.py:33-72)
// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011), counter = (offset+i, 0, 0, 0), key = seed
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t ctr) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (c0 >> 8) * (1.0f / 16777216.0f);   // [0, 1)
}

__device__ __forceinline__ float softplusf(float v) { return v > 20.f ? v : log1pf(expf(v)); }

// one element of the transform (utils.py:45-66): the dequantised, constrained
// pixel's logit, and its term of the log-determinant (sp_pre = softplus(-logit(cst)))
__device__ __forceinline__ float logit_elem(float x, float u, float cst) {
    float v = (x * 255.f + u) / 256.f;
    v = ((v * 2.f - 1.f) * cst + 1.f) / 2.f;
    return logf(v) - logf(1.f - v);
}
__device__ __forceinline__ float logit_ld(float l, float sp_pre) { return softplusf(l) + softplusf(-l) - sp_pre; }
__device__ __forceinline__ float logit_sp_pre(float cst) {
    return softplusf(-(float)(log((double)cst) - log(1.0 - (double)cst)));
}

__global__ void k_logit_fwd(const float* __restrict__ x, const float* __restrict__ noise, uint64_t seed, uint64_t offset,
                            const long long* epoch, float cst, float* __restrict__ y, float* __restrict__ logdet, int n) {
    __shared__ double red[16];
    const int b = blockIdx.x;
    const long long base = (long long)b * n;
    if (epoch) offset += (uint64_t)epoch[0] * (uint64_t)gridDim.x * (uint64_t)n;
    const float sp_pre = logit_sp_pre(cst);
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        long long e = base + i;
        float u = noise ? noise[e] : philox_uniform(seed, offset + (uint64_t)e);
        float l = logit_elem(x[e], u, cst);
        y[e] = l;
        acc += (double)logit_ld(l, sp_pre);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) logdet[b] = (float)acc;
}

extern "C" int rnvp_logit_fwd(const float* x, const float* noise, uint64_t seed, uint64_t offset,
                              const long long* epoch, float constraint, float* y, float* logdet, int B,
                              int n_per_sample, void* stream) {
    if (!x || !y || !logdet || B < 0 || n_per_sample <= 0) return RNVP_E_INVALID;
    if (B == 0) return RNVP_OK;
    k_logit_fwd<<<B, 512, 0, (hipStream_t)stream>>>(x, noise, seed, offset, epoch, constraint, y, logdet,
                                                     n_per_sample);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// The training step's input pass: the logit transform over pixel tiles of
// every sample (all CUs busy: k_logit_fwd has one workgroup per sample), the
// per-sample log-det added with one atomic per workgroup, and the first
// coupling's in_bn batch sums (k_in_stats) of the values just computed.
__global__ __launch_bounds__(256) void k_flow_in(const float* __restrict__ x, uint64_t seed, const long long* epoch,
                                                 uint64_t epoch_stride, float cst, float* __restrict__ y,
                                                 float* __restrict__ logdet, rnvp_coupling_args a, int first, int C,
                                                 int HW, int TP, int seg) {
    // the noise stream of rnvp_logit_fwd: Philox counter = NCHW index + epoch * B*C*H*W
    const uint64_t offset = epoch ? (uint64_t)epoch[0] * epoch_stride : 0;
    extern __shared__ double red[];   // [2*Cb]
    __shared__ double redl[16];
    const int tpi = (HW + TP - 1) / TP;
    const int b = blockIdx.x / tpi, p0 = (blockIdx.x - b * tpi) * TP, tp = min(TP, HW - p0);
    const int lane = threadIdx.x & 63;
    Geo g;
    int Cb = 0;
    if (first) {
        g = geo(a);
        Cb = g.Cb;
        lds_zero(red, 2 * Cb);
        __syncthreads();
    }
    const float sp_pre = logit_sp_pre(cst);
    const int total = C * tp;
    double acc = 0.0;
    for (int e0 = 0; e0 < total; e0 += 256) {   // block-uniform: the segment sums need every lane
        const int e = e0 + threadIdx.x;
        const bool ok = e < total;
        const int c = ok ? e / tp : 0, p = p0 + (ok ? e - c * tp : 0);
        const long long idx = ((long long)b * C + c) * HW + p;
        float l = 0.f;
        if (ok) {
            const float u = philox_uniform(seed, offset + (uint64_t)idx);
            l = logit_elem(x[idx], u, cst);
            y[idx] = l;
            acc += (double)logit_ld(l, sp_pre);
        }
        if (first) {
            int cb = c;
            float xm = l;
            if (g.kind == 0) {
                if (!ckbd_m(g, p)) xm = 0.f;
            } else {
                cb = c - g.off_base;
                if (cb < 0 || cb >= Cb) xm = 0.f;
            }
            const double s1 = seg_red((double)xm, seg), s2 = seg_red((double)xm * xm, seg);
            if (ok && cb >= 0 && cb < Cb && (lane & seg_mask(seg)) == 0) {
                atomicAdd(&red[cb], s1);
                atomicAdd(&red[Cb + cb], s2);
            }
        }
    }
    acc = block_sum(acc, redl);   // (barriers also publish red)
    if (threadIdx.x == 0) atomicAdd(&logdet[b], (float)acc);
    if (first) {
        double* dst = cshard(a.in_sums, 2 * Cb);
        for (int c = threadIdx.x; c < 2 * Cb; c += blockDim.x) atomicAdd(&dst[c], red[c]);
    }
}

extern "C" int rnvp_flow_in_fwd(const float* x, uint64_t seed, const long long* epoch, float constraint, float* y,
                                float* logdet, const rnvp_coupling_args* first, int B, int C, int H, int W,
                                void* stream) {
    if (!x || !y || !logdet || B < 0 || C <= 0 || H <= 0 || W <= 0) return RNVP_E_INVALID;
    if (first && (first->x != y || !first->training || !first->in_sums || first->B != B || first->C != C ||
                  first->H != H || first->W != W || (first->kind == 1 && (C & 1))))
        return RNVP_E_INVALID;
    if (B == 0) return RNVP_OK;
    const int HW = H * W;
    int TP = HW < 256 ? HW : 256;
    while (TP > 16 && TP % 2 == 0 && (long long)B * ((HW + TP - 1) / TP) < 1024) TP /= 2;
    int seg = 1;
    while (seg < 64 && TP % (2 * seg) == 0 && HW % (2 * seg) == 0) seg *= 2;
    const int grid = B * ((HW + TP - 1) / TP);
    const int Cb = first ? (first->kind == 0 ? C : C / 2) : 0;
    rnvp_coupling_args none{};
    k_flow_in<<<grid, 256, 16 * (size_t)Cb, (hipStream_t)stream>>>(x, seed, epoch, (uint64_t)B * C * HW, constraint,
                                                                   y, logdet, first ? *first : none, first ? 1 : 0, C,
                                                                   HW, TP, seg);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// scoring (include/realnvp_hip.h, "scoring"): per-image log-likelihoods of
// ragged batches, K noise draws per image, one device-resident control block
//   k_score_in       the logit transform with per-IMAGE noise, a chunk of one
//                    sample per workgroup
//   k_score_rows     one workgroup per row: this draw's log-likelihood, the
//                    online log-sum-exp over the draws, the finalised score
//   k_score_advance  one workgroup, behind the rows: the block's counters
// ---------------------------------------------------------------------------
constexpr int SCORE_CHUNKS = 8;   // per sample: one fp32 atomic on logdet[b] each (header: the rounding bound)

__global__ __launch_bounds__(256) void k_score_in(const float* __restrict__ x, const float* __restrict__ noise,
                                                  uint64_t seed, const rnvp_score_ctl* __restrict__ ctl, float cst,
                                                  float* __restrict__ y, float* __restrict__ logdet, int n, int chunks,
                                                  int chunk) {
    __shared__ double red[16];
    const int b = blockIdx.x / chunks, i0 = (blockIdx.x - b * chunks) * chunk, i1 = min(n, i0 + chunk);
    // the image's own stream: counter ((first + b) K + draw) n + e
    const uint64_t ctr = ((uint64_t)(ctl->first + b) * (uint64_t)ctl->n_draws + (uint64_t)ctl->draw) * (uint64_t)n;
    const long long base = (long long)b * n;
    const float sp_pre = logit_sp_pre(cst);
    double acc = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const float u = noise ? noise[base + i] : philox_uniform(seed, ctr + (uint64_t)i);
        const float l = logit_elem(x[base + i], u, cst);
        y[base + i] = l;
        acc += (double)logit_ld(l, sp_pre);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0 && i0 < i1) atomicAdd(&logdet[b], (float)acc);
}

extern "C" int rnvp_score_in_fwd(const float* x, const float* noise, uint64_t seed, const rnvp_score_ctl* ctl,
                                 float constraint, float* y, float* logdet, int B, int C, int H, int W, void* stream) {
    if (!x || !y || !logdet || !ctl || B < 0 || C <= 0 || H <= 0 || W <= 0) return RNVP_E_INVALID;
    if (((((uintptr_t)x) | ((uintptr_t)noise) | ((uintptr_t)y) | ((uintptr_t)logdet)) & 3) || (((uintptr_t)ctl) & 7))
        return RNVP_E_INVALID;
    const long long n = (long long)C * H * W;
    if (n > 0x7fffffffLL) return RNVP_E_INVALID;
    if (B == 0) return RNVP_OK;
    // more workgroups than samples at small B, a chunk no shorter than the workgroup's 256 threads
    int chunks = 1;
    while (chunks < SCORE_CHUNKS && (long long)B * chunks < 1024 && n / (2 * chunks) >= 256) chunks *= 2;
    if ((long long)B * chunks > 0x7fffffffLL) return RNVP_E_INVALID;
    const int chunk = (int)((n + chunks - 1) / chunks);
    k_score_in<<<B * chunks, 256, 0, (hipStream_t)stream>>>(x, noise, seed, ctl, constraint, y, logdet, (int)n, chunks,
                                                             chunk);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

__global__ __launch_bounds__(512) void k_score_rows(const float* __restrict__ z, float* __restrict__ ldj,
                                                    float* __restrict__ logdet, float* __restrict__ run,
                                                    float* __restrict__ lp, const rnvp_score_ctl* __restrict__ ctl,
                                                    int n) {
    __shared__ double red[16];
    const int b = blockIdx.x;
    const float* zb = z + (long long)b * n;
    const double c = 0.91893853320467274178;   // log(2 pi) / 2
    double acc = 0.0;
    if ((n & 3) == 0 && (((uintptr_t)z) & 15) == 0) {
        for (int i = threadIdx.x; i < (n >> 2); i += blockDim.x) {
            const floatx4 v = ((const floatx4*)zb)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += -0.5 * (double)v[j] * (double)v[j] - c;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += blockDim.x) acc += -0.5 * (double)zb[i] * (double)zb[i] - c;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x != 0) return;
    const double ll = acc + (double)ldj[b] + (double)logdet[b];
    ldj[b] = 0.f;
    logdet[b] = 0.f;
    if (b >= ctl->n_valid) return;   // a padding row: nothing but the zeroing
    if (lp) lp[b] = (float)ll;
    // online log-sum-exp over the draws: m is an fp32 value, the exponents are
    // taken against exactly that value, so its rounding costs nothing
    const int K = ctl->n_draws, k = ctl->draw;
    float m = (float)ll;
    double s = exp(ll - (double)m);
    if (k > 0) {
        const float m0 = run[2 * b];
        const double s0 = (double)run[2 * b + 1];
        if (m0 >= m) {
            s = s0 + exp(ll - (double)m0);
            m = m0;
        } else {
            s += s0 * exp((double)m0 - (double)m);
        }
    }
    if (k < K - 1) {
        run[2 * b] = m;
        run[2 * b + 1] = (float)s;
        return;
    }
    const float score = K == 1 ? (float)ll : (float)((double)m + log(s) - log((double)K));
    run[2 * b] = score;   // for k_score_advance's sum
    const long long at = ctl->first + b;
    if (at >= 0 && at < ctl->cap) ctl->scores[at] = score;
}

__global__ __launch_bounds__(256) void k_score_advance(const float* __restrict__ run, rnvp_score_ctl* ctl, int B) {
    __shared__ float sc[256];
    __shared__ int cfg[3];
    // one thread reads the fields that thread 0 writes below, for all (a wave
    // that started late must not see the advanced draw)
    if (threadIdx.x == 0) {
        cfg[0] = ctl->n_draws;
        cfg[1] = ctl->draw;
        cfg[2] = max(0, min(ctl->n_valid, B));
    }
    __syncthreads();
    const int K = cfg[0], k = cfg[1], nv = cfg[2];
    if (k < K - 1) {
        if (threadIdx.x == 0) ctl->draw = k + 1;
        return;
    }
    // the finalised scores, added in row order by one thread (256 rows' loads at a time)
    double sum = ctl->ll_sum;
    for (int b0 = 0; b0 < nv; b0 += 256) {
        if (b0 + (int)threadIdx.x < nv) sc[threadIdx.x] = run[2 * (b0 + (int)threadIdx.x)];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int j = 0; j < min(256, nv - b0); ++j) sum += (double)sc[j];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ctl->ll_sum = sum;
        if (ctl->first + nv > ctl->cap) ctl->overflow = 1;
        ctl->n_scored = ctl->n_scored + nv;
        ctl->first = ctl->first + nv;
        ctl->draw = 0;
    }
}

extern "C" int rnvp_score_struct_size(void) { return (int)sizeof(rnvp_score_ctl); }

extern "C" int rnvp_score_finish(const float* z, float* ldj, float* logdet, float* run, float* lp, rnvp_score_ctl* ctl,
                                 int B, int n_per_sample, void* stream) {
    if (!z || !ldj || !logdet || !run || !ctl || B < 0 || n_per_sample <= 0) return RNVP_E_INVALID;
    if (((((uintptr_t)z) | ((uintptr_t)ldj) | ((uintptr_t)logdet) | ((uintptr_t)run) | ((uintptr_t)lp)) & 3) ||
        (((uintptr_t)ctl) & 7))
        return RNVP_E_INVALID;
    if (B == 0) return RNVP_OK;
    k_score_rows<<<B, 512, 0, (hipStream_t)stream>>>(z, ldj, logdet, run, lp, ctl, n_per_sample);
    RNVP_LAUNCH_CHECK();
    k_score_advance<<<1, 256, 0, (hipStream_t)stream>>>(run, ctl, B);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

__global__ void k_logit_inv(const float* __restrict__ x, float* __restrict__ y, float cst, long long n) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        float v = 1.f / (expf(-x[e]) + 1.f);
        y[e] = ((v * 2.f - 1.f) / cst + 1.f) / 2.f;
    }
}

extern "C" int rnvp_logit_inv(const float* x, float* y, float constraint, long long n, void* stream) {
    if (!x || !y || n < 0) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;
    k_logit_inv<<<rnvp_grid(n, 256), 256, 0, (hipStream_t)stream>>>(x, y, constraint, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// transforms.ToTensor on the device (train.py:65-71): uint8 CHW images arrive
// over PCIe at 1 B/pixel and become k / 255 in fp32 (correctly rounded
// division, as torch's CPU uint8 -> float -> div(255)).  16 pixels per lane.
// ---------------------------------------------------------------------------
__global__ void k_u8_to_unit(const uint8_t* __restrict__ x, float* __restrict__ y, long long n) {
    const long long n16 = n >> 4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n16; q += stride) {
        const uint4 v = *(const uint4*)(x + 16 * q);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        float4* o = (float4*)(y + 16 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = make_float4((float)(w[j] & 255u) / 255.f, (float)((w[j] >> 8) & 255u) / 255.f,
                               (float)((w[j] >> 16) & 255u) / 255.f, (float)(w[j] >> 24) / 255.f);
    }
    for (long long e = 16 * n16 + blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += stride)
        y[e] = (float)x[e] / 255.f;
}

extern "C" int rnvp_u8_to_unit(const uint8_t* x, float* y, long long n, void* stream) {
    if (n < 0) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;   // empty tensors may carry null pointers
    if (!x || !y || (((uintptr_t)x) & 15) || (((uintptr_t)y) & 15)) return RNVP_E_INVALID;
    k_u8_to_unit<<<rnvp_grid((n + 15) / 16, 256), 256, 0, (hipStream_t)stream>>>(x, y, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// NCHW fp32 <-> NHWC (channel stride cs, fp32 / bf16) layout moves: the
// operands of a standalone WeightNormConv2d call (modules_realnvp.py:64-71).
// Off the training path (the coupling engine keeps the net in NHWC), so a
// plain grid-stride element map: coalesced on the written side.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_nchw_to_nhwc(const float* __restrict__ x, T* __restrict__ y, int C, int HW, int cs, long long n) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long m = e / cs;
        const int c = (int)(e - m * cs);
        const long long b = m / HW;
        const int p = (int)(m - b * HW);
        stv(&y[e], c < C ? x[(b * C + c) * HW + p] : 0.f);
    }
}

template <typename T>
__global__ void k_nhwc_to_nchw(const T* __restrict__ x, float* __restrict__ y, int C, int HW, int cs, long long n) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(e % HW);
        const long long t = e / HW;
        const int c = (int)(t % C);
        const long long b = t / C;
        y[e] = ldv(&x[(b * HW + p) * cs + c]);
    }
}

extern "C" int rnvp_nchw_to_nhwc(const float* x, void* y, int B, int C, int H, int W, int cs, int dtype, void* stream) {
    if (B < 0 || C <= 0 || H <= 0 || W <= 0 || cs < C) return RNVP_E_INVALID;
    if (dtype != RNVP_F32 && dtype != RNVP_BF16) return RNVP_E_INVALID;
    const long long n = (long long)B * H * W * cs;
    if (n == 0) return RNVP_OK;
    if (!x || !y) return RNVP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RNVP_F32) k_nchw_to_nhwc<float><<<rnvp_grid(n, 256), 256, 0, s>>>(x, (float*)y, C, H * W, cs, n);
    else k_nchw_to_nhwc<bf16_t><<<rnvp_grid(n, 256), 256, 0, s>>>(x, (bf16_t*)y, C, H * W, cs, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_nhwc_to_nchw(const void* x, float* y, int B, int C, int H, int W, int cs, int dtype, void* stream) {
    if (B < 0 || C <= 0 || H <= 0 || W <= 0 || cs < C) return RNVP_E_INVALID;
    if (dtype != RNVP_F32 && dtype != RNVP_BF16) return RNVP_E_INVALID;
    const long long n = (long long)B * C * H * W;
    if (n == 0) return RNVP_OK;
    if (!x || !y) return RNVP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RNVP_F32) k_nhwc_to_nchw<float><<<rnvp_grid(n, 256), 256, 0, s>>>((const float*)x, y, C, H * W, cs, n);
    else k_nhwc_to_nchw<bf16_t><<<rnvp_grid(n, 256), 256, 0, s>>>((const bf16_t*)x, y, C, H * W, cs, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// prior log-prob (flow_realnvp.py:329-340; train.py:109 prior = N(0,1))
// ---------------------------------------------------------------------------
__global__ void k_prior(const float* __restrict__ z, const float* __restrict__ ldj, float* __restrict__ out, int n) {
    __shared__ double red[16];
    const int b = blockIdx.x;
    const float* zb = z + (long long)b * n;
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float v = zb[i];
        acc += (double)(-0.5f * v * v - 0.91893853320467274178f);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[b] = (float)(acc + (ldj ? (double)ldj[b] : 0.0));
}

extern "C" int rnvp_prior_logprob(const float* z, const float* ldj, float* out, int B, int n, void* stream) {
    if (!z || !out || B < 0 || n <= 0) return RNVP_E_INVALID;
    if (B == 0) return RNVP_OK;
    k_prior<<<B, 512, 0, (hipStream_t)stream>>>(z, ldj, out, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

__global__ void k_prior_bwd(const float* __restrict__ z, const float* __restrict__ gout, float* __restrict__ gz, int n,
                            long long total) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
        gz[e] = -z[e] * gout[e / n];
}

extern "C" int rnvp_prior_logprob_bwd(const float* z, const float* gout, float* gz, int B, int n, void* stream) {
    if (!z || !gout || !gz || B < 0 || n <= 0) return RNVP_E_INVALID;
    long long total = (long long)B * n;
    if (total == 0) return RNVP_OK;
    k_prior_bwd<<<rnvp_grid(total, 256), 256, 0, (hipStream_t)stream>>>(z, gout, gz, n, total);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// end of the training step's forward (flow_realnvp.py:336-338, train.py:192-196):
// lp = prior + ldj per sample, the step's mean log-likelihood into the device
// accumulator, and the per-step accumulators left zero for the next step
__global__ void k_lp_finish(double* prior, float* ldj, float* logdet, int zero_logdet, float* lp, double* ll_acc,
                            int B) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float l = (float)(prior[b] + (double)ldj[b]);
        lp[b] = l;
        acc += (double)(l + logdet[b]);
        prior[b] = 0.0;
        ldj[b] = 0.f;
        if (zero_logdet) logdet[b] = 0.f;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) ll_acc[0] += acc / (double)B;
}

extern "C" int rnvp_flow_lp_finish(double* prior, float* ldj, float* logdet, int zero_logdet, float* lp,
                                   double* ll_acc, int B, void* stream) {
    if (!prior || !ldj || !logdet || !lp || !ll_acc || B <= 0) return RNVP_E_INVALID;
    k_lp_finish<<<1, 256, 0, (hipStream_t)stream>>>(prior, ldj, logdet, zero_logdet, lp, ll_acc, B);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// BatchNorm running statistics (torch BatchNorm2d train-mode semantics)
// ---------------------------------------------------------------------------
__global__ void k_bn_running(const rnvp_bn_running* __restrict__ d, float mom) {
    extern __shared__ double tmp[];   // [2*C]
    const rnvp_bn_running r = d[blockIdx.x];
    bn_running_site(r, mom, tmp);
}

extern "C" int rnvp_bn_running_update(const rnvp_bn_running* d, int n, int max_c, float momentum, void* stream) {
    if (n < 0 || (n > 0 && !d) || max_c <= 0) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;
    k_bn_running<<<n, 256, 16 * (size_t)max_c, (hipStream_t)stream>>>(d, momentum);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// weight_scale regulariser (flow_realnvp.py:362-369): multi-tensor sum of squares
// ---------------------------------------------------------------------------
__global__ void k_sumsq(const rnvp_tensor_ref* __restrict__ refs, float* out) {
    __shared__ double red[16];
    const rnvp_tensor_ref r = refs[blockIdx.x];
    double acc = 0;
    for (long long i = threadIdx.x; i < r.n; i += blockDim.x) acc += (double)r.p[i] * r.p[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) atomicAdd(out, (float)acc);
}

extern "C" int rnvp_sumsq_multi(const rnvp_tensor_ref* refs, int n_refs, float* out, void* stream) {
    if (!out || n_refs < 0 || (n_refs > 0 && !refs)) return RNVP_E_INVALID;
    if (n_refs == 0) return RNVP_OK;
    k_sumsq<<<n_refs, 256, 0, (hipStream_t)stream>>>(refs, out);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

__global__ void k_sumsq_bwd(const rnvp_tensor_ref* __restrict__ refs, const float* gout, float coef) {
    const rnvp_tensor_ref r = refs[blockIdx.x];
    const float s = 2.f * coef * gout[0];
    for (long long i = threadIdx.x; i < r.n; i += blockDim.x) r.g[i] += s * r.p[i];
}

extern "C" int rnvp_sumsq_bwd_multi(const rnvp_tensor_ref* refs, int n_refs, const float* gout, float coef, void* stream) {
    if (!gout || n_refs < 0 || (n_refs > 0 && !refs)) return RNVP_E_INVALID;
    if (n_refs == 0) return RNVP_OK;
    k_sumsq_bwd<<<n_refs, 256, 0, (hipStream_t)stream>>>(refs, gout, coef);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// fused Adam (torch.optim.Adam single-tensor semantics, coupled weight decay)
// ---------------------------------------------------------------------------
__global__ void k_step_inc(long long* step) { step[0] += 1; }

template <bool CTL>
__global__ void k_adam(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                       float4* __restrict__ v, long long n4, const long long* step, long long step_add, float lr,
                       float b1, float b2, float eps, float wd, const uint32_t* __restrict__ regm, float reg,
                       const rnvp_step_ctl* ctl) {
    __shared__ float sh[3];
    if (CTL && adam_skipped(ctl)) return;
    if (threadIdx.x == 0) adam_coef(step, step_add, lr, b1, b2, CTL ? ctl : nullptr, sh);
    __syncthreads();
    const float step_size = sh[0], inv_bc2s = sh[1], gclip = CTL ? sh[2] : 1.0f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
        const uint32_t mk = regm ? regm[i] : 0x01010101u;
        float* pa = (float*)&pp; float* ga = (float*)&gg; float* ma = (float*)&mm; float* va = (float*)&vv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t f = (mk >> (8 * j)) & 0xff;
            if (f == 0) continue;                      // frozen parameter
            pa[j] = adam_elem<CTL>(pa[j], ga[j], ma[j], va[j], (int)f, b1, b2, eps, wd, reg, step_size, inv_bc2s, gclip);
        }
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

extern "C" int rnvp_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                              long long* step, float lr, float beta1, float beta2, float eps, float weight_decay,
                              const uint8_t* reg_mask, float reg_coef, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step || n < 0 || (n & 3)) return RNVP_E_INVALID;
    if ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15) return RNVP_E_INVALID;
    if (reg_mask && (((uintptr_t)reg_mask) & 3)) return RNVP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    k_step_inc<<<1, 1, 0, s>>>(step);
    RNVP_LAUNCH_CHECK();
    if (n == 0) return RNVP_OK;
    long long n4 = n / 4;
    k_adam<false><<<rnvp_grid(n4, 256, 8192), 256, 0, s>>>((float4*)param, (const float4*)grad, (float4*)exp_avg,
                                                   (float4*)exp_avg_sq, n4, step, 0, lr, beta1, beta2, eps, weight_decay,
                                                   (const uint32_t*)reg_mask, reg_coef, nullptr);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_adam_update(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                                const long long* step, long long step_add, float lr, float beta1, float beta2,
                                float eps, float weight_decay, const uint8_t* reg_mask, float reg_coef, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step || n < 0 || (n & 3)) return RNVP_E_INVALID;
    if ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15) return RNVP_E_INVALID;
    if (reg_mask && (((uintptr_t)reg_mask) & 3)) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;
    const long long n4 = n / 4;
    k_adam<false><<<rnvp_grid(n4, 256, 8192), 256, 0, (hipStream_t)stream>>>(
        (float4*)param, (const float4*)grad, (float4*)exp_avg, (float4*)exp_avg_sq, n4, step, step_add, lr, beta1,
        beta2, eps, weight_decay, (const uint32_t*)reg_mask, reg_coef, nullptr);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_adam_range(const rnvp_adam_args* ad, long long n, void* stream) {
    if (!ad || n < 0 || (n & 3)) return RNVP_E_INVALID;
    if (!ad->param || !ad->grad || !ad->exp_avg || !ad->exp_avg_sq || !ad->step) return RNVP_E_INVALID;
    if ((((uintptr_t)ad->param) | ((uintptr_t)ad->grad) | ((uintptr_t)ad->exp_avg) | ((uintptr_t)ad->exp_avg_sq)) & 15)
        return RNVP_E_INVALID;
    if (ad->mask && (((uintptr_t)ad->mask) & 3)) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;
    const long long n4 = n / 4;
    const auto kern = ad->ctl ? k_adam<true> : k_adam<false>;
    kern<<<rnvp_grid(n4, 256, 8192), 256, 0, (hipStream_t)stream>>>(
        (float4*)ad->param, (const float4*)ad->grad, (float4*)ad->exp_avg, (float4*)ad->exp_avg_sq, n4, ad->step,
        ad->step_add, ad->lr, ad->beta1, ad->beta2, ad->eps, ad->weight_decay, (const uint32_t*)ad->mask,
        ad->reg_coef, ad->ctl);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_step_increment(long long* step, void* stream) {
    if (!step) return RNVP_E_INVALID;
    k_step_inc<<<1, 1, 0, (hipStream_t)stream>>>(step);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

__global__ void k_fill64(double* p, long long n, double v) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}

extern "C" int rnvp_fill_f64(double* p, long long n, double v, void* stream) {
    if (!p || n < 0) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;
    k_fill64<<<rnvp_grid(n, 256), 256, 0, (hipStream_t)stream>>>(p, n, v);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}
