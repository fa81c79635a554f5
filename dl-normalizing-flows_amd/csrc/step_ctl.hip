// Step control: the decisions a training step takes on the device between
// its backward and its parameter pass (include/realnvp_hip.h, "step control").
//
//   k_grad_sumsq    one pass over the gradient arena: per-workgroup fp64
//                   partial sums of squares of what p.grad holds in the
//                   reference loop (train.py:192-198)
//   k_grad_accumulate  the same pass with gradient accumulation: a held
//                   micro-step adds the arena into the accumulator, the final
//                   one leaves their average in the arena with its partials
//   k_step_control  one workgroup: hold or apply (accumulation), the partials
//                   added in a fixed order, the learning-rate schedule,
//                   clip_grad_norm_'s scale, the non-finite skip and the counters
//   k_step_advance  the step counter, unless the step was skipped
//
// No atomics anywhere: a workgroup owns its partial (one plain store), the
// control kernel adds them in index order, so an eager and a replayed step
// take bitwise the same decision from the same gradients.
#include "common.h"

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_MAX_PARTS = 2048;
constexpr int GS_U = 4;          // granules in flight per thread
constexpr int SC_THREADS = 256;

// the contribution of one element: nothing when frozen (a non-finite value
// behind mask 0 must not reach the sum: select, not multiply)
__device__ __forceinline__ double gs_elem(double acc, float g, uint32_t f, float p, double reg2) {
    double x = (double)g;
    if (f == 2) x = fma(reg2, (double)p, x);
    return f ? fma(x, x, acc) : acc;
}

__global__ __launch_bounds__(GS_THREADS) void k_grad_sumsq(const floatx4* __restrict__ g, const floatx4* __restrict__ p,
                                                           const uint32_t* __restrict__ mask, float reg_coef,
                                                           long long n4, double* __restrict__ partials) {
    __shared__ double red[GS_THREADS / 64];
    const double reg2 = (double)(2.f * reg_coef);
    const long long stride = (long long)gridDim.x * GS_THREADS;
    double acc = 0.0;
    // GS_U granules' loads (16 B of gradient, the 4 mask bytes as one word)
    // are issued before any is used; an index past the end is clamped to the
    // iteration's first granule and its contribution dropped
    for (long long i0 = (long long)blockIdx.x * GS_THREADS + threadIdx.x; i0 < n4; i0 += GS_U * stride) {
        floatx4 G[GS_U];
        uint32_t K[GS_U];
#pragma unroll
        for (int u = 0; u < GS_U; ++u) {
            const long long i = i0 + u * stride < n4 ? i0 + u * stride : i0;
            G[u] = g[i];
            K[u] = mask ? mask[i] : 0x01010101u;
        }
#pragma unroll
        for (int u = 0; u < GS_U; ++u) {
            const bool ok = i0 + u * stride < n4;
            const uint32_t mk = ok ? K[u] : 0u;
            // the parameter granule only where the regulariser applies
            // (weight_g / scale: a sliver of the arena)
            const bool reg = ((mk & 0x02020202u) & ~((mk & 0x01010101u) << 1)) != 0;
            floatx4 P = {0.f, 0.f, 0.f, 0.f};
            if (reg) P = p[i0 + u * stride];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = gs_elem(acc, G[u][e], (mk >> (8 * e)) & 0xffu, P[e], reg2);
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < GS_THREADS / 64; ++w) t += red[w];
        partials[blockIdx.x] = t;
    }
}

// Gradient accumulation: k_grad_sumsq's loop (grid, thread-to-granule mapping,
// GS_U loads in flight, clamped tail) over the gradient arena and its
// accumulator.  A held micro-step (ctl->micro < accum_steps - 1) stores
// acc += g and nothing else: 12 B / element, no mask.  The last one stores
// g = (acc + g) / K (a true division: correctly rounded for every K) and
// acc = 0, and sums the new g's squares exactly as k_grad_sumsq would -- same
// elements per thread in the same order, same reduction -- so the partials are
// bitwise those of a separate norm pass.
__global__ __launch_bounds__(GS_THREADS) void k_grad_accumulate(floatx4* __restrict__ g, floatx4* __restrict__ accum,
                                                                const floatx4* __restrict__ p,
                                                                const uint32_t* __restrict__ mask, float reg_coef,
                                                                long long n4, const rnvp_step_ctl* __restrict__ ctl,
                                                                double* __restrict__ partials) {
    __shared__ double red[GS_THREADS / 64];
    const int K = ctl->accum_steps > 1 ? ctl->accum_steps : 1;
    const bool last = !(ctl->micro < K - 1);
    const float kf = (float)K;
    const double reg2 = (double)(2.f * reg_coef);
    const long long stride = (long long)gridDim.x * GS_THREADS;
    double acc = 0.0;
    for (long long i0 = (long long)blockIdx.x * GS_THREADS + threadIdx.x; i0 < n4; i0 += GS_U * stride) {
        floatx4 G[GS_U], A[GS_U];
        uint32_t M[GS_U];
#pragma unroll
        for (int u = 0; u < GS_U; ++u) {
            const long long i = i0 + u * stride < n4 ? i0 + u * stride : i0;
            G[u] = g[i];
            A[u] = accum[i];
            M[u] = last ? (mask ? mask[i] : 0x01010101u) : 0u;
        }
        if (!last) {
#pragma unroll
            for (int u = 0; u < GS_U; ++u)
                if (i0 + u * stride < n4) accum[i0 + u * stride] = A[u] + G[u];
            continue;
        }
#pragma unroll
        for (int u = 0; u < GS_U; ++u) {
            const bool ok = i0 + u * stride < n4;
            const uint32_t mk = ok ? M[u] : 0u;
            const bool reg = ((mk & 0x02020202u) & ~((mk & 0x01010101u) << 1)) != 0;
            floatx4 P = {0.f, 0.f, 0.f, 0.f};
            if (reg) P = p[i0 + u * stride];
            floatx4 V;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                V[e] = (A[u][e] + G[u][e]) / kf;
                acc = gs_elem(acc, V[e], (mk >> (8 * e)) & 0xffu, P[e], reg2);
            }
            if (ok) {
                g[i0 + u * stride] = V;
                accum[i0 + u * stride] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    if (!last) return;
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < GS_THREADS / 64; ++w) t += red[w];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(SC_THREADS) void k_step_control(rnvp_step_ctl* __restrict__ ctl,
                                                             const long long* __restrict__ step,
                                                             const double* __restrict__ partials, int n_parts) {
    __shared__ double chunk[SC_THREADS];
    // a held micro-step of an accumulating block (every thread reads micro
    // before the barrier, thread 0 writes it after): the partials are stale
    const int K = ctl->accum_steps;
    const bool hold = partials && K > 1 && ctl->micro < K - 1;
    if (partials && !hold) {
        // thread t adds partials [t c, (t + 1) c) in index order, thread 0 the
        // chunk sums in index order
        const int c = (n_parts + SC_THREADS - 1) / SC_THREADS;
        const int lo = threadIdx.x * c, hi = min(n_parts, lo + c);
        double a = 0.0;
        for (int i = lo; i < hi; ++i) a += partials[i];
        chunk[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long u = step[0];
    const double W = (double)ctl->warmup_steps, s = (double)ctl->warmup_start;
    double f = 1.0;
    if (ctl->warmup_steps > 0) f = s + (1.0 - s) * fmin((double)u, W) / W;
    if (ctl->decay == RNVP_DECAY_EXP) {
        f *= pow(ctl->decay_rate, (double)u);
    } else if (ctl->decay == RNVP_DECAY_COSINE) {
        const double T = (double)ctl->decay_steps, fl = ctl->decay_rate;
        f *= fl + (1.0 - fl) * 0.5 * (1.0 + cos(M_PI * fmin((double)u, T) / T));
    }
    ctl->lr = (float)((double)ctl->base_lr * f);
    float scale = 1.0f;
    int skip = 0;
    if (hold) {
        // nothing is applied: the Adam kernels and k_step_advance see a skip;
        // grad_norm and the counters keep the last optimizer step's values
        skip = 1;
        ctl->hold = 1;
        ctl->micro += 1;
    } else if (partials) {
        if (K > 1) {
            ctl->micro = 0;
            ctl->hold = 0;
        }
        double ss = 0.0;
        for (int i = 0; i < SC_THREADS; ++i) ss += chunk[i];
        const double norm = sqrt(ss);
        ctl->grad_norm = (float)norm;
        if (!isfinite(ss)) {
            skip = 1;
            ctl->n_skipped += 1;
        } else if (ctl->max_norm > 0.f) {
            const double c = (double)ctl->max_norm / (norm + 1e-6);
            if (c < 1.0) scale = (float)c;
            if (scale < 1.0f) ctl->n_clipped += 1;
        }
    }
    ctl->grad_scale = scale;
    ctl->skip = skip;
}

__global__ void k_step_advance(long long* step, const rnvp_step_ctl* __restrict__ ctl) {
    if (!ctl->skip) step[0] += 1;
}

}  // namespace

extern "C" int rnvp_grad_sumsq_parts(long long n) {
    if (n < 0) return RNVP_E_INVALID;
    return rnvp_grid(n / 4, GS_THREADS, GS_MAX_PARTS);
}

extern "C" int rnvp_grad_sumsq(const rnvp_adam_args* ad, long long n, double* partials, int n_parts, void* stream) {
    if (!ad || !partials || n < 0 || (n & 3)) return RNVP_E_INVALID;
    if (!ad->grad || !ad->param) return RNVP_E_INVALID;
    if ((((uintptr_t)ad->grad) | ((uintptr_t)ad->param)) & 15) return RNVP_E_INVALID;
    if ((ad->mask && (((uintptr_t)ad->mask) & 3)) || (((uintptr_t)partials) & 7)) return RNVP_E_INVALID;
    if (n_parts != rnvp_grad_sumsq_parts(n)) return RNVP_E_INVALID;
    k_grad_sumsq<<<n_parts, GS_THREADS, 0, (hipStream_t)stream>>>((const floatx4*)ad->grad, (const floatx4*)ad->param,
                                                                  (const uint32_t*)ad->mask, ad->reg_coef, n / 4,
                                                                  partials);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_grad_accumulate(const rnvp_adam_args* ad, float* acc, long long n, const rnvp_step_ctl* ctl,
                                    double* partials, int n_parts, void* stream) {
    if (!ad || !acc || !ctl || !partials || n < 0 || (n & 3)) return RNVP_E_INVALID;
    if (!ad->grad || !ad->param) return RNVP_E_INVALID;
    if ((((uintptr_t)ad->grad) | ((uintptr_t)ad->param) | ((uintptr_t)acc)) & 15) return RNVP_E_INVALID;
    if ((ad->mask && (((uintptr_t)ad->mask) & 3)) || (((uintptr_t)partials) & 7)) return RNVP_E_INVALID;
    if (acc == ad->grad || n_parts != rnvp_grad_sumsq_parts(n)) return RNVP_E_INVALID;
    k_grad_accumulate<<<n_parts, GS_THREADS, 0, (hipStream_t)stream>>>((floatx4*)ad->grad, (floatx4*)acc,
                                                                       (const floatx4*)ad->param,
                                                                       (const uint32_t*)ad->mask, ad->reg_coef, n / 4,
                                                                       ctl, partials);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_step_control(rnvp_step_ctl* ctl, const long long* step, const double* partials, int n_parts,
                                 void* stream) {
    if (!ctl || !step) return RNVP_E_INVALID;
    if (partials && (n_parts < 1 || n_parts > GS_MAX_PARTS)) return RNVP_E_INVALID;
    k_step_control<<<1, SC_THREADS, 0, (hipStream_t)stream>>>(ctl, step, partials, partials ? n_parts : 0);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_step_advance(long long* step, const rnvp_step_ctl* ctl, void* stream) {
    if (!step || !ctl) return RNVP_E_INVALID;
    k_step_advance<<<1, 1, 0, (hipStream_t)stream>>>(step, ctl);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}
