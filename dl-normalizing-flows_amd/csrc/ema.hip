// Weight averaging (include/realnvp_hip.h, "weight averaging"): the
// exponential moving average of the parameter arena, kept by the training
// step itself, and the in-place exchange that lets evaluation read it.
//
//   k_ema_update   one pass over the arena: e += (1 - d) (p - e); a skipped or
//                  held step (ctl->skip) touches nothing
//   k_ema_swap     a <-> b
//
// Both take k_grad_sumsq's shape (step_ctl.hip): a capped grid, 16-byte
// granules, EMA_U granules' loads in flight per thread, a clamped tail.  No
// LDS, no atomics: an element is read and written by one thread.
#include "common.h"

// The update is three separately rounded fp32 operations (sub, mul, add), so
// that it can be reproduced bit for bit with any IEEE fp32 arithmetic; a
// contraction into an fma would round twice instead of three times.
#pragma clang fp contract(off)

namespace {

constexpr int EMA_THREADS = 256;
constexpr int EMA_MAX_BLOCKS = 2048;
constexpr int EMA_U = 4;          // granules in flight per thread and arena

__global__ __launch_bounds__(EMA_THREADS) void k_ema_update(floatx4* __restrict__ ema, const floatx4* __restrict__ p,
                                                            long long n4, rnvp_ema_ctl* __restrict__ ectl,
                                                            const long long* __restrict__ step, long long step_add,
                                                            const rnvp_step_ctl* __restrict__ ctl) {
    // a skipped step, or a held micro-step of an accumulating trainer: the
    // parameters did not move, and neither does their average
    if (ctl && ctl->skip) return;
    // the configuration and the step counter are read by every thread and
    // written by none (thread 0 below writes the two result fields only)
    float d = ectl->decay;
    if (ectl->warmup) {
        const float u = (float)(step[0] + step_add);
        d = fminf(d, (1.f + u) / (10.f + u));
    }
    const float om = 1.f - d;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ectl->applied = d;
        ectl->n_updates = ectl->n_updates + 1;
    }
    const long long stride = (long long)gridDim.x * EMA_THREADS;
    for (long long i0 = (long long)blockIdx.x * EMA_THREADS + threadIdx.x; i0 < n4; i0 += EMA_U * stride) {
        floatx4 E[EMA_U], P[EMA_U];
#pragma unroll
        for (int u = 0; u < EMA_U; ++u) {
            // an index past the end is clamped to the iteration's first granule and not stored
            const long long i = i0 + u * stride < n4 ? i0 + u * stride : i0;
            E[u] = ema[i];
            P[u] = p[i];
        }
#pragma unroll
        for (int u = 0; u < EMA_U; ++u) {
            floatx4 V;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float diff = P[u][e] - E[u][e];
                const float inc = om * diff;
                // (d == 0: e + (p - e) is p only where the subtraction is exact)
                V[e] = d == 0.f ? P[u][e] : E[u][e] + inc;
            }
            if (i0 + u * stride < n4) ema[i0 + u * stride] = V;
        }
    }
}

__global__ __launch_bounds__(EMA_THREADS) void k_ema_swap(floatx4* __restrict__ a, floatx4* __restrict__ b,
                                                          long long n4) {
    const long long stride = (long long)gridDim.x * EMA_THREADS;
    for (long long i0 = (long long)blockIdx.x * EMA_THREADS + threadIdx.x; i0 < n4; i0 += EMA_U * stride) {
        floatx4 A[EMA_U], B[EMA_U];
#pragma unroll
        for (int u = 0; u < EMA_U; ++u) {
            const long long i = i0 + u * stride < n4 ? i0 + u * stride : i0;
            A[u] = a[i];
            B[u] = b[i];
        }
#pragma unroll
        for (int u = 0; u < EMA_U; ++u)
            if (i0 + u * stride < n4) {
                a[i0 + u * stride] = B[u];
                b[i0 + u * stride] = A[u];
            }
    }
}

// [a, a + n) and [b, b + n) share an element (a == b included)
inline bool ema_overlap(const float* a, const float* b, long long n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    return x == y || (x < y ? y - x : x - y) < bytes;
}

}  // namespace

extern "C" int rnvp_ema_struct_size(void) { return (int)sizeof(rnvp_ema_ctl); }

extern "C" int rnvp_ema_update(float* ema, const float* param, long long n, rnvp_ema_ctl* ectl, const long long* step,
                               long long step_add, const rnvp_step_ctl* ctl, void* stream) {
    if (!ema || !param || !ectl || !step || n < 0 || (n & 3)) return RNVP_E_INVALID;
    if ((((uintptr_t)ema) | ((uintptr_t)param)) & 15) return RNVP_E_INVALID;
    if (((((uintptr_t)ectl) | ((uintptr_t)step)) & 7) || (ctl && (((uintptr_t)ctl) & 7))) return RNVP_E_INVALID;
    if (ema_overlap(ema, param, n)) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;
    k_ema_update<<<rnvp_grid(n / 4, EMA_THREADS, EMA_MAX_BLOCKS), EMA_THREADS, 0, (hipStream_t)stream>>>(
        (floatx4*)ema, (const floatx4*)param, n / 4, ectl, step, step_add, ctl);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_ema_swap(float* a, float* b, long long n, void* stream) {
    if (!a || !b || n < 0 || (n & 3)) return RNVP_E_INVALID;
    if ((((uintptr_t)a) | ((uintptr_t)b)) & 15) return RNVP_E_INVALID;
    if (ema_overlap(a, b, n)) return RNVP_E_INVALID;
    if (n == 0) return RNVP_OK;
    k_ema_swap<<<rnvp_grid(n / 4, EMA_THREADS, EMA_MAX_BLOCKS), EMA_THREADS, 0, (hipStream_t)stream>>>(
        (floatx4*)a, (floatx4*)b, n / 4);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}
