// Latents (include/realnvp_hip.h, "latents"): what a trained flow is used for
// after scoring -- prior draws that belong to the sample, the end of a decode
// into fp32 or bytes, and interpolation between latents.  One device-resident
// control block (rnvp_latent_ctl) carries what changes between replays.
//   k_latent_draw     z = temperature * N(0, 1), one Philox4x32-10 call per element
//   k_latent_out      the inverse logit transform of the valid rows, stored as
//                     fp32 / rounded bytes / floored bytes at their global index
//   k_latent_advance  one workgroup, behind the rows: the block's counters
//   k_mix_dots        per pair a.b, |a|^2, |b|^2 in fp64
//   k_mix_apply       the lerp / slerp weights per (pair, t) in fp64, applied in fp32
#include <limits.h>
#include <math.h>

#include "common.h"

// Philox4x32-10 (Salmon et al. 2011) with all four output words; the round
// function of flow_ops.hip's philox_uniform, counter = (ctr, 0, 0), key = seed
__device__ __forceinline__ void philox4x32(uint64_t seed, uint64_t ctr, uint32_t (&w)[4]) {
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
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

extern "C" int rnvp_latent_struct_size(void) { return (int)sizeof(rnvp_latent_ctl); }

// ---------------------------------------------------------------------------
// the prior draw: element e of row b is a function of (seed, (first + b) n + e,
// temperature) and of nothing else (Box-Muller on the first two words, the
// cosine branch only: one call per element, no pairing with a neighbour)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_latent_draw(float* __restrict__ z, uint64_t seed,
                                                     const rnvp_latent_ctl* __restrict__ ctl, long long total,
                                                     long long n) {
    const float T = ctl->temperature;
    const uint64_t base = (uint64_t)ctl->first * (uint64_t)n;   // row b, element e: base + b n + e
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += stride) {
        uint32_t w[4];
        philox4x32(seed, base + (uint64_t)i, w);
        const float u1 = (float)((w[0] >> 8) + 1u) * (1.0f / 16777216.0f);   // (0, 1]
        const float u2 = (float)(w[1] >> 8) * (1.0f / 16777216.0f);          // [0, 1)
        const float g = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        z[i] = T * g;
    }
}

extern "C" int rnvp_latent_draw(float* z, uint64_t seed, const rnvp_latent_ctl* ctl, int B, long long n, void* stream) {
    if (!z || !ctl || B < 0 || n < 0) return RNVP_E_INVALID;
    if ((((uintptr_t)z) & 3) || (((uintptr_t)ctl) & 7)) return RNVP_E_INVALID;
    if (B > 0 && n > LLONG_MAX / B) return RNVP_E_INVALID;
    const long long total = (long long)B * n;
    if (total == 0) return RNVP_OK;
    k_latent_draw<<<rnvp_grid(total, 256, 1 << 16), 256, 0, (hipStream_t)stream>>>(z, seed, ctl, total, n);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// the end of a decode
// ---------------------------------------------------------------------------
// rnvp_logit_inv's value (flow_ops.hip: k_logit_inv), the same operations in the same order
__device__ __forceinline__ float logit_inv_elem(float x, float cst) {
    float v = 1.f / (expf(-x) + 1.f);
    return ((v * 2.f - 1.f) / cst + 1.f) / 2.f;
}
// torchvision.utils.save_image: mul(255).add(0.5).clamp(0, 255).to(uint8), each step rounded on its own
__device__ __forceinline__ uint32_t quant_round(float v) {
    const float t = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
    return (uint32_t)fminf(fmaxf(t, 0.f), 255.f);
}
// the inverse of the dequantisation (k + u) / 256: min(255, floor(256 clamp(v, 0, 1)))
__device__ __forceinline__ uint32_t quant_floor(float v) {
    return (uint32_t)fminf(256.f * fminf(fmaxf(v, 0.f), 1.f), 255.f);
}

// grid (B, chunks of a row); 256 threads, a group of 4 elements per thread and trip
template <int MODE>
__global__ __launch_bounds__(256) void k_latent_out(const float* __restrict__ x,
                                                    const rnvp_latent_ctl* __restrict__ ctl, float cst, long long n) {
    const int b = blockIdx.x;
    if (b >= ctl->n_valid) return;              // a padding row
    const long long at = ctl->first + b;
    if (at < 0 || at >= ctl->cap) return;       // past the destination: k_latent_advance sets overflow
    const float* xb = x + (long long)b * n;
    const long long stride = (long long)gridDim.y * blockDim.x;
    const long long t0 = blockIdx.y * (long long)blockDim.x + threadIdx.x;
    if (MODE == RNVP_OUT_F32) {
        float* d = (float*)ctl->dst + at * n;
        for (long long e = t0; e < n; e += stride) d[e] = logit_inv_elem(xb[e], cst);
    } else {
        // the row starts at any byte address: group 0 is the `head` bytes in front of the first 4-byte
        // boundary, group g >= 1 the aligned word at head + 4 (g - 1) (bytes again where the row ends inside it)
        uint8_t* d = (uint8_t*)ctl->dst + at * n;
        const long long head = (long long)((4 - (((uintptr_t)d) & 3)) & 3);
        const long long groups = 1 + (n > head ? (n - head + 3) / 4 : 0);
        for (long long g = t0; g < groups; g += stride) {
            const long long e0 = g == 0 ? 0 : head + 4 * (g - 1);
            const long long e1 = min(n, g == 0 ? head : e0 + 4);
            uint32_t q[4] = {0, 0, 0, 0};
            for (long long e = e0; e < e1; ++e) {
                const float v = logit_inv_elem(xb[e], cst);
                q[e - e0] = MODE == RNVP_OUT_U8_ROUND ? quant_round(v) : quant_floor(v);
            }
            if (g > 0 && e1 - e0 == 4) {
                *(uint32_t*)(d + e0) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            } else {
                for (long long e = e0; e < e1; ++e) d[e] = (uint8_t)q[e - e0];
            }
        }
    }
}

__global__ void k_latent_advance(rnvp_latent_ctl* ctl, int B) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long nv = max(0, min(ctl->n_valid, B));
    const long long first = ctl->first, cap = ctl->cap;
    // rows b < nv with 0 <= first + b < cap were stored
    const long long lo = max(first, 0LL), hi = min(first + nv, cap);
    if (first + nv > cap) ctl->overflow = 1;
    ctl->n_done = ctl->n_done + (hi > lo ? hi - lo : 0);
    ctl->first = first + nv;
}

extern "C" int rnvp_latent_out(const float* x, rnvp_latent_ctl* ctl, float constraint, int B, long long n, int mode,
                               void* stream) {
    if (!x || !ctl || B < 0 || n < 0) return RNVP_E_INVALID;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)ctl) & 7)) return RNVP_E_INVALID;
    if (mode != RNVP_OUT_F32 && mode != RNVP_OUT_U8_ROUND && mode != RNVP_OUT_U8_FLOOR) return RNVP_E_INVALID;
    if (B > 0 && n > LLONG_MAX / B) return RNVP_E_INVALID;
    if (B == 0 || n == 0) return RNVP_OK;
    hipStream_t s = (hipStream_t)stream;
    const long long work = mode == RNVP_OUT_F32 ? n : n / 4 + 2;
    const dim3 grid(B, rnvp_grid(work, 256, 256));
    if (mode == RNVP_OUT_F32)
        k_latent_out<RNVP_OUT_F32><<<grid, 256, 0, s>>>(x, ctl, constraint, n);
    else if (mode == RNVP_OUT_U8_ROUND)
        k_latent_out<RNVP_OUT_U8_ROUND><<<grid, 256, 0, s>>>(x, ctl, constraint, n);
    else
        k_latent_out<RNVP_OUT_U8_FLOOR><<<grid, 256, 0, s>>>(x, ctl, constraint, n);
    RNVP_LAUNCH_CHECK();
    k_latent_advance<<<1, 64, 0, s>>>(ctl, B);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// ---------------------------------------------------------------------------
// interpolation
// ---------------------------------------------------------------------------
constexpr long long MIX_CHUNK = 16384;   // elements of a pair per workgroup of k_mix_dots
constexpr int MIX_CHUNKS_MAX = 8;        // so at most 8 fp64 atomics meet on one address

// grid (P, chunks).  One chunk (n <= MIX_CHUNK: every image up to 3 x 64 x 64
// and beyond) stores its sums, no atomic at all; more add their partials to
// the zeroed workspace, one atomic per workgroup and sum.
__global__ __launch_bounds__(512) void k_mix_dots(const float* __restrict__ a, const float* __restrict__ b,
                                                  double* __restrict__ ws, long long n, long long chunk) {
    __shared__ double red[16];
    const long long p = blockIdx.x, i0 = blockIdx.y * chunk, i1 = min(n, i0 + chunk);
    const float* ap = a + p * n;
    const float* bp = b + p * n;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (long long i = i0 + threadIdx.x; i < i1; i += 512) {
        const double x = (double)ap[i], y = (double)bp[i];
        ab += x * y;
        aa += x * x;
        bb += y * y;
    }
    ab = block_sum(ab, red);
    aa = block_sum(aa, red);
    bb = block_sum(bb, red);
    if (threadIdx.x != 0) return;
    double* w = ws + 3 * p;
    if (gridDim.y == 1) {
        w[0] = ab; w[1] = aa; w[2] = bb;
    } else {
        atomicAdd(&w[0], ab);
        atomicAdd(&w[1], aa);
        atomicAdd(&w[2], bb);
    }
}

// grid (P * T, chunks of n): the weights of (pair p, step j) once per workgroup
__global__ __launch_bounds__(256) void k_mix_apply(const float* __restrict__ a, const float* __restrict__ b,
                                                   const float* __restrict__ t, float* __restrict__ out,
                                                   const double* __restrict__ ws, int T, long long n, int mode) {
    __shared__ float wgt[2];
    const long long row = blockIdx.x, p = row / T;
    const int j = (int)(row - p * T);
    if (threadIdx.x == 0) {
        const double tt = (double)t[j];
        double wa = 1.0 - tt, wb = tt;
        if (mode == RNVP_MIX_SLERP) {
            const double ab = ws[3 * p], na = sqrt(ws[3 * p + 1]), nb = sqrt(ws[3 * p + 2]);
            if (na > 0.0 && nb > 0.0) {
                const double c = fmin(fmax(ab / (na * nb), -1.0), 1.0);
                if (!(1.0 - fabs(c) < 1e-9)) {
                    const double om = acos(c), so = sin(om);
                    wa = sin((1.0 - tt) * om) / so;
                    wb = sin(tt * om) / so;
                }
            }
        }
        wgt[0] = (float)wa;
        wgt[1] = (float)wb;
    }
    __syncthreads();
    const float wa = wgt[0], wb = wgt[1];
    const float* ap = a + p * n;
    const float* bp = b + p * n;
    float* o = out + row * n;
    const long long stride = (long long)gridDim.y * blockDim.x;
    for (long long e = blockIdx.y * (long long)blockDim.x + threadIdx.x; e < n; e += stride)
        o[e] = __fadd_rn(__fmul_rn(wa, ap[e]), __fmul_rn(wb, bp[e]));
}

extern "C" int rnvp_latent_mix(const float* a, const float* b, const float* t, float* out, int P, int T, long long n,
                               int mode, double* ws, void* stream) {
    if (!a || !b || !t || !out || P < 0 || T < 0 || n < 0) return RNVP_E_INVALID;
    if (mode != RNVP_MIX_LERP && mode != RNVP_MIX_SLERP) return RNVP_E_INVALID;
    if (mode == RNVP_MIX_SLERP && !ws) return RNVP_E_INVALID;
    if (((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)t) | ((uintptr_t)out)) & 3) || (((uintptr_t)ws) & 7))
        return RNVP_E_INVALID;
    const long long rows = (long long)P * T;
    if (rows > 0x7fffffffLL || (rows > 0 && n > LLONG_MAX / rows)) return RNVP_E_INVALID;
    if (rows == 0 || n == 0) return RNVP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (mode == RNVP_MIX_SLERP) {
        long long chunks = (n + MIX_CHUNK - 1) / MIX_CHUNK;
        if (chunks > MIX_CHUNKS_MAX) chunks = MIX_CHUNKS_MAX;
        const long long chunk = (n + chunks - 1) / chunks;
        if (chunks > 1) {
            hipError_t e = hipMemsetAsync(ws, 0, sizeof(double) * 3 * (size_t)P, s);
            if (e != hipSuccess) return (int)e;
        }
        k_mix_dots<<<dim3(P, (unsigned)chunks), 512, 0, s>>>(a, b, ws, n, chunk);
        RNVP_LAUNCH_CHECK();
    }
    k_mix_apply<<<dim3((unsigned)rows, rnvp_grid(n, 256, 64)), 256, 0, s>>>(a, b, t, out, ws, T, n, mode);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}
