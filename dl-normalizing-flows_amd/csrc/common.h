// Shared device helpers for the RealNVP MI355X (gfx950) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "realnvp_hip.h"

typedef uint16_t bf16_t;                                        // bf16 storage
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));      // MFMA operand
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define RNVP_LDS __attribute__((address_space(3)))
// global-memory view of a pointer read from memory (a descriptor table):
// accesses through it compile to global_* instead of flat_* operations (a
// flat operation also counts on lgkmcnt, so LDS waits wait for it as well)
#define RNVP_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }

// scalar load/store of a net-activation element as float
__device__ __forceinline__ float ldv(const float* p) { return *p; }
__device__ __forceinline__ float ldv(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void stv(float* p, float v) { *p = v; }
__device__ __forceinline__ void stv(bf16_t* p, float v) { *p = f2bf(v); }

// elements per 16-byte chunk
template <typename T> struct Chunk;
template <> struct Chunk<float> { static constexpr int N = 4; };
template <> struct Chunk<bf16_t> { static constexpr int N = 8; };

// unpack / pack one 16-byte chunk
__device__ __forceinline__ void unpack(const u32x4& c, float* v, float) {
    v[0] = __uint_as_float(c.x); v[1] = __uint_as_float(c.y);
    v[2] = __uint_as_float(c.z); v[3] = __uint_as_float(c.w);
}
__device__ __forceinline__ void unpack(const u32x4& c, float* v, bf16_t) {
    uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ u32x4 pack(const float* v, float) {
    u32x4 c;
    c.x = __float_as_uint(v[0]); c.y = __float_as_uint(v[1]);
    c.z = __float_as_uint(v[2]); c.w = __float_as_uint(v[3]);
    return c;
}
__device__ __forceinline__ u32x4 pack(const float* v, bf16_t) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
    u32x4 c;
    c.x = w[0]; c.y = w[1]; c.z = w[2]; c.w = w[3];
    return c;
}

// 4 consecutive elements (8 B of bf16 / 16 B of f32) <-> float[4]
__device__ __forceinline__ void ld4(const float* p, float* v) {
    const floatx4 t = *(const floatx4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ld4(const bf16_t* p, float* v) {
    const uint2 t = *(const uint2*)p;
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ __forceinline__ void st4(float* p, const float* v) { *(floatx4*)p = floatx4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void st4(bf16_t* p, const float* v) {
    uint2 t;
    t.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    t.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    *(uint2*)p = t;
}

// load / store through a global-memory view (pointers read from descriptor tables)
__device__ __forceinline__ float ldg(const RNVP_GLOBAL float* p) { return *p; }
__device__ __forceinline__ float ldg(const RNVP_GLOBAL bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void stg(float* p, float v) { *(RNVP_GLOBAL float*)p = v; }
__device__ __forceinline__ void stg(bf16_t* p, float v) { *(RNVP_GLOBAL bf16_t*)p = f2bf(v); }

// one element of torch.optim.Adam (single-tensor form, coupled L2 weight
// decay, train.py:134); f = 2 adds the 5e-5 * weight_scale regulariser's
// gradient 2*reg*p (train.py:194).  m, v updated in place; returns p'.
// step_size = lr / (1 - b1^t), inv_bc2s = 1 / sqrt(1 - b2^t).
// Every multiply-add is an explicit fmaf and no other product feeds an
// addition, so no FMA contraction is left to the compiler: the kernels that
// inline this (k_adam, k_adam_gather, k_wn_adam) compute bitwise the same
// update from the same operands.
// c = the step control's grad_scale (clip_grad_norm_'s factor on the whole
// p.grad: g and the regulariser's gradient, not Adam's weight decay).  c g and
// 2 reg c are single roundings that are exact for c = 1.0f, so the unclipped
// update keeps its bits.  The rounding error of c g (fmaf(c, g, -cg), exact;
// 0 for c = 1.0f) is added back after the weight-decay FMA: where wd p and
// c g nearly cancel (0.3 % of a real gradient arena) it is all that is left
// of the product's low bits, and gr stays within two roundings of ITSELF
// instead of one rounding of c g.  SCALED = false (no step control) is the
// unscaled update itself: the kernels instantiate both, so a launch without
// a control block runs the code it always ran.
template <bool SCALED = false>
__device__ __forceinline__ float adam_elem(float p, float g, float& m, float& v, int f, float b1, float b2, float eps,
                                           float wd, float reg, float step_size, float inv_bc2s, float c = 1.0f) {
    float gr;
    if (SCALED) {
        const float cg = c * g;
        gr = fmaf(wd, p, cg) + fmaf(c, g, -cg);
        if (f == 2) gr = fmaf(2.f * reg * c, p, gr);
    } else {
        gr = fmaf(wd, p, g);
        if (f == 2) gr = fmaf(2.f * reg, p, gr);
    }
    m = fmaf(1.f - b1, gr - m, m);
    const float t = (1.f - b2) * gr;
    v = fmaf(v, b2, t * gr);
    const float den = fmaf(sqrtf(v), inv_bc2s, eps);
    return p - (step_size * m) / den;
}

// The per-launch scalars of the Adam kernels, by one thread into LDS:
// coef = {lr / (1 - b1^t), 1 / sqrt(1 - b2^t), gradient scale}, t = *step +
// step_add; the learning rate and the scale come from the step control when
// there is one (rnvp_adam_args.ctl).
__device__ __forceinline__ void adam_coef(const long long* step, long long step_add, float lr, float b1, float b2,
                                          const rnvp_step_ctl* ctl, float* coef) {
    const double t = (double)(step[0] + step_add);
    const double bc1 = 1.0 - pow((double)b1, t), bc2 = 1.0 - pow((double)b2, t);
    coef[0] = (float)((ctl ? ctl->lr : lr) / bc1);
    coef[1] = (float)(1.0 / sqrt(bc2));
    coef[2] = ctl ? ctl->grad_scale : 1.0f;
}
// a skipped step (non-finite gradient norm): the Adam kernels touch nothing
__device__ __forceinline__ bool adam_skipped(const rnvp_step_ctl* ctl) { return ctl && ctl->skip; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the 16 lanes of a DPP row (lanes 16r .. 16r+15 = one MFMA column
// group); every lane of the row gets the result.  row_ror butterfly on the
// VALU (no LDS round trip: __shfl_xor lowers to ds_bpermute).
// (every lane of a row_ror / quad_perm has a source lane: bound_ctrl leaves the
// move no `old` operand to zero first)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_f<0x128>(v); v += dpp_f<0x124>(v); v += dpp_f<0x122>(v); v += dpp_f<0x121>(v);
    return v;
}
__device__ __forceinline__ double row_sum16(double v) {
    v += dpp_d<0x128>(v); v += dpp_d<0x124>(v); v += dpp_d<0x122>(v); v += dpp_d<0x121>(v);
    return v;
}

// ---- transposing row reduction ---------------------------------------------
// Several values per lane summed over the 16 lanes of a DPP row as a
// reduce-scatter: at lane distance 8, 4, 2, 1 a lane keeps one half of its
// values, adds its partner's copies of them and hands the other half over,
// until one value is left (15 adds for 16 values; row_sum16 on each spends
// 64).  The pairs are row_sum16's -- lane i with i ^ 8, then (i, i ^ 8) with
// (i ^ 4, i ^ 12), then the lanes that differ in bit 1, then bit 0 -- and IEEE
// addition commutes, so every total is bitwise what row_sum16 leaves in lane 0
// (tools/probe/row_reduce_check.hip).
//
// dpp_into: the lanes of the 4-lane banks in BANK (lanes 4b .. 4b+3 are bank b)
// take v from their CTRL source lane, the others keep `old`: the move is the
// select.
template <int CTRL, int BANK>
__device__ __forceinline__ float dpp_into(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, 0xf, BANK, false));
}
template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_into(double old, double v) {
    const unsigned long long o = (unsigned long long)__double_as_longlong(old);
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)u, CTRL, 0xf, BANK, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(u >> 32), CTRL, 0xf, BANK, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// One distance D (4, 2 or 1) of the reduction on v[0 .. n): n >= 2 halves the
// array (a lane whose index has bit D clear keeps v[k], one with it set keeps
// v[k + n/2], k < n/2, in v[k]); n == 1 (distance 1 only: the two lanes of a
// pair hold the same slot) is the plain butterfly.  Distance 4 is row_shl:4 /
// row_shr:4, each written into the lanes of one side by bank mask; distances 2
// and 1 are the quad_perm swaps, with the halves chosen by select.
template <int D, int n>
__device__ __forceinline__ void row_reduce_step(double* v, int li) {
    static_assert(D == 4 || D == 2 || D == 1, "distance 8 is row_stats16's first step");
    if constexpr (n >= 2) {
        constexpr int h = n / 2;
#pragma unroll
        for (int k = 0; k < h; ++k) {
            const double lo = v[k], hi = v[k + h];
            if constexpr (D == 4) {
                v[k] = dpp_into<0x104, 0x5>(hi, lo) + dpp_into<0x114, 0xa>(lo, hi);
            } else {
                const bool up = (li & D) != 0;
                const double send = up ? lo : hi, keep = up ? hi : lo;
                v[k] = keep + (D == 2 ? dpp_d<0x4e>(send) : dpp_d<0xb1>(send));
            }
        }
    } else {
        static_assert(n >= 2 || D == 1, "one value left before distance 1");
        v[0] += dpp_d<0xb1>(v[0]);
    }
}

// The conv epilogues' statistics tail: a thread's partial sums s1[J][4] /
// s2[J][4] (J column groups of 4 channels; 8, 16 or 32 values a round) reduced
// over the row together, and park(j, r, which, total) called in the ONE lane
// that ends up owning column (j, r)'s sum (which = 0) or sum of squares
// (which = 1) -- where lane 0 used to park all 8 J of them.  Input order
// (j * 4 + r) * 2 + which.  Distance 8 (row_ror:8, by bank mask) moves the
// partials as they are -- fp32 ones one move each -- and widens them on
// arrival: (double)a + (double)b either way.  Every lane of the row must be
// active.
template <int J0, int J, typename F, typename Park>
__device__ __forceinline__ void row_stats16_from(const F (&s1)[J][4], const F (&s2)[J][4], int li, Park&& park) {
    constexpr int REM = J - J0;
    constexpr int P = REM >= 4 ? 4 : (REM >= 2 ? 2 : 1);   // column groups in this round
    constexpr int N = 8 * P, H = N / 2;
    F w[N];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            w[(j * 4 + r) * 2] = s1[J0 + j][r];
            w[(j * 4 + r) * 2 + 1] = s2[J0 + j][r];
        }
    double v[H];
#pragma unroll
    for (int k = 0; k < H; ++k)
        v[k] = (double)dpp_into<0x128, 0x3>(w[k + H], w[k]) + (double)dpp_into<0x128, 0xc>(w[k], w[k + H]);
    row_reduce_step<4, H>(v, li);
    row_reduce_step<2, H / 2>(v, li);
    row_reduce_step<1, (H >= 8 ? H / 4 : 1)>(v, li);
    if constexpr (N == 32) {          // lane li: both sums of column li
        park(J0 + (li >> 2), li & 3, 0, v[0]);
        park(J0 + (li >> 2), li & 3, 1, v[1]);
    } else if constexpr (N == 16) {   // lane li: column li / 2, sum li & 1
        park(J0 + (li >> 3), (li >> 1) & 3, li & 1, v[0]);
    } else {                          // lanes 2i, 2i + 1: column i / 2, sum i & 1
        if (!(li & 1)) park(J0, li >> 2, (li >> 1) & 1, v[0]);
    }
    if constexpr (J0 + P < J) row_stats16_from<J0 + P>(s1, s2, li, park);
}
template <int J, typename F, typename Park>
__device__ __forceinline__ void row_stats16(const F (&s1)[J][4], const F (&s2)[J][4], int li, Park&& park) {
    row_stats16_from<0>(s1, s2, li, park);
}

// block-wide sum (blockDim.x multiple of 64, <= 1024); every thread gets the result
template <typename F>
__device__ __forceinline__ F block_sum(F v, F* red /* >= 16 entries of LDS */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    F t = 0;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// per-channel BN affine (scale, shift) such that bn(x) = x*scale + shift:
// the alpha/beta form ATen's batch_norm applies (the reference's own
// arithmetic; a centred (x - mean)*scale + beta form was measured further
// from the fp64 truth on the deep goldens, whose near-degenerate channels
// make ReLU decisions rounding-sensitive)
__device__ __forceinline__ void bn_affine(const rnvp_bn_src& s, int C, int c, float& scale, float& shift,
                                          float* mean_out = nullptr, float* rstd_out = nullptr) {
    double mean, var;
    if (s.sums) {
        // shards <= 32 (rnvp_stat_shards, RNVP_COUPLING_SHARDS): every load is
        // issued up front (clamped address, masked contribution), then added in
        // shard order -- one memory round trip instead of one per shard
        double v1[32], v2[32];
        const int ns = s.shards > 0 ? s.shards : 1;
#pragma unroll
        for (int h = 0; h < 32; ++h) {
            const long long o = (long long)(h < ns ? h : 0) * 2 * C;
            v1[h] = s.sums[o + c];
            v2[h] = s.sums[o + C + c];
        }
        double s1 = 0, s2 = 0;
#pragma unroll
        for (int h = 0; h < 32; ++h) {
            if (h < ns) {
                s1 += v1[h];
                s2 += v2[h];
            }
        }
        mean = s1 / s.count;
        var = s2 / s.count - mean * mean;
        if (var < 0) var = 0;
    } else {
        mean = s.mean[c];
        var = s.var[c];
    }
    float rstd = (float)(1.0 / sqrt(var + (double)s.eps));
    float g = s.gamma ? s.gamma[c] : 1.f;
    float b = s.beta ? s.beta[c] : 0.f;
    scale = g * rstd;
    shift = b - (float)mean * g * rstd;
    if (mean_out) *mean_out = (float)mean;
    if (rstd_out) *rstd_out = rstd;
}

// Whole-block reduction of sharded BN sums ([shards][2*C] fp64) for channels
// [c0, c0+nc) into LDS s1[nc], s2[nc]; up to two independent sources in one
// pass.  Every (channel, shard) pair is a separate load spread over the block;
// a thread issues up to 4 pairs' loads at once (the first round before the
// barrier that zeroes the outputs), then accumulates them with LDS fp64
// atomics (ds_add_f64).  Must be reached by every thread of the block.
struct ShardSrc {
    const double* sums; int C, shards, c0, nc; double* s1; double* s2;
};

template <int NS>
__device__ __forceinline__ void block_shard_sums_n(const ShardSrc (&src)[NS]) {
    constexpr int U = 4;
    int total[NS], tmax = 0;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        total[q] = src[q].sums ? src[q].nc * (src[q].shards < 1 ? 1 : src[q].shards) : 0;
        tmax = max(tmax, total[q]);
    }
    auto zero = [&]() {
#pragma unroll
        for (int q = 0; q < NS; ++q)
            for (int i = threadIdx.x; i < src[q].nc; i += blockDim.x) {
                src[q].s1[i] = 0.0;
                src[q].s2[i] = 0.0;
            }
        __syncthreads();
    };
    if (tmax <= 0) zero();
    for (int t0 = 0; t0 < tmax; t0 += U * blockDim.x) {
        double v1[NS][U], v2[NS][U];
        int cc[NS][U];
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * blockDim.x + threadIdx.x;
                cc[q][u] = -1;
                v1[q][u] = v2[q][u] = 0.0;
                if (t < total[q]) {
                    const int c = t % src[q].nc, h = t / src[q].nc;
                    const double* p = src[q].sums + (long long)h * 2 * src[q].C + src[q].c0 + c;
                    v1[q][u] = p[0];
                    v2[q][u] = p[src[q].C];
                    cc[q][u] = c;
                }
            }
        if (t0 == 0) zero();
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (cc[q][u] >= 0) {
                    atomicAdd(&src[q].s1[cc[q][u]], v1[q][u]);
                    atomicAdd(&src[q].s2[cc[q][u]], v2[q][u]);
                }
    }
    __syncthreads();
}

__device__ __forceinline__ void block_shard_sums(const double* sums, int C, int shards, int c0, int nc, double* s1,
                                                 double* s2) {
    const ShardSrc src[1] = {{sums, C, shards, c0, nc, s1, s2}};
    block_shard_sums_n<1>(src);
}

// block_shard_sums split in two: shard_issue loads a thread's entries into
// registers (first thing in a kernel, ahead of its bulk loads: vmcnt waits in
// issue order), shard_finish folds them into s1 / s2 (LDS fp64 atomics, as
// block_shard_sums).  Needs nc * shards <= U * blockDim.x (shard_fits).
template <int U>
struct ShardLoads {
    double v1[U], v2[U];
    int cc[U];
};
__device__ __forceinline__ bool shard_fits(int nc, int shards, int U) {
    return (long long)nc * (shards < 1 ? 1 : shards) <= (long long)U * blockDim.x;
}
template <int U>
__device__ __forceinline__ void shard_issue(const double* sums, int C, int shards, int c0, int nc, ShardLoads<U>& L) {
    const int total = nc * (shards < 1 ? 1 : shards);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // unconditional loads (an index past the table reads entry 0 and is
        // marked unused): no branch, so no wait is forced at its join
        const int t = u * blockDim.x + threadIdx.x;
        const bool ok = t < total;
        const int tt = ok ? t : 0;
        const int c = tt % nc, h = tt / nc;
        const double* p = sums + (long long)h * 2 * C + c0 + c;
        L.v1[u] = p[0];
        L.v2[u] = p[C];
        L.cc[u] = ok ? c : -1;
    }
}
template <int U>
__device__ __forceinline__ void shard_finish(const ShardLoads<U>& L, int nc, double* s1, double* s2) {
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        s1[i] = 0.0;
        s2[i] = 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (L.cc[u] >= 0) {
            atomicAdd(&s1[L.cc[u]], L.v1[u]);
            atomicAdd(&s2[L.cc[u]], L.v2[u]);
        }
    __syncthreads();
}

// shard_finish without zeroing and without LDS atomics: every thread parks
// its loaded entries in tab (2 * U * blockDim.x doubles of LDS) at their
// entry index h * nc + c, ONE barrier, then thread c < nc adds channel c's
// shards in shard order into s1[c] / s2[c] (deterministic).  No branch and no
// loop sits between the shard loads and their first use, so the wait for
// them counts only the loads issued before them (the tile loads a kernel
// issued after them stay in flight).  The sums are left for the SAME thread
// (block_bn_finish_aff reads entry threadIdx.x): no trailing barrier.
// Needs nc <= blockDim.x and shard_fits(nc, shards, U).
template <int U>
__device__ __forceinline__ void shard_sum_tab(const ShardLoads<U>& L, int nc, int shards, double* tab, double* s1,
                                              double* s2) {
    const int n = U * blockDim.x;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = u * blockDim.x + threadIdx.x;
        tab[t] = L.v1[u];
        tab[n + t] = L.v2[u];
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < nc) {
        const int hs = shards < 1 ? 1 : shards;
        double a = 0.0, b = 0.0;
        for (int h = 0; h < hs; ++h) {
            a += tab[h * nc + i];
            b += tab[n + h * nc + i];
        }
        s1[i] = a;
        s2[i] = b;
    }
}

// Affine parameters of channel c0 + threadIdx.x, loaded into registers with
// a prologue's other loads (bn_aff_issue) so that the table finish below
// waits on no global load.  No branch: an absent gamma / beta reads `any` (a
// valid global address of the same launch, value unused) and the finish
// applies the default 1 / 0.
struct BnAff { float g, b; };
__device__ __forceinline__ BnAff bn_aff_issue(const rnvp_bn_src& s, int C, int c0, const void* any) {
    const int c = max(0, min(c0 + (int)threadIdx.x, C - 1));
    const float* gp = s.gamma ? s.gamma : (const float*)any;
    const float* bp = s.beta ? s.beta : (const float*)any;
    return BnAff{gp[s.gamma ? c : 0], bp[s.beta ? c : 0]};
}

// one channel of the BN table (i < nv: a real channel; else padding)
__device__ __forceinline__ void bn_finish_entry(const rnvp_bn_src& s, int c, int i, int nc, int nv, const double* tmp,
                                                float g, float b, float* scale, float* shift, float* mean_out,
                                                float* rstd_out) {
    float sc = 0.f, sf = 0.f, mo = 0.f, ro = 1.f;
    if (i < nv) {
        double mean, var;
        if (s.sums) {
            mean = tmp[i] / s.count;
            var = tmp[nc + i] / s.count - mean * mean;
            if (var < 0) var = 0;
        } else {
            mean = s.mean[c];
            var = s.var[c];
        }
        const float rstd = (float)(1.0 / sqrt(var + (double)s.eps));
        sc = g * rstd;
        sf = b - (float)mean * g * rstd;
        mo = (float)mean;
        ro = rstd;
    }
    scale[i] = sc;
    shift[i] = sf;
    if (mean_out) mean_out[i] = mo;
    if (rstd_out) rstd_out[i] = ro;
}

// BN table for channels [c0, c0+nc) from already-reduced sums tmp[0..nc) /
// tmp[nc..2nc) (train) or the running stats (eval): scale/shift such that
// bn(x) = x*scale + shift, plus mean / rstd when requested.  Channels >= C
// (padding) get scale = shift = 0, mean = 0, rstd = 1.
__device__ __forceinline__ void block_bn_finish(const rnvp_bn_src& s, int C, int c0, int nc, float* scale, float* shift,
                                                float* mean_out, float* rstd_out, const double* tmp) {
    const int nv = max(0, min(nc, C - c0));
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        const int c = c0 + i;
        const float g = (i < nv && s.gamma) ? s.gamma[c] : 1.f;
        const float b = (i < nv && s.beta) ? s.beta[c] : 0.f;
        bn_finish_entry(s, c, i, nc, nv, tmp, g, b, scale, shift, mean_out, rstd_out);
    }
    __syncthreads();
}

// block_bn_finish for nc <= blockDim.x with the affine parameters in
// registers (bn_aff_issue(s, C, c0, ...))
__device__ __forceinline__ void block_bn_finish_aff(const rnvp_bn_src& s, int C, int c0, int nc, float* scale,
                                                    float* shift, float* mean_out, float* rstd_out, const double* tmp,
                                                    BnAff A) {
    const int nv = max(0, min(nc, C - c0));
    const int i = threadIdx.x;
    if (i < nc)
        bn_finish_entry(s, c0 + i, i, nc, nv, tmp, s.gamma ? A.g : 1.f, s.beta ? A.b : 0.f, scale, shift, mean_out,
                        rstd_out);
    __syncthreads();
}

// ---- finalized BN tables (rnvp_bn_src.tab: [C][4] fp32) --------------------
// entry {mean, rstd | mean, rstd}: flavour 0 has mean = sum * (1 / count)
// (tab_finish), flavour 1 mean = sum / count (every other reader); a reader
// forms scale = gamma rstd and shift = beta - mean gamma rstd in fp32 from its
// flavour, exactly as from its own shard reduction
enum { BN_TAB_MUL = 0, BN_TAB_DIV = 1 };
typedef float bn_f32x2 __attribute__((ext_vector_type(2)));
struct BnEntry { float scale, shift, mean, rstd; };
__device__ __forceinline__ BnEntry bn_entry(float mean, float rstd, float g, float b) {
    return BnEntry{g * rstd, b - mean * g * rstd, mean, rstd};
}
// channel c's {mean, rstd} of a finalized table (c clamped into the table: no branch)
__device__ __forceinline__ bn_f32x2 bn_tab_load(const float* tab, int C, int c, int flavour) {
    return *(const bn_f32x2*)(tab + (long long)max(0, min(c, C - 1)) * 4 + 2 * flavour);
}
// padding channels (>= C) of an LDS table: scale = shift = 0, mean = 0, rstd = 1
__device__ __forceinline__ void bn_entry_store(const BnEntry& e, bool valid, int i, float* scale, float* shift,
                                               float* mean_out, float* rstd_out) {
    scale[i] = valid ? e.scale : 0.f;
    shift[i] = valid ? e.shift : 0.f;
    if (mean_out) mean_out[i] = valid ? e.mean : 0.f;
    if (rstd_out) rstd_out[i] = valid ? e.rstd : 1.f;
}
// LDS table of channels [c0, c0+nc) from the finalized table: one 8-byte
// load per channel (+ the affine), no reduction, no fp64, ONE barrier
// (block_bn_table's result)
__device__ __forceinline__ void block_bn_load(const rnvp_bn_src& s, int C, int c0, int nc, float* scale, float* shift,
                                              float* mean_out, float* rstd_out, int flavour = BN_TAB_DIV) {
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        const int c = max(0, min(c0 + i, C - 1));
        const bn_f32x2 mr = bn_tab_load(s.tab, C, c, flavour);
        const float g = s.gamma ? s.gamma[c] : 1.f, b = s.beta ? s.beta[c] : 0.f;
        bn_entry_store(bn_entry(mr.x, mr.y, g, b), c0 + i < C, i, scale, shift, mean_out, rstd_out);
    }
    __syncthreads();
}

// The finalized-table form of shard_issue: thread i < nc loads channel
// c0 + i's {mean, rstd} (flavour BN_TAB_DIV) into slot 0 of its ShardLoads --
// registers the shard path would have used, so a kernel that takes either
// path by a uniform branch holds no more -- and tabf_entry forms the entry
// with the affine parameters of bn_aff_issue.  The 8 bytes travel as one
// double's bit pattern (moves only).
template <int U>
__device__ __forceinline__ void tabf_issue(const float* tab, int C, int c0, int nc, ShardLoads<U>& L) {
    const int i = (int)threadIdx.x < nc ? (int)threadIdx.x : 0;
    L.v1[0] = *(const double*)(tab + (long long)max(0, min(c0 + i, C - 1)) * 4 + 2 * BN_TAB_DIV);
}
template <int U>
__device__ __forceinline__ BnEntry tabf_entry(const ShardLoads<U>& L, const rnvp_bn_src& s, BnAff A) {
    const unsigned long long a = (unsigned long long)__double_as_longlong(L.v1[0]);
    return bn_entry(__uint_as_float((unsigned)a), __uint_as_float((unsigned)(a >> 32)), s.gamma ? A.g : 1.f,
                    s.beta ? A.b : 0.f);
}
// block_bn_finish_aff's result from tabf_issue's registers (nc <= blockDim.x);
// NO barrier: the caller's next one publishes the table
template <int U>
__device__ __forceinline__ void tabf_finish(const ShardLoads<U>& L, const rnvp_bn_src& s, BnAff A, int C, int c0,
                                            int nc, float* scale, float* shift, float* mean_out, float* rstd_out) {
    const int i = threadIdx.x;
    if (i < nc) bn_entry_store(tabf_entry(L, s, A), c0 + i < C, i, scale, shift, mean_out, rstd_out);
}

// The writer: one s/t-net BatchNorm site's running-statistics update (torch
// BatchNorm2d train-mode semantics) and, when r.tab is set, its finalized
// table, by one workgroup with the complete batch sums in hand.  tmp: 2*C
// doubles of LDS.  Must be reached by every thread of the block.
__device__ __forceinline__ void bn_running_site(const rnvp_bn_running& r, float mom, double* tmp) {
    const int C = r.C;
    // the shards added in shard order (what the register tables and
    // shard_sum_tab add: the result does not depend on an atomic's turn), 8
    // loads in flight at a time
    const int ns = r.shards < 1 ? 1 : r.shards;
    for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) {
        double acc = 0.0;
        for (int h0 = 0; h0 < ns; h0 += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = r.sums[(long long)min(h0 + u, ns - 1) * 2 * C + c];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (h0 + u < ns) acc += v[u];
        }
        tmp[c] = acc;
    }
    __syncthreads();
    const double inv = 1.0 / r.count;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const double s1 = tmp[c], s2 = tmp[C + c];
        const double mean = s1 / r.count;
        double var = s2 / r.count - mean * mean;
        if (var < 0) var = 0;
        const double unb = r.count > 1 ? var * r.count / (r.count - 1) : var;
        r.rmean[c] = (1.f - mom) * r.rmean[c] + mom * (float)mean;
        r.rvar[c] = (1.f - mom) * r.rvar[c] + mom * (float)unb;
        if (r.tab) {
            const double m0 = s1 * inv;
            double v0 = s2 * inv - m0 * m0;
            if (v0 < 0) v0 = 0;
            *(floatx4*)(r.tab + (long long)c * 4) =
                floatx4{(float)m0, (float)(1.0 / sqrt(v0 + (double)r.eps)), (float)mean,
                        (float)(1.0 / sqrt(var + (double)r.eps))};
        }
    }
    if (threadIdx.x == 0 && r.nbt) r.nbt[0] += 1;
}

// Whole-block BN table (shard reduction + finish).  tmp: 2*nc doubles of LDS.
// Must be reached by every thread of the block.
__device__ __forceinline__ void block_bn_table(const rnvp_bn_src& s, int C, int c0, int nc, float* scale, float* shift,
                                               float* mean_out, float* rstd_out, double* tmp) {
    if (s.tab) {
        block_bn_load(s, C, c0, nc, scale, shift, mean_out, rstd_out);
        return;
    }
    const int nv = max(0, min(nc, C - c0));
    if (s.sums) block_shard_sums(s.sums, C, s.shards, c0, nv, tmp, tmp + nc);
    block_bn_finish(s, C, c0, nc, scale, shift, mean_out, rstd_out, tmp);
}

static inline int rnvp_grid(long long n, int block, int cap = 4096) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

#define RNVP_LAUNCH_CHECK() do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return (int)e__; } while (0)
