// Generic grouped weight gradient of the s/t ResNet convolutions: reduces
// over pixels with both operands transposed through LDS
// (ds_read_b64_tr_b16 for bf16).  fp32 groups, and the bf16 groups the
// tap-shared kernel (wgrad_tap.hip) declines.
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"

namespace {

// ---------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------
// Output tile [64 co][64 k]; 4 waves as 2x2 of 32x32.  A stage is STG pixels
// (64 bf16 / 32 f32) of dy (P) and act(x) (Q), staged row-major [m][col] in
// double-buffered LDS; MFMA operands are columns, read transposed
// (ds_read_b64_tr_b16 for bf16).
struct WgView {
    const void* x; const void* dy; rnvp_bn_src pro;
    int H, W, ks, cs_in, cin, cs_dy, n, kp, pro_bn_relu;
};

// one [TC co] x [TC k] tile (TC = 64 or 128) over pixels [mb, me): result to out[co*kp + k]
// (fp32 atomics or plain stores) and, when bias_out, the bias sums of the
// tile's co columns to bias_out[co] (atomic or plain).
template <typename T, int TC>
__device__ __forceinline__ void wgrad_tile(const WgView& a, int co0, int k0, long long mb, long long me,
                                           long long M, float* out, bool atomic, float* bias_out, bool bias_atomic) {
    constexpr int CH = Mf<T>::CH;
    constexpr int STG = (sizeof(T) == 2) ? 64 : 32;   // pixels per stage (two MFMA K-steps)
    constexpr int CPR = TC / CH;                      // chunks per TC-column row
    constexpr int ROWB = TC * sizeof(T) + 16;         // padded row bytes
    constexpr int PER = STG * CPR / 256;              // chunks per thread per operand (2 / 4)
    constexpr int D = TC == 64 ? 4 : 2;               // stages of global loads in flight per thread
    constexpr int WT = TC / 2, FT = WT / 16;          // per-wave tile (2 x 2 waves), its 16x16 fragments
    __shared__ __attribute__((aligned(16))) char Ps[2][STG * ROWB];
    __shared__ __attribute__((aligned(16))) char Qs[2][STG * ROWB];
    __shared__ float dbs[TC];
    extern __shared__ double dsm[];   // tmp [2*cs] fp64 | bnp scale [cs] | shift [cs]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wc = wid >> 1, wk = wid & 1;
    const int N = a.n, cs = a.cs_in, ks = a.ks, pad = ks >> 1;
    const int K = ks * ks * cs;
    const int H = a.H, W = a.W;
    const T* __restrict__ X = (const T*)a.x;
    const T* __restrict__ DY = (const T*)a.dy;
    const bool do_bias = bias_out != nullptr;
    const bool pro = a.pro_bn_relu != 0;

    float* bnp = (float*)(dsm + 2 * cs);
    if (tid < TC) dbs[tid] = 0.f;
    const int sc_ = tid % CPR;
    const int pk = k0 + sc_ * CH;                // Q column
    const int ptap = pk / cs, pci = pk - ptap * cs;
    const int pdy = ptap / ks - pad, pdx = ptap % ks - pad;
    const int pco = co0 + sc_ * CH;              // P column
    const bool colp = pco < N, colq = pk < K;
    const float rW = 1.0f / (float)W, rH = 1.0f / (float)H;   // pixel decode (M / W < 2^22, host-checked)
    const int nst = mb < me ? (int)((me - mb + STG - 1) / STG) : 0;
    const int mfirst = nst > 0 ? (int)mb : 0;

    floatx4 acc[FT][FT];
#pragma unroll
    for (int i = 0; i < FT; ++i)
#pragma unroll
        for (int j = 0; j < FT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    // D-deep ring of register stages.  Loads are unconditional (clamped
    // addresses) so none of them sits under a branch (which would make the
    // compiler drain the queue); validity travels as bit masks applied when
    // the stage is written to LDS.
    u32x4 rp[D][PER], rq[D][PER];
    unsigned pm[D], qm[D];
    auto gload = [&](int u, long long mt) {
        unsigned bp = 0, bq = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = (tid + i * 256) / CPR;
            const long long m = mt + r;
            const bool inm = m < me;
            const int mi = inm ? (int)m : mfirst;
            const int row = fdiv_exact(mi, W, rW);
            const int xx = mi - row * W, yy = row - fdiv_exact(row, H, rH) * H;
            const int y2 = yy + pdy, x2 = xx + pdx;
            const bool okq = inm & colq & (y2 >= 0) & (y2 < H) & (x2 >= 0) & (x2 < W);
            rp[u][i] = *(const u32x4*)(DY + (long long)mi * a.cs_dy + (colp ? pco : 0));
            rq[u][i] = *(const u32x4*)(X + (okq ? ((long long)mi + pdy * W + pdx) * cs + pci : 0));
            bp |= (unsigned)(inm & colp) << i;
            bq |= (unsigned)okq << i;
        }
        pm[u] = bp;
        qm[u] = bq;
    };
    auto lstore = [&](int u, int buf) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = (tid + i * 256) / CPR;
            const uint32_t kp = ((pm[u] >> i) & 1u) ? ~0u : 0u;
            const uint32_t kq = ((qm[u] >> i) & 1u) ? ~0u : 0u;
            u32x4 v = rq[u][i];
            if (pro) {
                float f[CH];
                unpack(v, f, T());
#pragma unroll
                for (int j = 0; j < CH; ++j) f[j] = fmaxf(f[j] * bnp[pci + j] + bnp[cs + pci + j], 0.f);
                v = pack(f, T());
            }
            *(u32x4*)(Ps[buf] + r * ROWB + sc_ * 16) = rp[u][i] & u32x4{kp, kp, kp, kp};
            *(u32x4*)(Qs[buf] + r * ROWB + sc_ * 16) = v & u32x4{kq, kq, kq, kq};
        }
    };

    if (nst > 0) {   // the first D stages in flight while the BN table settles
#pragma unroll
        for (int u = 0; u < D; ++u) gload(u, mb + (long long)u * STG);
    }
    if (pro) block_bn_table(a.pro, a.cin, 0, cs, bnp, bnp + cs, nullptr, nullptr, dsm);
    __syncthreads();
    if (nst > 0) lstore(0, 0);
    __syncthreads();
    const int g = lane >> 4, li = lane & 15;
    float bpart = 0.f;   // bias partial: column tid % TC, rows (tid / TC) * STG*TC/256 .. of every stage
    for (int it0 = 0; it0 < nst; it0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int it = it0 + u;
            if (it >= nst) break;
            const int cur = it & 1;
            // ring slot u (stage it) is in LDS already: refill it with stage it + D
            gload(u, mb + (long long)(it + D) * STG);
            if (do_bias) {
                constexpr int RB = STG * TC / 256;
                const int c = tid % TC, r0 = (tid / TC) * RB;
#pragma unroll
                for (int r = 0; r < RB; ++r) bpart += ldv((const T*)(Ps[cur] + (r0 + r) * ROWB) + c);
            }
            if constexpr (sizeof(T) == 2) {
                const int q = li >> 2, p = li & 3;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    u32x4 af[FT], bfr[FT];
#pragma unroll
                    for (int i = 0; i < FT; ++i) {
                        const int c0 = wc * WT + i * 16 + 4 * p;
                        const char* base = Ps[cur] + (32 * s + 8 * g + q) * ROWB + c0 * 2;
                        i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((RNVP_LDS i16x4*)base);
                        i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((RNVP_LDS i16x4*)(base + 4 * ROWB));
                        af[i].x = (uint32_t)(uint16_t)lo.x | ((uint32_t)(uint16_t)lo.y << 16);
                        af[i].y = (uint32_t)(uint16_t)lo.z | ((uint32_t)(uint16_t)lo.w << 16);
                        af[i].z = (uint32_t)(uint16_t)hi.x | ((uint32_t)(uint16_t)hi.y << 16);
                        af[i].w = (uint32_t)(uint16_t)hi.z | ((uint32_t)(uint16_t)hi.w << 16);
                    }
#pragma unroll
                    for (int j = 0; j < FT; ++j) {
                        const int c0 = wk * WT + j * 16 + 4 * p;
                        const char* base = Qs[cur] + (32 * s + 8 * g + q) * ROWB + c0 * 2;
                        i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((RNVP_LDS i16x4*)base);
                        i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((RNVP_LDS i16x4*)(base + 4 * ROWB));
                        bfr[j].x = (uint32_t)(uint16_t)lo.x | ((uint32_t)(uint16_t)lo.y << 16);
                        bfr[j].y = (uint32_t)(uint16_t)lo.z | ((uint32_t)(uint16_t)lo.w << 16);
                        bfr[j].z = (uint32_t)(uint16_t)hi.x | ((uint32_t)(uint16_t)hi.y << 16);
                        bfr[j].w = (uint32_t)(uint16_t)hi.z | ((uint32_t)(uint16_t)hi.w << 16);
                    }
#pragma unroll
                    for (int i = 0; i < FT; ++i)
#pragma unroll
                        for (int j = 0; j < FT; ++j) Mf<bf16_t>::step(af[i], bfr[j], acc[i][j]);
                }
            } else {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    u32x4 af[FT], bfr[FT];
#pragma unroll
                    for (int i = 0; i < FT; ++i) {
                        const char* pcol = Ps[cur] + (16 * s + 4 * g) * ROWB + (wc * WT + i * 16 + li) * 4;
                        af[i].x = *(const uint32_t*)(pcol);
                        af[i].y = *(const uint32_t*)(pcol + ROWB);
                        af[i].z = *(const uint32_t*)(pcol + 2 * ROWB);
                        af[i].w = *(const uint32_t*)(pcol + 3 * ROWB);
                    }
#pragma unroll
                    for (int j = 0; j < FT; ++j) {
                        const char* qcol = Qs[cur] + (16 * s + 4 * g) * ROWB + (wk * WT + j * 16 + li) * 4;
                        bfr[j].x = *(const uint32_t*)(qcol);
                        bfr[j].y = *(const uint32_t*)(qcol + ROWB);
                        bfr[j].z = *(const uint32_t*)(qcol + 2 * ROWB);
                        bfr[j].w = *(const uint32_t*)(qcol + 3 * ROWB);
                    }
#pragma unroll
                    for (int i = 0; i < FT; ++i)
#pragma unroll
                        for (int j = 0; j < FT; ++j) Mf<float>::step(af[i], bfr[j], acc[i][j]);
                }
            }
            if (it + 1 < nst) lstore((u + 1) % D, cur ^ 1);
            __syncthreads();
        }
    }
    // D rows = co, cols = k
#pragma unroll
    for (int i = 0; i < FT; ++i)
#pragma unroll
        for (int j = 0; j < FT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + wc * WT + i * 16 + (lane >> 4) * 4 + r;
                const int k = k0 + wk * WT + j * 16 + (lane & 15);
                if (co < N && k < K) {
                    float* o = out + (long long)co * a.kp + k;
                    if (atomic) atomicAdd(o, acc[i][j][r]);
                    else *o = acc[i][j][r];
                }
            }
    if (do_bias) atomicAdd(&dbs[tid % TC], bpart);
    __syncthreads();
    if (do_bias && tid < TC && co0 + tid < N) {
        if (bias_atomic) atomicAdd(&bias_out[co0 + tid], dbs[tid]);
        else bias_out[co0 + tid] = dbs[tid];
    }
}

// grouped: block -> (conv, slab z, co tile, k tile).  Consecutive tasks (the
// tiles of one slab, which re-read the same pixels through L2) are placed on
// one XCD: dispatch hands block b to XCD b % 8, so task = bijective remap.
template <typename T, int TC>
__global__ __launch_bounds__(256) void k_wgrad_grouped(rnvp_wgrad_group g) {
    const int nb = gridDim.x, b = blockIdx.x;
    const int q = nb / 8, r = nb % 8, xcd = b % 8;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
    int c = 0;
    while (c + 1 < g.n_conv && g.conv[c + 1].task0 <= t) ++c;
    const rnvp_wgrad_conv& cv = g.conv[c];
    const int tco = (cv.n + TC - 1) / TC;
    const int local = t - cv.task0;
    const int per = tco * cv.tk;
    const int z = local / per, rr = local - z * per;
    const int cot = rr / cv.tk, kt = rr - cot * cv.tk;
    const long long M = (long long)g.B * g.H * g.W;
    const long long mb = (long long)z * cv.m_per_slab;
    const long long me = (mb + cv.m_per_slab < M) ? mb + cv.m_per_slab : M;
    const WgView v{cv.x, cv.dy, cv.pro, g.H, g.W, cv.ks, cv.cs_in, cv.cin, cv.cs_dy, cv.n, cv.kp, cv.pro_bn_relu};
    const int rep = z % cv.nrep;
    const bool atomic = cv.nrep < cv.nz;
    wgrad_tile<T, TC>(v, cot * TC, kt * TC, mb, me, M, cv.ws + (long long)rep * cv.n * cv.kp, atomic,
                  (cv.wsb && kt == 0) ? cv.wsb + (long long)rep * cv.n : nullptr, atomic);
}

// per-conv argument checks of a group (both the tap-shared and the generic path)
int wgrad_conv_status(const rnvp_wgrad_conv& v) {
    if (!v.x || !v.dy || !v.ws) return RNVP_E_INVALID;
    if (v.ks != 1 && v.ks != 3) return RNVP_E_UNSUPPORTED;
    if (v.n <= 0 || v.cin <= 0 || v.nz <= 0 || v.nrep <= 0 || v.nrep > v.nz) return RNVP_E_INVALID;
    if ((v.cs_in & 7) || (v.cs_dy & 7) || v.cs_in < v.cin || v.cs_dy < v.n) return RNVP_E_INVALID;
    if (v.kp < v.ks * v.ks * v.cs_in) return RNVP_E_INVALID;
    if (!al16(v.x) || !al16(v.dy)) return RNVP_E_INVALID;
    if (v.pro_bn_relu && v.pro.tab && (!v.pro.sums || !al16(v.pro.tab))) return RNVP_E_INVALID;
    return RNVP_OK;
}

}  // namespace

#ifndef RNVP_SLAB_PX
#define RNVP_SLAB_PX 2048
#endif
extern "C" int rnvp_wgrad_slabs(long long M) {
    // ~2048 pixels per slab (32 stages of 64), at most 128 slabs
    long long z = M / RNVP_SLAB_PX;
    if (z > 128) z = 128;
    if (z < 1) z = 1;
    return (int)z;
}

extern "C" int rnvp_wgrad_replicas(int nz) { return nz < 8 ? (nz < 1 ? 1 : nz) : 8; }

// host only: the tap-shared kernel class (0 .. 3) conv c of the group runs in,
// RNVP_E_UNSUPPORTED when the group takes the generic kernel
extern "C" int rnvp_wgrad_class(const rnvp_wgrad_group* gin, int c) {
    if (!gin || c < 0 || c >= gin->n_conv || gin->n_conv > RNVP_WGRAD_GROUP_MAX) return RNVP_E_INVALID;
    rnvp_wgrad_group gt = *gin;
    const int st = rnvp_wgrad_tap_prepare(&gt);
    return st != RNVP_OK ? st : gt.conv[c].cls;
}

extern "C" int rnvp_conv2d_wgrad_grouped(const rnvp_wgrad_group* gin, void* stream) {
    if (!gin || gin->n_conv <= 0 || gin->n_conv > RNVP_WGRAD_GROUP_MAX) return RNVP_E_INVALID;
    if (gin->dtype != RNVP_F32 && gin->dtype != RNVP_BF16) return RNVP_E_INVALID;
    if (gin->B < 0 || gin->H <= 0 || gin->W <= 0) return RNVP_E_INVALID;
    if (gin->B == 0) return RNVP_OK;
    // bf16: the tap-shared kernel (wgrad_tap.hip) where it applies
    if (gin->dtype == RNVP_BF16) {
        for (int c = 0; c < gin->n_conv; ++c) {
            const int st = wgrad_conv_status(gin->conv[c]);
            if (st != RNVP_OK) return st;
        }
        rnvp_wgrad_group gt = *gin;
        const int rc = rnvp_wgrad_tap_launch(&gt, (hipStream_t)stream);
        if (rc != RNVP_E_UNSUPPORTED) return rc;
    }
    rnvp_wgrad_group g = *gin;
    const long long M = (long long)g.B * g.H * g.W;
    const int STG = g.dtype == RNVP_BF16 ? 64 : 32;
    if (M >= (1ll << 31) || M / g.W >= (1ll << 22)) return RNVP_E_UNSUPPORTED;
    // 64 x 64 output tiles (128 x 128 halves the operand re-reads but was
    // measured slower at every scale of config 1: 5.0 vs 4.3 ms per step)
    constexpr int TC = 64;
    long long tasks = 0;
    int max_cs = 8;
    for (int c = 0; c < g.n_conv; ++c) {
        rnvp_wgrad_conv& v = g.conv[c];
        const int st = wgrad_conv_status(v);
        if (st != RNVP_OK) return st;
        const long long steps = (M + STG - 1) / STG;
        v.m_per_slab = ((steps + v.nz - 1) / v.nz) * STG;
        if ((M + v.m_per_slab - 1) / v.m_per_slab > v.nz) return RNVP_E_INVALID;
        v.tk = (v.ks * v.ks * v.cs_in + TC - 1) / TC;
        v.task0 = (int)tasks;
        tasks += (long long)v.nz * ((v.n + TC - 1) / TC) * v.tk;
        if (v.cs_in > max_cs) max_cs = v.cs_in;
    }
    if (tasks <= 0 || tasks > (1ll << 30)) return RNVP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t shm = 24 * (size_t)max_cs;
    if (g.dtype == RNVP_F32) k_wgrad_grouped<float, TC><<<(unsigned)tasks, 256, shm, s>>>(g);
    else k_wgrad_grouped<bf16_t, TC><<<(unsigned)tasks, 256, shm, s>>>(g);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_wgrad_multi_struct_size(int which) {
    if (which == 0) return (int)sizeof(rnvp_wgrad_multi_conv);
    if (which == 1) return (int)sizeof(rnvp_wgrad_multi);
    return -1;
}

// host only: the plan of the model-wide tap-shared launch of class cls
extern "C" int rnvp_wgrad_multi_plan(const rnvp_wgrad_group* groups, int n_groups, int cls,
                                     rnvp_wgrad_multi_conv* convs, int conv_cap, int* xcd_start, int* tasks,
                                     int task_cap, rnvp_wgrad_multi* m) {
    if (!groups || n_groups <= 0 || !m || cls < 0 || cls > 3 || conv_cap < 0 || task_cap < 0) return RNVP_E_INVALID;
    for (int g = 0; g < n_groups; ++g) {
        const rnvp_wgrad_group& gr = groups[g];
        if (gr.n_conv <= 0 || gr.n_conv > RNVP_WGRAD_GROUP_MAX) return RNVP_E_INVALID;
        if (gr.dtype != RNVP_F32 && gr.dtype != RNVP_BF16) return RNVP_E_INVALID;
        if (gr.B <= 0 || gr.H <= 0 || gr.W <= 0) return RNVP_E_INVALID;
        for (int c = 0; c < gr.n_conv; ++c) {
            const int st = wgrad_conv_status(gr.conv[c]);
            if (st != RNVP_OK) return st;
        }
    }
    return rnvp_wgrad_tap_multi_plan(groups, n_groups, cls, convs, conv_cap, xcd_start, tasks, task_cap, m);
}

extern "C" int rnvp_conv2d_wgrad_multi(const rnvp_wgrad_multi* m, void* stream) {
    if (!m) return RNVP_E_INVALID;
    return rnvp_wgrad_tap_multi_launch(m, (hipStream_t)stream);
}
