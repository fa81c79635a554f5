// LDS-tiled s/t ResNet convolution on the MFMA matrix cores (gfx950): the
// family of rnvp_conv2d's dispatch (conv.hip) that takes every shape.
//
// Implicit GEMM over NHWC activations: M = B*H*W pixels, N = output channels,
// K = ks*ks*cs_in (tap-major, channel-minor).  BatchNorm+ReLU of the operand is
// applied while staging the A tile (global -> registers -> LDS); bias /
// residual / skip accumulation and the next BatchNorm's batch statistics are
// fused into the epilogue.  The data gradient is the same kernel on the
// flipped/transposed weight image with a ReLU+BN-backward epilogue.
//
// Pipeline: a stage is 128 B of K per tile row (64 bf16 / 32 f32), double
// buffered in LDS; the global loads of stage k+1 are issued before the MFMAs
// of stage k and land in registers, the BN/ReLU transform and the LDS store
// happen after the MFMAs -> one barrier per stage, load latency under compute.
// Small grids (deep scales: M = 1024..4096 pixels, K up to 4608) split K over
// workgroups into an fp32 workspace reduced by a second, epilogue kernel.
// BN statistics go to rnvp_stat_shards(M) shards (bounded atomic contention).
//
// MFMA: bf16 -> v_mfma_f32_16x16x32_bf16 (fp32 accumulate);
//       f32  -> v_mfma_f32_16x16x4_f32 (exact fp32, parity mode).
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"

namespace {

// ---------------------------------------------------------------------------
// forward / data-gradient conv
// ---------------------------------------------------------------------------
template <typename T, int BM, int BN, int WM, int WN, bool PARTIAL>
__global__ __launch_bounds__(256) void k_conv(rnvp_conv_args a, int kt_per_split, int shards) {
    constexpr int CH = Mf<T>::CH;
    constexpr int BKS = 8 * CH;                        // K elements per stage
    constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
    constexpr int A_PER = (BM * 8) / 256;
    constexpr int B_CH = BN * 8;
    constexpr int B_PER = (B_CH + 255) / 256;
    static_assert(WM * WN == 4, "4 waves");
    static_assert(A_PER >= 1, "BM >= 32");

    __shared__ u32x4 As[2][BM * 8];
    __shared__ u32x4 Bs[2][BN * 8];
    __shared__ double red[WM * BN * 2];
    extern __shared__ double dsm[];   // tmp [2*max(cs,BN)] fp64 | bnp [2*cs] | etab [4*BN]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const long long M = (long long)a.B * a.H * a.W;
    const int N = a.n, cs = a.cs_in, ks = a.ks, pad = a.ks >> 1;
    const int K = ks * ks * cs;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const T* __restrict__ X = (const T*)a.x;
    const T* __restrict__ Wt = (const T*)a.w;
    const bool pro = a.pro_bn_relu != 0;
    const bool epi_bn = a.epi_relu_bn_bwd != 0;

    double* tmp = dsm;
    float* bnp = (float*)(dsm + 2 * max(cs, BN));   // prologue scale [cs] | shift [cs]
    float* etab = bnp + 2 * cs;                      // epilogue scale | shift | mean | rstd [BN each]
    float* btab = etab + 4 * BN;                     // bias [BN]

    // per-thread A rows (fixed over K) and chunk column
    const int cA = tid & 7;
    long long arow_m[A_PER];
    int arow_y[A_PER], arow_x[A_PER];
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
        const int r = (tid + i * 256) >> 3;
        const long long m = m0 + r;
        arow_m[i] = m < M ? m : -1;
        const long long mm = m < M ? m : 0;
        arow_x[i] = (int)(mm % a.W);
        arow_y[i] = (int)((mm / a.W) % a.H);
    }

    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int nk = (K + BKS - 1) / BKS;
    const int kt0 = blockIdx.z * kt_per_split;
    const int kt1 = min(nk, kt0 + kt_per_split);

    u32x4 ra[A_PER], rb[B_PER];
    unsigned amask = 0;
    int aci = 0;

    auto gload = [&](int kt) {
        const int k = kt * BKS + cA * CH;
        const int tap = k / cs, ci = k - tap * cs;
        const int dy = tap / ks - pad, dx = tap % ks - pad;
        aci = ci;
        amask = 0;
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int yy = arow_y[i] + dy, xx = arow_x[i] + dx;
            ra[i] = u32x4{0u, 0u, 0u, 0u};
            if (arow_m[i] >= 0 && k < K && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                ra[i] = *(const u32x4*)(X + (arow_m[i] + (long long)dy * a.W + dx) * cs + ci);
                amask |= 1u << i;
            }
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int q = tid + i * 256;
            rb[i] = u32x4{0u, 0u, 0u, 0u};
            if (q < B_CH) {
                const int nr = q >> 3, cc = q & 7;
                if (n0 + nr < N) rb[i] = *(const u32x4*)(Wt + (long long)(n0 + nr) * a.kp + kt * BKS + cc * CH);
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int r = (tid + i * 256) >> 3;
            u32x4 v = ra[i];
            if (pro) {
                if (amask & (1u << i)) {
                    float f[CH];
                    unpack(v, f, T());
#pragma unroll
                    for (int j = 0; j < CH; ++j) f[j] = fmaxf(f[j] * bnp[aci + j] + bnp[cs + aci + j], 0.f);
                    v = pack(f, T());
                } else {
                    v = u32x4{0u, 0u, 0u, 0u};
                }
            }
            As[buf][sw8(r, cA)] = v;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int q = tid + i * 256;
            if (q < B_CH) Bs[buf][sw8(q >> 3, q & 7)] = rb[i];
        }
    };

    // the first stage's loads are in flight while the BN tables are built
    if (kt0 < kt1) gload(kt0);
    if (pro) block_bn_table(a.pro, a.cin, 0, cs, bnp, bnp + cs, nullptr, nullptr, tmp);
    if (epi_bn && !PARTIAL)
        block_bn_table(a.epi, N, n0, BN, etab, etab + BN, etab + 2 * BN, etab + 3 * BN, tmp);
    for (int c = tid; c < BN; c += 256) btab[c] = (a.bias && n0 + c < N) ? a.bias[n0 + c] : 0.f;
    __syncthreads();   // bnp / etab / btab ready
    if (kt0 < kt1) lstore(0);
    __syncthreads();
    const int g = lane >> 4, li = lane & 15;
    for (int kt = kt0; kt < kt1; ++kt) {
        const int cur = (kt - kt0) & 1;
        const bool more = kt + 1 < kt1;
        if (more) gload(kt + 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = As[cur][sw8(wm * WTM + i * 16 + li, s * 4 + g)];
#pragma unroll
            for (int j = 0; j < TN; ++j) bfr[j] = Bs[cur][sw8(wn * WTN + j * 16 + li, s * 4 + g)];
            // transposed product: acc[i][j] = D[n][m], a lane owns 4 channels of one pixel
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) Mf<T>::step(bfr[j], af[i], acc[i][j]);
        }
        if (more) lstore(cur ^ 1);
        __syncthreads();
    }

    const int cso = a.cs_out;
    if constexpr (PARTIAL) {
        float* ws = a.ws + (long long)blockIdx.z * M * cso;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const long long m = m0 + wm * WTM + i * 16 + li;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 16 + 4 * g;
                if (n < cso) *(floatx4*)(ws + m * cso + n) = acc[i][j];
            }
        }
        return;
    } else {
        // ---- fused epilogue (4 channels of one pixel per lane) ----
        const bool want_sums = a.out_sums || (a.epi_relu_bn_bwd && a.epi_sums);
        double s1[TN][4], s2[TN][4];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) s1[j][r] = s2[j][r] = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const long long m = m0 + wm * WTM + i * 16 + li;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = wn * WTN + j * 16 + 4 * g;
                const int n = n0 + col;
                if (n >= cso) continue;
                epi4<T>(a, m * cso + n, acc[i][j], btab + col, epi_bn, etab + col, BN, s1[j], s2[j], N - n);
            }
        }
        if (want_sums) {
            double* sums = shard_ptr(a.epi_relu_bn_bwd ? a.epi_sums : a.out_sums, shards, N);
            row_stats16(s1, s2, li, [&](int j, int r, int which, double u) {
                const int col = wn * WTN + j * 16 + 4 * g + r;
                red[(wm * BN + col) * 2 + which] = u;
            });
            __syncthreads();
            for (int col = tid; col < BN; col += 256) {
                const int n = n0 + col;
                if (n >= N) continue;
                double t1 = 0.0, t2 = 0.0;
#pragma unroll
                for (int w = 0; w < WM; ++w) {
                    t1 += red[(w * BN + col) * 2];
                    t2 += red[(w * BN + col) * 2 + 1];
                }
                atomicAdd(&sums[n], (double)t1);
                atomicAdd(&sums[N + n], (double)t2);
            }
        }
    }
}

// split-K reduction + epilogue: block = [16 pixels][64 channels], thread =
// 4 channels of one pixel; partials ws[z][m][cs_out] (fp32).
constexpr int MAX_SPLITS = 8;

template <typename T>
__global__ __launch_bounds__(256) void k_splitk_epi(rnvp_conv_args a, int splits, int shards) {
    __shared__ double red[16][64][2];
    __shared__ double tmp[128];
    __shared__ float etab[4 * 64];
    __shared__ float btab[64];
    const int tid = threadIdx.x, c4 = tid & 15, row = tid >> 4;
    const long long M = (long long)a.B * a.H * a.W;
    const int N = a.n, cso = a.cs_out;
    const int n0 = blockIdx.y * 64;
    const long long m = (long long)blockIdx.x * 16 + row;
    const int col = 4 * c4, n = n0 + col;
    const bool epi_bn = a.epi_relu_bn_bwd != 0;
    // partial loads first (independent of the tables)
    floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
    const bool live = m < M && n < cso;
    if (live) {
        const float* wz = a.ws + m * cso + n;
#pragma unroll
        for (int z = 0; z < MAX_SPLITS; ++z)
            if (z < splits) acc += *(const floatx4*)(wz + (long long)z * M * cso);
    }
    if (epi_bn) block_bn_table(a.epi, N, n0, 64, etab, etab + 64, etab + 128, etab + 192, tmp);
    if (tid < 64) btab[tid] = (a.bias && n0 + tid < N) ? a.bias[n0 + tid] : 0.f;
    __syncthreads();
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) epi4<T>(a, m * cso + n, acc, btab + col, epi_bn, etab + col, 64, s1, s2, N - n);
    const bool want_sums = a.out_sums || (epi_bn && a.epi_sums);
    if (want_sums) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[row][col + r][0] = s1[r];
            red[row][col + r][1] = s2[r];
        }
        __syncthreads();
        if (tid < 64 && n0 + tid < N) {
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                t1 += red[r][tid][0];
                t2 += red[r][tid][1];
            }
            double* sums = shard_ptr(epi_bn ? a.epi_sums : a.out_sums, shards, N);
            atomicAdd(&sums[n0 + tid], (double)t1);
            atomicAdd(&sums[N + n0 + tid], (double)t2);
        }
    }
}

// SPLITK false: the caller's grid is >= 512 workgroups and K is split only
// below 384, so that tile has no split-K instantiation
template <typename T, int BM, int BN, int WM, int WN, bool SPLITK = true>
int launch_conv(const rnvp_conv_args* a, hipStream_t s) {
    constexpr int BKS = 8 * Mf<T>::CH;
    const long long M = (long long)a->B * a->H * a->W;
    const int K = a->ks * a->ks * a->cs_in;
    const int nk = (K + BKS - 1) / BKS;
    const long long gm = (M + BM - 1) / BM, gn = (a->n + BN - 1) / BN;
    const long long grid = gm * gn;
    const int shards = rnvp_stat_shards(M);
    const int cs = a->cs_in;
    const size_t shm = 16 * (size_t)(cs > BN ? cs : BN) + 8 * (size_t)cs + 20 * (size_t)BN;
    if constexpr (SPLITK) {
        int splits = 1;
        if (a->ws && grid < 384 && nk >= 8) {
            splits = (int)((512 + grid - 1) / grid);
            if (splits > MAX_SPLITS) splits = MAX_SPLITS;
            if (splits > nk / 4) splits = nk / 4;
            while (splits > 1 && (long long)splits * M * a->cs_out > a->ws_elems) --splits;
        }
        if (splits > 1) {
            const int kps = (nk + splits - 1) / splits;
            splits = (nk + kps - 1) / kps;
            dim3 g1((unsigned)gm, (unsigned)gn, (unsigned)splits);
            k_conv<T, BM, BN, WM, WN, true><<<g1, 256, shm, s>>>(*a, kps, shards);
            RNVP_LAUNCH_CHECK();
            dim3 g2((unsigned)((M + 15) / 16), (unsigned)((a->cs_out + 63) / 64));
            k_splitk_epi<T><<<g2, 256, 0, s>>>(*a, splits, shards);
            RNVP_LAUNCH_CHECK();
            return RNVP_OK;
        }
    }
    dim3 g1((unsigned)gm, (unsigned)gn, 1);
    k_conv<T, BM, BN, WM, WN, false><<<g1, 256, shm, s>>>(*a, nk, shards);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

template <typename T>
int dispatch_tiled(const rnvp_conv_args* a, hipStream_t s) {
    const long long M = (long long)a->B * a->H * a->W;
    // largest tile that still gives >= 512 workgroups (2 per CU); small grids
    // fall through to 64x64 tiles and split K
    if (a->n <= 16) return launch_conv<T, 128, 16, 4, 1>(a, s);
    if (a->n <= 32) return M >= 512 * 128 ? launch_conv<T, 128, 32, 4, 1, false>(a, s) : launch_conv<T, 64, 32, 4, 1>(a, s);
    if (a->n <= 64) return M >= 512 * 128 ? launch_conv<T, 128, 64, 2, 2, false>(a, s) : launch_conv<T, 64, 64, 2, 2>(a, s);
    const long long g128 = ((M + 127) / 128) * ((a->n + 127) / 128);
    if (g128 >= 512) return launch_conv<T, 128, 128, 2, 2, false>(a, s);
    return launch_conv<T, 64, 64, 2, 2>(a, s);
}

}  // namespace

// every conv that passes rnvp_conv2d's argument checks
int rnvp_conv_tiled_launch(const rnvp_conv_args* a, hipStream_t s) {
    return a->dtype == RNVP_F32 ? dispatch_tiled<float>(a, s) : dispatch_tiled<bf16_t>(a, s);
}
