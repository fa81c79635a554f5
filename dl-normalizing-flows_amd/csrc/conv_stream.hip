// Register-streaming conv for small channel counts (scales 1-2): one of the
// families of rnvp_conv2d's dispatch (conv.hip); same fused operation as the
// LDS-tiled kernel (conv_tiled.hip).
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"

namespace {

// ---------------------------------------------------------------------------
// register-streaming conv for small channel counts (scales 1-2)
// ---------------------------------------------------------------------------
// For K <= ~600 and N <= 64 the whole packed weight matrix fits in LDS, and an
// MFMA B-fragment column (lane&15) x k-group (lane>>4) is exactly one pixel's
// 16-byte channel chunk: waves stream pixel fragments from global/L2 straight
// into registers (BN+ReLU applied there), no LDS round trip and no barrier in
// the main loop.  The product is formed transposed, D[n][m] = W[n][k] X[m][k]^T,
// so a lane ends up owning 4 consecutive output channels of one pixel: the
// epilogue reads/writes 8-byte (bf16) / 16-byte (f32) vectors.  Each wave owns
// 64-pixel tiles (4 MFMA column tiles); the next k-step's (or the next tile's)
// fragments are loaded before the current MFMAs, and the first tile's loads
// are issued before the BN-table / weight prologue.

template <typename T, int NT, int TW>
__global__ __launch_bounds__(256) void k_conv_stream(rnvp_conv_args a, int shards) {
    constexpr int CH = Mf<T>::CH;
    constexpr int KS = 4 * CH;             // K per step call (bf16: one 16x16x32, f32: four 16x16x4)
    constexpr int NC = 16 * NT;            // columns held by a wave
    extern __shared__ double dsm[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const long long M = (long long)a.B * a.H * a.W;
    const int N = a.n, cs = a.cs_in, ks = a.ks, pad = ks >> 1;
    const int K = ks * ks * cs;
    const int nsteps = (K + KS - 1) / KS;
    const int kpl = lds_mfma_pitch(nsteps * KS, CH);   // LDS row pitch (conflict-free row reads)
    const bool pro = a.pro_bn_relu != 0;
    const bool epi_bn = a.epi_relu_bn_bwd != 0;
    const int ntmp = cs > NC ? cs : NC;

    double* tmp = dsm;
    float* bnp = (float*)(dsm + 2 * ntmp);
    float* etab = bnp + 2 * cs;            // scale | shift | mean | rstd [NC each]
    float* btab = etab + 4 * NC;           // bias [NC]
    double* red = (double*)(btab + NC);    // [4 waves][NC][2]
    T* Wl = (T*)(red + 4 * NC * 2);

    // pixel decode of this wave's tile (4 column tiles of 16 pixels); M < 2^31
    const int ntiles = (int)((M + 16 * TW - 1) / (16 * TW));
    const int tstride = gridDim.x * 4;
    int mrow[TW], yr[TW], xr[TW];
    auto decode = [&](int t) {
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            const int m = t * (16 * TW) + i * 16 + li;
            mrow[i] = (t < ntiles && m < M) ? m : -1;
            const int mm = mrow[i] >= 0 ? m : 0;
            xr[i] = mm % a.W;
            yr[i] = (mm / a.W) % a.H;
        }
    };
    const T* __restrict__ X = (const T*)a.x;
    u32x4 ra[TW];
    unsigned msk = 0;
    int cur_ci = 0;
    auto load = [&](int s) {
        const int k = s * KS + g * CH;
        const int tap = k / cs, ci = k - tap * cs;
        const int dy = tap / ks - pad, dx = tap % ks - pad;
        cur_ci = ci;
        msk = 0;
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            ra[i] = u32x4{0u, 0u, 0u, 0u};
            const int yy = yr[i] + dy, xx = xr[i] + dx;
            if (mrow[i] >= 0 && k < K && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                ra[i] = *(const u32x4*)(X + (long long)(mrow[i] + dy * a.W + dx) * cs + ci);
                msk |= 1u << i;
            }
        }
    };
    // first tile's fragments in flight while the prologue runs
    int t = blockIdx.x * 4 + wid;
    decode(t);
    load(0);

    if (pro) block_bn_table(a.pro, a.cin, 0, cs, bnp, bnp + cs, nullptr, nullptr, tmp);
    if (epi_bn) block_bn_table(a.epi, N, 0, NC, etab, etab + NC, etab + 2 * NC, etab + 3 * NC, tmp);
    // weights -> LDS (rows >= N and k >= K zero), bias -> LDS
    {
        const T* Wg = (const T*)a.w;
        const int cpr = kpl / CH;
        for (int q = tid; q < NC * cpr; q += 256) {
            const int r = q / cpr, c = q - r * cpr;
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (r < N && c * CH < nsteps * KS) v = *(const u32x4*)(Wg + (long long)r * a.kp + c * CH);
            *(u32x4*)(Wl + r * kpl + c * CH) = v;
        }
        for (int n = tid; n < NC; n += 256) btab[n] = (a.bias && n < N) ? a.bias[n] : 0.f;
    }
    __syncthreads();

    const int cso = a.cs_out;
    double s1[NT][4], s2[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) s1[j][r] = s2[j][r] = 0.f;

    for (; t < ntiles; t += tstride) {
        floatx4 acc[TW][NT];
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

        for (int s = 0; s < nsteps; ++s) {
            u32x4 av[TW];
            const int ci = cur_ci;
            const unsigned mk = msk;
#pragma unroll
            for (int i = 0; i < TW; ++i) av[i] = ra[i];
            if (s + 1 < nsteps) load(s + 1);   // next k-step in flight under these MFMAs
            if (pro) {
#pragma unroll
                for (int i = 0; i < TW; ++i) {
                    if (mk & (1u << i)) {
                        float f[CH];
                        unpack(av[i], f, T());
#pragma unroll
                        for (int j = 0; j < CH; ++j) f[j] = fmaxf(f[j] * bnp[ci + j] + bnp[cs + ci + j], 0.f);
                        av[i] = pack(f, T());
                    }
                }
            }
            u32x4 wv[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) wv[j] = *(const u32x4*)(Wl + (j * 16 + li) * kpl + s * KS + g * CH);
#pragma unroll
            for (int i = 0; i < TW; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) Mf<T>::step(wv[j], av[i], acc[i][j]);
        }
        // epilogue: lane owns channels j*16 + 4g .. +3 of pixel t*64 + i*16 + li
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            const long long m = mrow[i];
            if (m < 0) continue;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n0 = j * 16 + 4 * g;
                if (n0 >= cso) continue;
                epi4<T>(a, m * cso + n0, acc[i][j], btab + n0, epi_bn, etab + n0, NC, s1[j], s2[j], N - n0);
            }
        }
        if (t + tstride < ntiles) {
            decode(t + tstride);
            load(0);
        }
    }
    const bool want_sums = a.out_sums || (epi_bn && a.epi_sums);
    if (want_sums) {
        row_stats16(s1, s2, li, [&](int j, int r, int which, double u) {
            red[(wid * NC + j * 16 + 4 * g + r) * 2 + which] = u;
        });
        __syncthreads();
        double* sums = shard_ptr(epi_bn ? a.epi_sums : a.out_sums, shards, N);
        for (int n = tid; n < N; n += 256) {
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                t1 += red[(w * NC + n) * 2];
                t2 += red[(w * NC + n) * 2 + 1];
            }
            atomicAdd(&sums[n], (double)t1);
            atomicAdd(&sums[N + n], (double)t2);
        }
    }
}

template <typename T>
size_t stream_lds_bytes(const rnvp_conv_args* a, int nt) {
    constexpr int CH = Mf<T>::CH, KS = 4 * CH;
    const int K = a->ks * a->ks * a->cs_in;
    const int kpl = lds_mfma_pitch(((K + KS - 1) / KS) * KS, CH);
    const int nc = 16 * nt, ntmp = a->cs_in > nc ? a->cs_in : nc;
    return 16 * (size_t)ntmp + 8 * (size_t)a->cs_in + 16 * (size_t)nc + 4 * (size_t)nc + 64 * (size_t)nc +
           (size_t)nc * kpl * sizeof(T);
}

template <typename T, int NT, int TW>
int launch_stream(const rnvp_conv_args* a, hipStream_t s) {
    const long long M = (long long)a->B * a->H * a->W;
    const long long ntiles = (M + 16 * TW - 1) / (16 * TW);
    long long grid = (ntiles + 3) / 4;
    // two workgroups per CU, each walking several tiles: the next tile's
    // fragments load under the current tile's epilogue (measured: 10-20 %
    // faster than one tile per wave at scale 1, equal at scale 2)
    if (grid > 512) grid = 512;
    k_conv_stream<T, NT, TW><<<(unsigned)grid, 256, stream_lds_bytes<T>(a, NT), s>>>(*a, rnvp_stat_shards(M));
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// pixels per wave (16 * TW), picked per pixel count from measurements
template <typename T, int NT>
int launch_stream_tw(const rnvp_conv_args* a, hipStream_t s) {
    const long long M = (long long)a->B * a->H * a->W;
    const int tw = M >= 4 * 64 * 1024 ? 4 : (M >= 32 * 1024 ? 2 : 1);   // measured: s1 4, s2 2
    if (tw == 1) return launch_stream<T, NT, 1>(a, s);
    if (tw == 2) return launch_stream<T, NT, 2>(a, s);
    return launch_stream<T, NT, 4>(a, s);
}

// true when the streaming kernel handles this conv (N <= 64, weights fit LDS)
template <typename T>
bool stream_ok(const rnvp_conv_args* a) {
    if (a->n > 64 || a->cs_in > 64) return false;
    const int nt = a->n <= 16 ? 1 : (a->n <= 32 ? 2 : 4);
    return stream_lds_bytes<T>(a, nt) <= 48 * 1024;
}

template <typename T>
int dispatch_stream(const rnvp_conv_args* a, hipStream_t s) {
    if (a->n <= 16) return launch_stream_tw<T, 1>(a, s);
    if (a->n <= 32) return launch_stream_tw<T, 2>(a, s);
    return launch_stream_tw<T, 4>(a, s);
}

}  // namespace

// n <= 64, cs_in <= 64 and the packed weights fit 48 KiB of LDS
// (RNVP_E_UNSUPPORTED otherwise)
int rnvp_conv_stream_launch(const rnvp_conv_args* a, hipStream_t s) {
    if (a->dtype == RNVP_F32) return stream_ok<float>(a) ? dispatch_stream<float>(a, s) : RNVP_E_UNSUPPORTED;
    return stream_ok<bf16_t>(a) ? dispatch_stream<bf16_t>(a, s) : RNVP_E_UNSUPPORTED;
}
