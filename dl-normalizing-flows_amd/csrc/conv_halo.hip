// Halo-tile conv for the deep scales: one of the families of rnvp_conv2d's
// dispatch (conv.hip), tried where the deep family (conv_deep.hip) declines;
// same fused operation as the LDS-tiled kernel (conv_tiled.hip).
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"

namespace {

// prologue BN table capacity of the halo-tile kernel (channels)
constexpr int DK_MAX_CS = 1024;

// ---------------------------------------------------------------------------
// halo-tile conv (deep scales): act(x) staged ONCE per workgroup in LDS
// ---------------------------------------------------------------------------
// A workgroup owns 64 consecutive output pixels (NHW order: a band of image
// rows, or several whole 4x4 / 8x8 images) x BN channels.  Its input rows
// [m0 - hal, m0 + 64 + hal) (hal = one image row + 1 for 3x3) are loaded
// once, BN+ReLU'd once and kept in LDS; every tap of the 3x3 then reads its
// A fragments from LDS (tap validity from a per-pixel 9-bit mask, invalid
// taps read a zero row), so the transform and the activation traffic are not
// repeated per tap and per channel tile.  Only the weights stream from global
// memory (register ring, DK k-steps ahead; every load unconditional).  The
// four waves split K (interleaved k-steps) and their partial tiles are summed
// through LDS for the fused epilogue.

template <typename T, int BN>
size_t halo_lds_bytes(int cs, int W, int ks) {
    constexpr int BM = 64, TM = BM / 16;
    const int pad = ks / 2, hal = pad * (W + 1), R = BM + 2 * hal;
    const size_t head = 4 * (4 * BN + BN) + 8 * (2 * TM * BN);
    const size_t zrow = (size_t)halo_pitch<T>(cs) * sizeof(T);
    size_t act = (size_t)R * halo_pitch<T>(cs) * sizeof(T);
    const size_t red = 4 * (size_t)BM * (BN + 4) * 4;
    if (red > act) act = red;
    const size_t tail = 8 * 2 * (size_t)(cs > BN ? cs : BN) + 4 * 2 * (size_t)cs;
    return head + zrow + act + tail;
}

template <typename T, int BN, int KSZ, bool PRO, int DK, bool UNI>
__global__ __launch_bounds__(256) void k_conv_halo(rnvp_conv_args a, int shards) {
    constexpr int BM = 64;
    constexpr int CH = Mf<T>::CH, KS = 4 * CH;
    constexpr int TM = BM / 16, TN = BN / 16;
    constexpr int PAD = KSZ / 2;
    constexpr int RP = BN + 4;
    constexpr int FR = TM * TN / 4;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int M = a.B * a.H * a.W, W = a.W, H = a.H;
    const int N = a.n, cs = a.cs_in;
    const int K = KSZ * KSZ * cs;
    const int nsteps = (K + KS - 1) / KS;
    const int gm = (M + BM - 1) / BM;
    const int nb = gridDim.x, b = blockIdx.x;
    const int q8 = nb / 8, r8 = nb % 8, xcd = b % 8;
    const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + b / 8;
    const int nt = t / gm, mt = t - nt * gm;
    const int m0 = mt * BM, n0 = nt * BN;
    const T* __restrict__ X = (const T*)a.x;
    const T* __restrict__ Wt = (const T*)a.w;
    const bool epi_bn = a.epi_relu_bn_bwd != 0;

    const int hal = PAD * (W + 1);
    const int R = BM + 2 * hal;
    const int pitch = halo_pitch<T>(cs);
    float* etab = (float*)lds;                 // scale | shift | mean | rstd [BN each]
    float* btab = etab + 4 * BN;
    double* sred = (double*)(btab + BN);       // [TM][BN][2]
    T* zrow = (T*)(sred + TM * BN * 2);
    T* act = zrow + pitch;
    size_t act_bytes = (size_t)R * pitch * sizeof(T);
    if (act_bytes < 4 * (size_t)BM * RP * 4) act_bytes = 4 * (size_t)BM * RP * 4;
    double* tmp = (double*)((char*)act + act_bytes);
    float* bnp = (float*)(tmp + 2 * (cs > BN ? cs : BN));
    float* red = (float*)act;                  // [4][BM][RP], after the K loop

    // ---- prologue, ordered for the in-order vmcnt: staging loads, then the
    // BN-table loads (the table code waits for both), then the weight ring
    // (stays in flight across the transform and the barrier) ----
    const int cpr = cs / CH;
    const int total = R * cpr;
    const float rcpr = 1.0f / (float)cpr;
    constexpr int SB = 20;                     // chunks per thread per batch (deep scales: one batch)
    u32x4 sv[SB];
    auto stage_load = [&](int q0) {
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int q = q0 + u * 256 + tid;
            const int r = fdiv_small(q, rcpr), c = q - r * cpr;
            const int p = m0 - hal + r;
            const bool ok = (q < total) & (p >= 0) & (p < M);
            sv[u] = *(const u32x4*)(X + (ok ? (long long)p * cs + c * CH : 0));
        }
    };
    auto stage_store = [&](int q0) {
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int q = q0 + u * 256 + tid;
            if (q >= total) continue;
            const int r = fdiv_small(q, rcpr), c = q - r * cpr;
            const int p = m0 - hal + r;
            u32x4 w = sv[u];
            if (PRO) {
                float f[CH];
                unpack(w, f, T());
                const int c0 = c * CH;
#pragma unroll
                for (int e = 0; e < CH; e += 4) {
                    const floatx4 sc = *(const floatx4*)&bnp[c0 + e];
                    const floatx4 sh = *(const floatx4*)&bnp[cs + c0 + e];
                    f[e] = fmaxf(f[e] * sc.x + sh.x, 0.f);
                    f[e + 1] = fmaxf(f[e + 1] * sc.y + sh.y, 0.f);
                    f[e + 2] = fmaxf(f[e + 2] * sc.z + sh.z, 0.f);
                    f[e + 3] = fmaxf(f[e + 3] * sc.w + sh.w, 0.f);
                }
                w = pack(f, T());
            }
            const uint32_t keep = (p >= 0 && p < M) ? ~0u : 0u;
            *(u32x4*)(act + r * pitch + c * CH) = w & u32x4{keep, keep, keep, keep};
        }
    };
    BnTab<DK_MAX_CS / 256> ptab;
    BnTab<1> etb;
    if (PRO) tab_issue(a.pro, a.cin, 0, cs, ptab);
    if (epi_bn) tab_issue(a.epi, N, n0, BN, etb);
    stage_load(0);
    if (PRO) tab_finish(a.pro, a.cin, 0, cs, ptab, bnp, bnp + cs, nullptr, nullptr);
    if (epi_bn) tab_finish(a.epi, N, n0, BN, etb, etab, etab + BN, etab + 2 * BN, etab + 3 * BN);
    for (int c = tid; c < BN; c += 256) btab[c] = (a.bias && n0 + c < N) ? a.bias[n0 + c] : 0.f;
    for (int c = tid * CH; c < pitch; c += 256 * CH) *(u32x4*)(zrow + c) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    const T* wrow[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        // rows >= N (clamped to row 0) only feed output columns that are never stored
        const int row = n0 + j * 16 + li;
        wrow[j] = Wt + (long long)(row < N ? row : 0) * a.kp + g * CH;
    }
    const int wv = __builtin_amdgcn_readfirstlane(wid);     // wave-uniform: step math on the SALU
    const int my_steps = wv < nsteps ? (nsteps - wv + 3) / 4 : 0;
    u32x4 rb[DK][TN];
    auto bload = [&](int u, int it) {
        const int st = wv + 4 * (it < my_steps ? it : 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) rb[u][j] = *(const u32x4*)(wrow[j] + st * KS);
    };
#pragma unroll
    for (int u = 0; u < DK; ++u) bload(u, u);

    // ---- act(x) rows [m0 - hal, m0 + BM + hal) -> LDS (transformed once) ----
    stage_store(0);
    for (int q0 = 256 * SB; q0 < total; q0 += 256 * SB) {   // wide channels only
        stage_load(q0);
        stage_store(q0);
    }
    __syncthreads();

    // ---- per-lane pixel state ----
    int rowoff[TM];      // LDS element offset of the pixel's own row
    unsigned tvm[TM];    // bit tap set iff that tap of this output pixel is inside the image
    const float rW = 1.0f / (float)W, rH = 1.0f / (float)H;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int lp = i * 16 + li, m = m0 + lp;
        rowoff[i] = (lp + hal) * pitch;
        const int mm = m < M ? m : 0;
        const int row = fdiv_small(mm, rW);
        const int x = mm - row * W, y = row - fdiv_small(row, rH) * H;
        tvm[i] = tap_mask<KSZ>(x, y, W, H, m < M);
    }
    // K position of k = (wid + 4 it) * KS (+ g * CH for this lane).  UNI
    // (cs % KS == 0): a k-step never straddles a tap, so (tap, ci) are
    // wave-uniform (SALU) and the lane offset g * CH folds into rowoff.
    int tap, ci;
    {
        const int k = wv * KS + (UNI ? 0 : g * CH);
        tap = k / cs;
        ci = k - tap * cs;
    }
    if (UNI) {
#pragma unroll
        for (int i = 0; i < TM; ++i) rowoff[i] += g * CH;
    }
    const int zoff = UNI ? 0 : 0;

    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (int it0 = 0; it0 < my_steps; it0 += DK) {
#pragma unroll
        for (int u = 0; u < DK; ++u) {
            const int it = it0 + u;
            const int dy = tap / KSZ - PAD, dx = tap - (tap / KSZ) * KSZ - PAD;
            const int toff = (dy * W + dx) * pitch + ci;
            const bool live = it < my_steps;
            const int tsh = live ? tap : 31;   // bit 31 of tvm is never set
            u32x4 av[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const bool ok = (tvm[i] >> tsh) & 1u;
                const T* src = ok ? act + rowoff[i] + toff : zrow + zoff;
                av[i] = *(const u32x4*)src;
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) Mf<T>::step(rb[u][j], av[i], acc[i][j]);
            // refill this ring slot after its MFMAs (no register copies)
            bload(u, it + DK);
            // advance (tap, ci) by 4 k-steps; cs >= 2 * 4 * KS / 2 -> at most two wraps
            ci += 4 * KS;
            if (ci >= cs) { ci -= cs; ++tap; }
            if (ci >= cs) { ci -= cs; ++tap; }
        }
    }

    // ---- reduce the four partial tiles through LDS (aliases the act tile) ----
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) *(floatx4*)&red[(wid * BM + i * 16 + li) * RP + j * 16 + 4 * g] = acc[i][j];
    __syncthreads();

    const int fi = wid % TM, fj0 = (wid / TM) * FR;
    const int m = m0 + fi * 16 + li;
    const int cso = a.cs_out;
    double s1[FR][4], s2[FR][4];
#pragma unroll
    for (int f = 0; f < FR; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) s1[f][r] = s2[f][r] = 0.f;
    if (m < M) {
#pragma unroll
        for (int f = 0; f < FR; ++f) {
            const int col = (fj0 + f) * 16 + 4 * g;
            const int n = n0 + col;
            if (n >= cso) continue;
            floatx4 v = *(const floatx4*)&red[(fi * 16 + li) * RP + col];
#pragma unroll
            for (int w = 1; w < 4; ++w) v += *(const floatx4*)&red[(w * BM + fi * 16 + li) * RP + col];
            epi4<T>(a, (long long)m * cso + n, v, btab + col, epi_bn, etab + col, BN, s1[f], s2[f], N - n);
        }
    }
    const bool want_sums = a.out_sums || (epi_bn && a.epi_sums);
    if (want_sums) {
        row_stats16(s1, s2, li, [&](int f, int r, int which, double u) {
            const int col = (fj0 + f) * 16 + 4 * g + r;
            sred[(fi * BN + col) * 2 + which] = u;
        });
        __syncthreads();
        double* sums = (epi_bn ? a.epi_sums : a.out_sums) + (long long)(blockIdx.x % shards) * 2 * N;
        for (int col = tid; col < BN; col += 256) {
            const int n = n0 + col;
            if (n >= N) continue;
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int w = 0; w < TM; ++w) {
                t1 += sred[(w * BN + col) * 2];
                t2 += sred[(w * BN + col) * 2 + 1];
            }
            atomicAdd(&sums[n], (double)t1);
            atomicAdd(&sums[N + n], (double)t2);
        }
    }
}

template <typename T, int BN, int KSZ>
int launch_halo(const rnvp_conv_args* a, hipStream_t s) {
    const long long M = (long long)a->B * a->H * a->W;
    const long long gm = (M + 63) / 64, gn = (a->n + BN - 1) / BN;
    const size_t shm = halo_lds_bytes<T, BN>(a->cs_in, a->W, KSZ);
    const int sh = rnvp_stat_shards(M);
    const bool uni = a->cs_in % (4 * Mf<T>::CH) == 0;
    constexpr int DK = BN >= 64 ? 6 : 8;      // weight k-steps in flight per wave
    const unsigned grid = (unsigned)(gm * gn);
    if (a->pro_bn_relu) {
        if (uni) k_conv_halo<T, BN, KSZ, true, DK, true><<<grid, 256, shm, s>>>(*a, sh);
        else k_conv_halo<T, BN, KSZ, true, DK, false><<<grid, 256, shm, s>>>(*a, sh);
    } else {
        if (uni) k_conv_halo<T, BN, KSZ, false, DK, true><<<grid, 256, shm, s>>>(*a, sh);
        else k_conv_halo<T, BN, KSZ, false, DK, false><<<grid, 256, shm, s>>>(*a, sh);
    }
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// deep scales: few pixels, wide channels, the halo tile fits LDS
template <typename T>
bool halo_ok(const rnvp_conv_args* a) {
    const long long M = (long long)a->B * a->H * a->W;
    // measured against the LDS-tiled kernel: the halo tile wins at M <= 1024
    // (every shape) and for 3x3 at M <= 4096, loses above
    if (M > 4096 || (M > 1024 && a->ks != 3)) return false;
    if (a->cs_in < 64 || a->cs_in > DK_MAX_CS || a->n <= 16) return false;
    if (a->pro_bn_relu && a->pro.sums && a->pro.shards > 2) return false;
    if (a->epi_relu_bn_bwd && a->epi.sums && a->epi.shards > 2) return false;
    return halo_lds_bytes<T, 64>(a->cs_in, a->W, a->ks) <= 150 * 1024;
}

template <typename T>
int dispatch_halo(const rnvp_conv_args* a, hipStream_t s) {
    const long long M = (long long)a->B * a->H * a->W;
    // 64-channel tiles when that still gives >= 256 workgroups
    const bool wide = ((M + 63) / 64) * ((a->n + 63) / 64) >= 256;
    if (a->ks == 3) return wide ? launch_halo<T, 64, 3>(a, s) : launch_halo<T, 32, 3>(a, s);
    return wide ? launch_halo<T, 64, 1>(a, s) : launch_halo<T, 32, 1>(a, s);
}

}  // namespace

// M <= 1024 (3x3: <= 4096), 64 <= cs_in <= 1024, more than 16 outputs, BN
// sources of at most 2 stat shards, halo tile within 150 KiB of LDS
// (RNVP_E_UNSUPPORTED otherwise)
int rnvp_conv_halo_launch(const rnvp_conv_args* a, hipStream_t s) {
    if (a->dtype == RNVP_F32) return halo_ok<float>(a) ? dispatch_halo<float>(a, s) : RNVP_E_UNSUPPORTED;
    return halo_ok<bf16_t>(a) ? dispatch_halo<bf16_t>(a, s) : RNVP_E_UNSUPPORTED;
}
