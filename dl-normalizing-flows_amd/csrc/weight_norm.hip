// Weight normalisation of the conv weights: w = g v / ||v|| packed into the
// forward and data-gradient images the conv families read (and their
// fragment-major copies for the deep tiles), and its backward from the weight
// gradient slabs.  The fused backward + Adam pass lives in wn_adam.hip.
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"

namespace {

// ---------------------------------------------------------------------------
// weight normalisation
// ---------------------------------------------------------------------------
__device__ __forceinline__ int find_desc(const rnvp_wn_desc* d, int n, int row) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].row0 <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int find_tile(const rnvp_wn_desc* d, int n, int t) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].tile0 <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

constexpr int WN_ROW_LDS = 4608;

// Weight-norm forward, pass 1: ||v|| of every output row, one wave per row
// (coalesced 4-byte loads, 8 in flight per lane; v rows need not be 16-B
// aligned inside the parameter arena).  16-B loads (an aligned body between
// scalar head and tail) measured slower: 184 vs 147 us for config 1's rows.
__global__ __launch_bounds__(256) void k_wn_norm(const rnvp_wn_desc* __restrict__ descs, int n_desc, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const rnvp_wn_desc& d = descs[find_desc(descs, n_desc, row)];
    const int co = row - d.row0;
    const int kr = d.cin * d.ks * d.ks;
    const float* v = d.v + (long long)co * kr;
    double ss = 0.0;
    int i = lane;
    for (; i + 7 * 64 < kr; i += 8 * 64) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = v[i + u * 64];
#pragma unroll
        for (int u = 0; u < 8; ++u) ss = fma((double)x[u], (double)x[u], ss);
    }
    for (; i < kr; i += 64) ss = fma((double)v[i], (double)v[i], ss);
    ss = wave_sum(ss);
    if (lane == 0) d.norm[co] = (float)sqrt(ss);
}

// Pass 2: w = g v / ||v|| on tiles of WN_TCO output x WN_TCI input channels
// (all taps): the v tile is read once (runs of WN_TCI*ks*ks contiguous floats
// per output channel) into LDS, then written as both packed images in
// 4-element stores -- wf[co][tap*cs_in + ci] and the flipped, transposed
// wd[ci][tp*cs_out + co] = w[co][ci][ks*ks-1-tp].  The images' padding
// (ci >= cin, co >= cout, k >= ks*ks*cs) is zero from allocation and never
// written.
// A 1x1 conv's tile spans WN_TCI1 input channels (the same LDS row, ks*ks = 1
// float per channel): 8x fewer, 8x larger blocks than 32-channel tiles, with
// 512-byte forward-image runs.  With the XCD-contiguous tile order and
// float-reciprocal index math below, config 1's large refresh went from 376
// to 284 us (profiles/r2_small_kernel_sweeps.txt).
constexpr int WN_TCO = 32, WN_TCI = 32, WN_TCI1 = 256;

__host__ __device__ constexpr int wn_tci(int ks) { return ks == 1 ? WN_TCI1 : WN_TCI; }

// The fragment-major copies (rnvp_wn_desc.wf_frag / wd_frag, read by the deep
// tiles through rnvp_conv_args.w_frag) of one k_wn_pack / k_wn_wd tile
// ([32 co] x [32 ci] x 3x3, or [32 co] x [256 ci] for 1x1): block (row / 16,
// k / 32) of 512 elements, lane L = row % 16 + 16 * (k % 32 / 8) holding
// k % 8 = 0..7.  With cs_in, cs_out, co0 and ci0 multiples of 32 every block
// the tile touches lies wholly in it (per tap: 16 rows x 32 ci, resp. 16 ci x
// 32 co) and is written whole: 16-byte stores, 1 KiB per block.
// val(c, ci, tap) is the tile's value of w[co0 + c][ci0 + ci][tap] as the
// row-major image holds it (0 outside the conv's rows / channels).
template <typename T, typename F>
__device__ __forceinline__ void wn_frag_tile(const rnvp_wn_desc& d, int co0, int ci0, int nco, int ncc, F val) {
    if constexpr (sizeof(T) != 2) return;   // the deep tiles read fragment-major images in bf16 only
    const int kk = d.ks * d.ks;
    const int rbo = (nco + 15) >> 4, rbi = (ncc + 15) >> 4, nkb = (ncc + 31) >> 5;
    if (d.wf_frag) {
        for (int q = threadIdx.x; q < rbo * kk * nkb * 64; q += blockDim.x) {
            const int L = q & 63, r = q >> 6, kb = r % nkb, r2 = r / nkb, tap = r2 % kk, rb = r2 / kk;
            const int c = rb * 16 + (L & 15), ci = kb * 32 + (L >> 4) * 8;
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (c < nco && ci + e < ncc) ? val(c, ci + e, tap) : 0.f;
            T* dst = (T*)d.wf_frag +
                     ((long long)((co0 >> 4) + rb) * (d.kp_f >> 5) + ((tap * d.cs_in + ci0) >> 5) + kb) * 512 + L * 8;
            *(RNVP_GLOBAL u32x4*)dst = pack(f, T());
        }
    }
    if (d.wd_frag) {
        for (int q = threadIdx.x; q < rbi * kk * 64; q += blockDim.x) {
            const int L = q & 63, r = q >> 6, tp = r % kk, rb = r / kk;
            const int ci = rb * 16 + (L & 15), co = (L >> 4) * 8;
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (ci < ncc && co + e < nco) ? val(co + e, ci, kk - 1 - tp) : 0.f;
            T* dst = (T*)d.wd_frag + ((long long)((ci0 >> 4) + rb) * (d.kp_d >> 5) + ((tp * d.cs_out + co0) >> 5)) * 512 + L * 8;
            *(RNVP_GLOBAL u32x4*)dst = pack(f, T());
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_wn_pack(const rnvp_wn_desc* __restrict__ descs, int n_desc) {
    constexpr int TP = WN_TCI * 9 + 1;                      // LDS row pitch (floats), odd
    static_assert(WN_TCI1 < TP, "1x1 tile row must fit the LDS row");
    __shared__ float tile[WN_TCO * TP];
    __shared__ float scl[WN_TCO];
    // consecutive tiles (the two halves of a 128-byte line of either image)
    // on one XCD: block b runs on XCD b % 8, so remap b bijectively
    const int nb = gridDim.x, b = blockIdx.x;
    const int q8 = nb / 8, r8 = nb % 8, xcd = b % 8;
    const int tg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + b / 8;
    const rnvp_wn_desc& d = descs[find_tile(descs, n_desc, tg)];
    const int t = tg - d.tile0;
    const int tci = wn_tci(d.ks);
    const int nci = (d.cin + tci - 1) / tci;
    const int co0 = (t / nci) * WN_TCO, ci0 = (t % nci) * tci;
    const int kk = d.ks * d.ks, kr = d.cin * kk;
    const int nco = min(WN_TCO, d.cout - co0), ncc = min(tci, d.cin - ci0);
    const int run = ncc * kk;                               // contiguous floats per output channel
    if (threadIdx.x < WN_TCO) {
        const int co = co0 + threadIdx.x;
        scl[threadIdx.x] = (threadIdx.x < nco && d.g) ? d.g[co] / d.norm[co] : 1.f;
    }
    // item indices stay < 2^17: float-reciprocal divisions (fdiv_small)
    const float r_run = 1.0f / (float)run;
    for (int q = threadIdx.x; q < nco * run; q += 256) {
        const int c = fdiv_small(q, r_run), j = q - c * run;
        tile[c * TP + j] = d.v[(long long)(co0 + c) * kr + (long long)ci0 * kk + j];
    }
    __syncthreads();
    // forward image: 4 consecutive ci per item
    const int ng = (ncc + 3) / 4;
    const float r_kng = 1.0f / (float)(kk * ng), r_ng = 1.0f / (float)ng;
    for (int q = threadIdx.x; q < nco * kk * ng; q += 256) {
        const int c = fdiv_small(q, r_kng), r = q - c * (kk * ng), tap = fdiv_small(r, r_ng), c4 = (r - tap * ng) * 4;
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = c4 + e < ncc ? scl[c] * tile[c * TP + (c4 + e) * kk + tap] : 0.f;
        T* dst = (T*)d.wf + (long long)(co0 + c) * d.kp_f + tap * d.cs_in + ci0 + c4;
        if (c4 + 4 <= ncc) {
            st4(dst, w);
        } else {
            for (int e = 0; e < 4 && c4 + e < ncc; ++e) stv(dst + e, w[e]);
        }
    }
    wn_frag_tile<T>(d, co0, ci0, nco, ncc, [&](int c, int ci, int tap) { return scl[c] * tile[c * TP + ci * kk + tap]; });
    if (!d.wd) return;
    // data-gradient image: 4 consecutive co per item
    const int mg = (nco + 3) / 4;
    const float r_kmg = 1.0f / (float)(kk * mg), r_mg = 1.0f / (float)mg;
    for (int q = threadIdx.x; q < ncc * kk * mg; q += 256) {
        const int ci = fdiv_small(q, r_kmg), r = q - ci * (kk * mg), tp = fdiv_small(r, r_mg), o4 = (r - tp * mg) * 4;
        const int tap = kk - 1 - tp;
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = o4 + e < nco ? scl[o4 + e] * tile[(o4 + e) * TP + ci * kk + tap] : 0.f;
        T* dst = (T*)d.wd + (long long)(ci0 + ci) * d.kp_d + tp * d.cs_out + co0 + o4;
        if (o4 + 4 <= nco) {
            st4(dst, w);
        } else {
            for (int e = 0; e < 4 && o4 + e < nco; ++e) stv(dst + e, w[e]);
        }
    }
}

// The data-gradient image from the forward image: wd[ci][tp*cs_out + co] =
// wf[co][(ks*ks-1-tp)*cs_in + ci], on k_wn_pack's tiles (the same XCD order
// and LDS tile, read from the forward image instead of v -- the values are
// already g v / ||v|| rounded to T, so the two images stay bitwise what
// k_wn_pack writes).  Used after the fused parameter pass (wn_adam.hip),
// which writes the forward image row by row: a row of wd spans every output
// channel, so writing it from one row block would be RB-element scatter.
template <typename T>
__global__ __launch_bounds__(256) void k_wn_wd(const rnvp_wn_desc* __restrict__ descs, int n_desc) {
    constexpr int TP = WN_TCI * 9 + 1;
    __shared__ float tile[WN_TCO * TP];
    const int nb = gridDim.x, b = blockIdx.x;
    const int q8 = nb / 8, r8 = nb % 8, xcd = b % 8;
    const int tg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + b / 8;
    const rnvp_wn_desc& d = descs[find_tile(descs, n_desc, tg)];
    if (!d.wd) return;
    const int t = tg - d.tile0;
    const int tci = wn_tci(d.ks);
    const int nci = (d.cin + tci - 1) / tci;
    const int co0 = (t / nci) * WN_TCO, ci0 = (t % nci) * tci;
    const int kk = d.ks * d.ks;
    const int nco = min(WN_TCO, d.cout - co0), ncc = min(tci, d.cin - ci0);
    // tile[c][ci * kk + tap] (k_wn_pack's layout) from the forward image rows,
    // 8 input channels per item: ci0 and cs_in are multiples of 8 and a row's
    // channel padding (up to cs_in) is in bounds, so every group is one
    // aligned 16-byte (bf16) or two (fp32) loads
    const int ng = (ncc + 7) / 8;
    const float r_kg = 1.0f / (float)(kk * ng), r_g = 1.0f / (float)ng;
    const RNVP_GLOBAL T* wf = (const RNVP_GLOBAL T*)d.wf;
    // WD_U items' loads issued before any is used (a latency-bound loop
    // otherwise: one 16-byte load in flight per thread); a clamped duplicate
    // past the end reloads the thread's first item and is not stored
    constexpr int WD_U = 4, NV = sizeof(T) == 4 ? 2 : 1;
    const int nit = nco * kk * ng;
    for (int q0 = threadIdx.x; q0 < nit; q0 += WD_U * 256) {
        u32x4 v[WD_U][NV];
#pragma unroll
        for (int u = 0; u < WD_U; ++u) {
            const int q = q0 + u * 256 < nit ? q0 + u * 256 : q0;
            const int c = fdiv_small(q, r_kg), r = q - c * (kk * ng), tap = fdiv_small(r, r_g), c8 = (r - tap * ng) * 8;
            const RNVP_GLOBAL T* src = wf + (long long)(co0 + c) * d.kp_f + tap * d.cs_in + ci0 + c8;
#pragma unroll
            for (int h = 0; h < NV; ++h) v[u][h] = *(const RNVP_GLOBAL u32x4*)(src + 4 * h);
        }
#pragma unroll
        for (int u = 0; u < WD_U; ++u) {
            const int q = q0 + u * 256;
            if (q >= nit) break;
            const int c = fdiv_small(q, r_kg), r = q - c * (kk * ng), tap = fdiv_small(r, r_g), c8 = (r - tap * ng) * 8;
            float f[8];
            unpack(v[u][0], f, T());
            if constexpr (NV == 2) unpack(v[u][1], f + 4, T());
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c8 + e < ncc) tile[c * TP + (c8 + e) * kk + tap] = f[e];
        }
    }
    __syncthreads();
    wn_frag_tile<T>(d, co0, ci0, nco, ncc, [&](int c, int ci, int tap) { return tile[c * TP + ci * kk + tap]; });
    // 8 consecutive output channels per item: one 16-byte store (bf16)
    const int mg = (nco + 7) / 8;
    const float r_kmg = 1.0f / (float)(kk * mg), r_mg = 1.0f / (float)mg;
    for (int q = threadIdx.x; q < ncc * kk * mg; q += 256) {
        const int ci = fdiv_small(q, r_kmg), r = q - ci * (kk * mg), tp = fdiv_small(r, r_mg), o8 = (r - tp * mg) * 8;
        const int tap = kk - 1 - tp;
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = o8 + e < nco ? tile[(o8 + e) * TP + ci * kk + tap] : 0.f;
        T* dst = (T*)d.wd + (long long)(ci0 + ci) * d.kp_d + tp * d.cs_out + co0 + o8;
        if (o8 + 8 <= nco) {
            if constexpr (sizeof(T) == 2) {
                *(RNVP_GLOBAL u32x4*)dst = pack(w, T());
            } else {
                *(RNVP_GLOBAL u32x4*)dst = pack(w, T());
                *(RNVP_GLOBAL u32x4*)(dst + 4) = pack(w + 4, T());
            }
        } else {
            for (int e = 0; e < 8 && o8 + e < nco; ++e) stg(dst + e, w[e]);
        }
    }
}

// one block per output row co: dW row = sum of the nz partial slabs, gathered
// into LDS in v's [ci][tap] order (coalesced over the packed k), then the
// weight-norm backward and the bias partial sum.

// bias sum over the replicas, and re-zeroing of the replicas (zero_after)
__device__ __forceinline__ void wn_bwd_tail(const rnvp_wn_desc& d, float* gbase, int co, int nz, long long zs,
                                            double* red) {
    if (d.dbp) {
        float bs = 0.f;
        for (int z = threadIdx.x; z < nz; z += blockDim.x) bs += d.dbp[(long long)z * d.cout + co];
        bs = block_sum(bs, (float*)red);
        if (threadIdx.x == 0) gbase[d.db_off + co] = bs;
        if (d.zero_after) {
            __syncthreads();
            for (int z = threadIdx.x; z < nz; z += blockDim.x) d.dbp[(long long)z * d.cout + co] = 0.f;
        }
    }
    if (d.zero_after) {   // leave the replicas zero for the next atomic accumulation
        __syncthreads();
        RNVP_GLOBAL float* dwz = (RNVP_GLOBAL float*)(d.dw + (long long)co * d.kp_f);
        const int K = d.ks * d.ks * d.cs_in;
        if ((K & 3) == 0 && (zs & 3) == 0 && (((uintptr_t)dwz) & 15) == 0) {
            for (int z = 0; z < nz; ++z)
                for (int k = 4 * threadIdx.x; k < K; k += 4 * blockDim.x)
                    *(RNVP_GLOBAL floatx4*)(dwz + z * zs + k) = floatx4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int z = 0; z < nz; ++z)
                for (int k = threadIdx.x; k < K; k += blockDim.x) dwz[z * zs + k] = 0.f;
        }
    }
}

__global__ void k_wn_bwd(const rnvp_wn_desc* __restrict__ descs, int n_desc, float* gbase, int rows, double* z0,
                         long long n0, double* z1, long long n1) {
    if ((int)blockIdx.x >= rows) {   // extra workgroups: zero the caller's sums ranges
        const long long stride = (long long)(gridDim.x - rows) * blockDim.x;
        const long long i0 = (long long)(blockIdx.x - rows) * blockDim.x + threadIdx.x;
        for (long long i = i0; i < n0; i += stride) z0[i] = 0.0;
        for (long long i = i0; i < n1; i += stride) z1[i] = 0.0;
        return;
    }
    __shared__ double red[16];
    __shared__ float rowbuf[WN_ROW_LDS];
    const int row = blockIdx.x;
    const rnvp_wn_desc d = descs[find_desc(descs, n_desc, row)];
    const int co = row - d.row0;
    const int kk = d.ks * d.ks, kr = d.cin * kk;
    const int nz = d.nz > 0 ? d.nz : 1;
    const long long zs = (long long)d.cout * d.kp_f;
    const float* v = d.v + (long long)co * kr;
    const float* dw = d.dw + (long long)co * d.kp_f;
    const bool in_lds = kr <= WN_ROW_LDS;
    auto dw_at = [&](int k) {
        float t = 0.f;
        for (int z = 0; z < nz; ++z) t += dw[z * zs + k];
        return t;
    };
    if (in_lds && blockDim.x == 256 && nz <= 8 && kk * d.cs_in <= WN_ROW_LDS) {
        // one memory round trip: every load of the row is issued up front --
        // this thread's v elements (kept in registers for both passes) and its
        // float4 chunks of the packed dW row, summed over the nz replicas --
        // then the dW row is gathered into v's [ci][tap] order in LDS
        constexpr int PT = WN_ROW_LDS / 256, P4 = (WN_ROW_LDS / 4 + 255) / 256;
        const int K4 = kk * d.cs_in / 4;            // cs_in % 8 == 0: a chunk never straddles a tap
        const float rcs = 1.0f / (float)d.cs_in;
        const RNVP_GLOBAL float* vg = (const RNVP_GLOBAL float*)v;
        float vr[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int i = threadIdx.x + j * 256;
            vr[j] = vg[i < kr ? i : 0];
        }
        float4 cw[P4];
#pragma unroll
        for (int j = 0; j < P4; ++j) {
            const int q4 = threadIdx.x + j * 256;
            const RNVP_GLOBAL floatx4* src = (const RNVP_GLOBAL floatx4*)dw + (q4 < K4 ? q4 : 0);
            floatx4 t = src[0];
#pragma unroll
            for (int z = 1; z < 8; ++z) {
                if (z < nz) t += src[z * zs / 4];
            }
            cw[j] = float4{t.x, t.y, t.z, t.w};
        }
#pragma unroll
        for (int j = 0; j < P4; ++j) {
            const int q4 = threadIdx.x + j * 256;
            if (q4 < K4) {
                const int k = 4 * q4, tap = fdiv_small(k, rcs), ci = k - tap * d.cs_in;
                const float e[4] = {cw[j].x, cw[j].y, cw[j].z, cw[j].w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (ci + u < d.cin) rowbuf[(ci + u) * kk + tap] = e[u];
            }
        }
        __syncthreads();
        float dr[PT];
        double dot = 0;
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int i = threadIdx.x + j * 256;
            dr[j] = i < kr ? rowbuf[i] : 0.f;
            dot = fma((double)dr[j], (double)vr[j], dot);
        }
        dot = block_sum(dot, red);
        RNVP_GLOBAL float* dv = (RNVP_GLOBAL float*)(gbase + d.dv_off + (long long)co * kr);
        if (d.g) {
            const float nrm = d.norm[co];
            const float gs = d.g[co] / nrm;
            const float proj = (float)(dot / ((double)nrm * nrm));
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int i = threadIdx.x + j * 256;
                if (i < kr) dv[i] = gs * fmaf(-proj, vr[j], dr[j]);
            }
            if (threadIdx.x == 0 && d.dg_off >= 0) gbase[d.dg_off + co] = (float)(dot / nrm);
        } else {
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int i = threadIdx.x + j * 256;
                if (i < kr) dv[i] = dr[j];
            }
        }
        wn_bwd_tail(d, gbase, co, nz, zs, red);
        return;
    }
    if (in_lds) {
        const int K = kk * d.cs_in;
        const float rcs = 1.0f / (float)d.cs_in;
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            const int tap = fdiv_small(k, rcs), ci = k - tap * d.cs_in;
            if (ci < d.cin) rowbuf[ci * kk + tap] = dw_at(k);
        }
        __syncthreads();
    }
    auto dwv = [&](int i) {
        if (in_lds) return rowbuf[i];
        const int ci = i / kk, tap = i - ci * kk;
        return dw_at(tap * d.cs_in + ci);
    };
    double dot = 0;
    for (int i = threadIdx.x; i < kr; i += blockDim.x) dot = fma((double)dwv(i), (double)v[i], dot);
    dot = block_sum(dot, red);
    float* dv = gbase + d.dv_off + (long long)co * kr;
    if (d.g) {
        const float nrm = d.norm[co];
        const float gs = d.g[co] / nrm;
        const float proj = (float)(dot / ((double)nrm * nrm));
        for (int i = threadIdx.x; i < kr; i += blockDim.x) dv[i] = gs * fmaf(-proj, v[i], dwv(i));
        if (threadIdx.x == 0 && d.dg_off >= 0) gbase[d.dg_off + co] = (float)(dot / nrm);
    } else {
        for (int i = threadIdx.x; i < kr; i += blockDim.x) dv[i] = dwv(i);
    }
    wn_bwd_tail(d, gbase, co, nz, zs, red);
}

}  // namespace

extern "C" int rnvp_weight_norm_tiles(int cout, int cin, int ks) {
    if (cout <= 0 || cin <= 0 || (ks != 1 && ks != 3)) return RNVP_E_INVALID;
    return ((cout + WN_TCO - 1) / WN_TCO) * ((cin + wn_tci(ks) - 1) / wn_tci(ks));
}

extern "C" int rnvp_weight_norm_fwd(const rnvp_wn_desc* d, int n_desc, int total_rows, int total_tiles, int dtype,
                                    void* stream) {
    if (!d || n_desc <= 0 || total_rows <= 0 || total_tiles <= 0) return RNVP_E_INVALID;
    if (dtype != RNVP_F32 && dtype != RNVP_BF16) return RNVP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    k_wn_norm<<<(total_rows + 3) / 4, 256, 0, s>>>(d, n_desc, total_rows);
    RNVP_LAUNCH_CHECK();
    if (dtype == RNVP_F32) k_wn_pack<float><<<total_tiles, 256, 0, s>>>(d, n_desc);
    else k_wn_pack<bf16_t><<<total_tiles, 256, 0, s>>>(d, n_desc);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_weight_norm_transpose(const rnvp_wn_desc* d, int n_desc, int total_tiles, int dtype, void* stream) {
    if (!d || n_desc <= 0 || total_tiles <= 0) return RNVP_E_INVALID;
    if (dtype != RNVP_F32 && dtype != RNVP_BF16) return RNVP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RNVP_F32) k_wn_wd<float><<<total_tiles, 256, 0, s>>>(d, n_desc);
    else k_wn_wd<bf16_t><<<total_tiles, 256, 0, s>>>(d, n_desc);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

extern "C" int rnvp_weight_norm_bwd(const rnvp_wn_desc* d, int n_desc, int total_rows, float* grad_base, void* zero0,
                                    long long zero0_bytes, void* zero1, long long zero1_bytes, void* stream) {
    if (!d || !grad_base || n_desc <= 0 || total_rows <= 0) return RNVP_E_INVALID;
    if (zero0_bytes < 0 || zero1_bytes < 0 || (zero0_bytes & 7) || (zero1_bytes & 7)) return RNVP_E_INVALID;
    if ((zero0_bytes && (!zero0 || ((uintptr_t)zero0 & 7))) || (zero1_bytes && (!zero1 || ((uintptr_t)zero1 & 7))))
        return RNVP_E_INVALID;
    const long long nz = (zero0_bytes > zero1_bytes ? zero0_bytes : zero1_bytes) / 8;
    const int extra = nz > 0 ? (int)((nz + 255) / 256 < 16 ? (nz + 255) / 256 : 16) : 0;
    k_wn_bwd<<<total_rows + extra, 256, 0, (hipStream_t)stream>>>(d, n_desc, grad_base, total_rows, (double*)zero0,
                                                                  zero0_bytes / 8, (double*)zero1, zero1_bytes / 8);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}
