// Deep-scale conv family, the instantiating templates: the kernels around
// conv_deep.h's tile body and the launchers that pick one by channel-chunk
// count, prologue and weight layout.  Compiling them dominates the library's
// build, so conv_deep_inst.hip instantiates them once per (dtype,
// configuration) in objects of their own; conv_deep.hip (the policy) calls the
// two per-configuration entry points at the end of this file through their
// declarations in conv_common.h.
#pragma once
#include "conv_deep.h"

namespace {

template <typename T, int BN, int KSZ, bool PRO, int NW, int WK, int DK, int NC, bool FM = false, int BM = DEEP_BM,
          bool BP = false>
__global__ __launch_bounds__(64 * NW) void k_conv_deep(rnvp_conv_args a, int shards, int xa, int xb) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    deep_tile<T, BN, KSZ, PRO, NW, WK, DK, NC, FM, BM, BP>(a, shards, xa, xb, blockIdx.x, gridDim.x, lds);
}

// the BatchNorm-backward prologue (a->bp) is compiled for the data-gradient
// configurations only: 32-channel tiles, whole tile per wave, 64 pixels
// (rnvp_deep_auto_cfg's cfg 0 / 4)
template <int BN, int NW, int WK, int BM>
constexpr bool bp_cfg() { return BN == 32 && WK == NW && BM == DEEP_BM; }

// dry: every check, nothing launched (rnvp_conv2d_check)
template <typename T, int BN, int NW, int WK, int DK, int NC, int KSZ, int BM = DEEP_BM>
int launch_deep_nc(const rnvp_conv_args* a, hipStream_t s, bool dry) {
    const long long M = (long long)a->B * a->H * a->W;
    const size_t shm = deep_lds_bytes<T, BN, NW, WK, BM>(a->cs_in, a->W, a->ks, a->bp != 0);
    if (shm > 160 * 1024) return RNVP_E_UNSUPPORTED;
    const long long gm = (M + BM - 1) / BM, gn = (a->n + BN - 1) / BN;
    const unsigned grid = (unsigned)(gm * gn);
    const int sh = rnvp_stat_shards(M);
    const dim3 blk(64 * NW);
    int xa, xb;
    xcd_blocks(a, (int)gm, (int)gn, BN, sizeof(T), &xa, &xb, BM);
    if (a->bp) {
        if constexpr (bp_cfg<BN, NW, WK, BM>()) {
            if (dry) return RNVP_OK;
            if constexpr (sizeof(T) == 2 && NC <= 4) {
                if (a->w_frag) {
                    k_conv_deep<T, BN, KSZ, false, NW, WK, DK, NC, true, BM, true><<<grid, blk, shm, s>>>(*a, sh, xa, xb);
                    RNVP_LAUNCH_CHECK();
                    return RNVP_OK;
                }
            }
            k_conv_deep<T, BN, KSZ, false, NW, WK, DK, NC, false, BM, true><<<grid, blk, shm, s>>>(*a, sh, xa, xb);
            RNVP_LAUNCH_CHECK();
            return RNVP_OK;
        } else {
            return RNVP_E_UNSUPPORTED;
        }
    }
    if (dry) return RNVP_OK;
    // the fragment-major weight image where the caller provides one (bf16)
    if constexpr (sizeof(T) == 2 && NC <= 4) {
        if (a->w_frag) {
            if (a->pro_bn_relu) k_conv_deep<T, BN, KSZ, true, NW, WK, DK, NC, true, BM><<<grid, blk, shm, s>>>(*a, sh, xa, xb);
            else k_conv_deep<T, BN, KSZ, false, NW, WK, DK, NC, true, BM><<<grid, blk, shm, s>>>(*a, sh, xa, xb);
            RNVP_LAUNCH_CHECK();
            return RNVP_OK;
        }
    }
    if (a->pro_bn_relu) k_conv_deep<T, BN, KSZ, true, NW, WK, DK, NC, false, BM><<<grid, blk, shm, s>>>(*a, sh, xa, xb);
    else k_conv_deep<T, BN, KSZ, false, NW, WK, DK, NC, false, BM><<<grid, blk, shm, s>>>(*a, sh, xa, xb);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}

// channel chunks per wave NC = cs / (WK * KS), a template parameter (the
// k-step sequence is unrolled): the channel strides of the RealNVP nets
template <typename T, int BN, int NW, int WK, int DK>
int launch_deep(const rnvp_conv_args* a, hipStream_t s, bool dry) {
    constexpr int KS = 4 * Mf<T>::CH;
    const long long M = (long long)a->B * a->H * a->W;
    if (M > 65536 || a->n < BN / 2 || a->cs_in % (WK * KS)) return RNVP_E_UNSUPPORTED;
    if (a->pro_bn_relu && a->pro.sums && a->pro.shards > 2) return RNVP_E_UNSUPPORTED;
    if (a->epi_relu_bn_bwd && a->epi.sums && a->epi.shards > 2) return RNVP_E_UNSUPPORTED;
    if (a->cs_in > DEEP_MAX_CS) return RNVP_E_UNSUPPORTED;
    if (a->bp && (a->pro_bn_relu || (a->bp_bn.sums && a->bp_bn.shards > 2) || a->bp_shards > 2)) return RNVP_E_UNSUPPORTED;
    const int nc = a->cs_in / (WK * KS);
    if (a->ks == 1) {
        switch (nc) {
            case 1: return launch_deep_nc<T, BN, NW, WK, DK, 1, 1>(a, s, dry);
            case 2: return launch_deep_nc<T, BN, NW, WK, DK, 2, 1>(a, s, dry);
            case 4: return launch_deep_nc<T, BN, NW, WK, DK, 4, 1>(a, s, dry);
            case 8: return launch_deep_nc<T, BN, NW, WK, DK, 8, 1>(a, s, dry);
            case 16: return launch_deep_nc<T, BN, NW, WK, DK, 16, 1>(a, s, dry);
        }
        return RNVP_E_UNSUPPORTED;
    }
    if constexpr (WK == NW) {   // 3x3: whole-tile-per-wave configurations only
        switch (nc) {
            case 1: return launch_deep_nc<T, BN, NW, WK, DK, 1, 3>(a, s, dry);
            case 2: return launch_deep_nc<T, BN, NW, WK, DK, 2, 3>(a, s, dry);
            case 4: return launch_deep_nc<T, BN, NW, WK, DK, 4, 3>(a, s, dry);
            case 8: return launch_deep_nc<T, BN, NW, WK, DK, 8, 3>(a, s, dry);
        }
    }
    return RNVP_E_UNSUPPORTED;
}

// 128-pixel 3x3 tiles (bf16, <= 4 channel chunks per wave): each weight
// slice serves twice the pixels of the 64-pixel tiles
template <typename T, int BN, int NW, int WK, int DK>
int launch_deep_tall(const rnvp_conv_args* a, hipStream_t s, bool dry) {
    constexpr int KS = 4 * Mf<T>::CH;
    if constexpr (sizeof(T) != 2) {
        return RNVP_E_UNSUPPORTED;
    } else {
        const long long M = (long long)a->B * a->H * a->W;
        if (a->ks != 3 || M > 65536 || a->n < BN / 2 || a->cs_in % (WK * KS)) return RNVP_E_UNSUPPORTED;
        if (a->pro_bn_relu && a->pro.sums && a->pro.shards > 2) return RNVP_E_UNSUPPORTED;
        if (a->epi_relu_bn_bwd && a->epi.sums && a->epi.shards > 2) return RNVP_E_UNSUPPORTED;
        switch (a->cs_in / (WK * KS)) {
            case 1: return launch_deep_nc<T, BN, NW, WK, DK, 1, 3, 128>(a, s, dry);
            case 2: return launch_deep_nc<T, BN, NW, WK, DK, 2, 3, 128>(a, s, dry);
            case 4: return launch_deep_nc<T, BN, NW, WK, DK, 4, 3, 128>(a, s, dry);
        }
        return RNVP_E_UNSUPPORTED;
    }
}

// ---------------------------------------------------------------------------
// grouped independent 1x1 convs: one launch, the convs' tiles concatenated
// (block b -> the conv whose tile range holds b; every conv keeps its own
// XCD-aware tile order).  Both prologue forms are compiled in.
template <typename T, int BN, int NW, int WK, int DK, int NC, bool FM = false>
__global__ __launch_bounds__(64 * NW) void k_net_group(const rnvp_group_kargs g) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int b = blockIdx.x, c = 0;
    while (c + 1 < g.n && b >= g.tiles[c]) {   // uniform scan over <= RNVP_NET_GROUP_MAX tile counts
        b -= g.tiles[c];
        ++c;
    }
    if (g.conv[c].pro_bn_relu)
        deep_tile<T, BN, 1, true, NW, WK, DK, NC, FM>(g.conv[c], g.shards[c], g.xa[c], g.xb[c], b, g.tiles[c], lds);
    else
        deep_tile<T, BN, 1, false, NW, WK, DK, NC, FM>(g.conv[c], g.shards[c], g.xa[c], g.xb[c], b, g.tiles[c], lds);
}

template <typename T, int BN, int NW, int WK, int DK>
GroupKernel group_kernel_nc(int nc, bool fm) {
    if constexpr (sizeof(T) == 2) {
        if (fm) {   // every member carries a fragment-major weight image
            switch (nc) {
                case 1: return k_net_group<T, BN, NW, WK, DK, 1, true>;
                case 2: return k_net_group<T, BN, NW, WK, DK, 2, true>;
                case 4: return k_net_group<T, BN, NW, WK, DK, 4, true>;
            }
            return nullptr;
        }
    }
    if (fm) return nullptr;
    switch (nc) {
        case 1: return k_net_group<T, BN, NW, WK, DK, 1>;
        case 2: return k_net_group<T, BN, NW, WK, DK, 2>;
        case 4: return k_net_group<T, BN, NW, WK, DK, 4>;
        case 8: return k_net_group<T, BN, NW, WK, DK, 8>;
        case 16: return k_net_group<T, BN, NW, WK, DK, 16>;
    }
    return nullptr;
}

}  // namespace

//                       BN  NW  WK  DK
// cfg 0                 32   4   4   8   whole 64x32 tile per wave, K / 4 (deep K)
// cfg 1                 64   4   4   6   whole 64x64 tile per wave, K / 4
// cfg 2                 64   4   1   8   16-pixel quarters, all of K (1x1, small K)
// cfg 3                 32   4   2   8   32-pixel halves x K / 2
// cfg 4                 32   8   8   8   cfg 0 with 8 waves (two per SIMD: one's memory waits under the other's MFMAs)
// cfg 5                 64   8   8   6   cfg 1 with 8 waves
// cfg 6                 32   4   4   8   cfg 0 on 128-pixel tiles (bf16 3x3)
template <typename T, int CFG>
int rnvp_deep_cfg_launch(const rnvp_conv_args* a, hipStream_t s, bool dry) {
    static_assert(CFG >= 0 && CFG < RNVP_DEEP_CFGS, "configuration");
    if constexpr (CFG == 0) return launch_deep<T, 32, 4, 4, 8>(a, s, dry);
    if constexpr (CFG == 1) return launch_deep<T, 64, 4, 4, 6>(a, s, dry);
    if constexpr (CFG == 2) return a->ks == 1 ? launch_deep<T, 64, 4, 1, 8>(a, s, dry) : RNVP_E_UNSUPPORTED;
    if constexpr (CFG == 3) return a->ks == 1 ? launch_deep<T, 32, 4, 2, 8>(a, s, dry) : RNVP_E_UNSUPPORTED;
    if constexpr (CFG == 4) return launch_deep<T, 32, 8, 8, 8>(a, s, dry);
    if constexpr (CFG == 5) return launch_deep<T, 64, 8, 8, 6>(a, s, dry);
    if constexpr (CFG == 6) return launch_deep_tall<T, 32, 4, 4, 8>(a, s, dry);
}

// the grouped kernel of configuration 0 / 1 / 4 / 5 (the table above)
template <typename T, int CFG>
GroupKernel rnvp_deep_cfg_group(int nc, bool fm) {
    static_assert(CFG == 0 || CFG == 1 || CFG == 4 || CFG == 5, "whole-tile-per-wave configurations");
    if constexpr (CFG == 0) return group_kernel_nc<T, 32, 4, 4, 8>(nc, fm);
    if constexpr (CFG == 1) return group_kernel_nc<T, 64, 4, 4, 6>(nc, fm);
    if constexpr (CFG == 4) return group_kernel_nc<T, 32, 8, 8, 8>(nc, fm);
    if constexpr (CFG == 5) return group_kernel_nc<T, 64, 8, 8, 6>(nc, fm);
}
