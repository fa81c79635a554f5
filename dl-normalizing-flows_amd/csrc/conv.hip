// rnvp_conv2d: argument checks and the routing of a conv to a kernel family.
//
// Every family computes the same fused operation (BatchNorm+ReLU of the
// operand, bias / residual / skip accumulation, the next BatchNorm's batch
// sums, or the data-gradient ReLU/BN-backward epilogue) and exports one
// launcher (conv_common.h) that returns RNVP_E_UNSUPPORTED outside its
// domain.  dispatch_conv tries them in this order; the first that does not
// decline runs:
//
//   1. deep (conv_deep.hip)      M <= 16384 pixels, 128..1024 channels: LDS
//                                activation tile + streamed weights.  variant
//                                0 / RNVP_VARIANT_DEEP: rnvp_deep_auto_cfg's
//                                configuration; RNVP_VARIANT_DEEP0 + c: forced
//                                configuration c, no fallback
//   2. s1 (conv_s1.hip)          bf16 1x1, <= 64 channels, M >= 16k: the
//                                register-pipelined stream kernel
//   3. band (conv_band.hip,      3x3, <= 64 channels, 32k <= M < 2^21
//      then conv_band1.hip)      (rnvp_conv_band_ok): the persistent band
//                                kernel, else one band per workgroup
//   4. stream (conv_stream.hip)  <= 64 channels, weights fit LDS: pixel
//                                fragments streamed through registers
//   5. halo (conv_halo.hip)      M <= 4096, 64..1024 channels: halo tile in
//                                LDS, the four waves split K
//   6. tiled (conv_tiled.hip)    everything else: LDS-tiled implicit GEMM
//                                with split-K
//
// variant 1 (the untuned baseline) skips 1, 2, 3 and 5.  A conv with a
// BatchNorm-backward prologue (a->bp) runs on the families that have one:
// deep's data-gradient configurations (bp_cfg_of), s1, band.
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"

#ifndef RNVP_SHARD_PX
#define RNVP_SHARD_PX 8192
#endif
extern "C" int rnvp_stat_shards(long long M) {
    long long s = M / RNVP_SHARD_PX;
    int r = 1;
    while (r < 32 && r * 2 <= s) r *= 2;
    return r;
}

namespace {

// argument checks shared by rnvp_conv2d and rnvp_conv2d_check
int conv_args_status(const rnvp_conv_args* a) {
    if (!a || !a->x || !a->w || !a->y) return RNVP_E_INVALID;
    if (a->variant < 0 || (a->variant > RNVP_VARIANT_DEEP && a->variant < RNVP_VARIANT_DEEP0) ||
        a->variant >= RNVP_VARIANT_DEEP0 + RNVP_DEEP_CFGS)
        return RNVP_E_INVALID;
    if (a->w_frag && !al16(a->w_frag)) return RNVP_E_INVALID;
    if (a->dtype != RNVP_F32 && a->dtype != RNVP_BF16) return RNVP_E_INVALID;
    if (a->ks != 1 && a->ks != 3) return RNVP_E_UNSUPPORTED;
    if (a->B < 0 || a->H <= 0 || a->W <= 0 || a->n <= 0 || a->cin <= 0) return RNVP_E_INVALID;
    if ((a->cs_in & 7) || (a->cs_out & 7) || a->cs_in < a->cin || a->cs_out < a->n) return RNVP_E_INVALID;
    if ((a->kp & 63) || a->kp < a->ks * a->ks * a->cs_in) return RNVP_E_INVALID;
    if (!al16(a->x) || !al16(a->w)) return RNVP_E_INVALID;
    if (a->epi_relu_bn_bwd && !a->epi_x) return RNVP_E_INVALID;
    // a finalized table stands for batch sums: 16-byte entries, train mode only
    auto tab_bad = [](const rnvp_bn_src& s) { return s.tab && (!s.sums || !al16(s.tab)); };
    if ((a->pro_bn_relu && tab_bad(a->pro)) || (a->epi_relu_bn_bwd && tab_bad(a->epi)) || (a->bp && tab_bad(a->bp_bn)))
        return RNVP_E_INVALID;
    if ((long long)a->B * a->H * a->W >= (1ll << 31)) return RNVP_E_UNSUPPORTED;
    if (a->bp) {
        if (!a->bp_x || !al16(a->bp_x) || (a->bp_out && !al16(a->bp_out))) return RNVP_E_INVALID;
        if (a->bp_bn.sums && (!a->bp_sums || a->bp_shards < 1 || a->bp_bn.count <= 0)) return RNVP_E_INVALID;
        if (!a->bp_bn.sums && (!a->bp_bn.mean || !a->bp_bn.var)) return RNVP_E_INVALID;
        if (a->pro_bn_relu) return RNVP_E_INVALID;
    }
    return RNVP_OK;
}

// the configuration a BatchNorm-backward prologue runs on: the deep family's
// data-gradient tiles only (the other families have no such prologue).  The
// tuned dispatch folds where that measured faster than the apply's launch +
// the plain conv (tools/probe/deep_stamps.py bp / bp8, profiles/r6_bnfold.txt):
// the 3x3 tiles, the 8-wave tiles and the 4-wave 1x1 tiles up to 4096 pixels
// (+2.8 us against a ~5.7 us apply); at 16384 pixels the 4-wave 1x1 tile loses
// a wave per SIMD to the prologue's registers (+7.8 us) and keeps the apply (a
// forced deep configuration still runs it)
int bp_cfg_of(const rnvp_conv_args* a) {
    if (a->variant >= RNVP_VARIANT_DEEP0) {
        const int cfg = a->variant - RNVP_VARIANT_DEEP0;
        return (cfg == 0 || cfg == 4) ? cfg : -1;
    }
    if (a->variant != 0 && a->variant != RNVP_VARIANT_DEEP) return -1;
    const int cfg = rnvp_deep_auto_cfg(a);
    const long long M = (long long)a->B * a->H * a->W;
    if (cfg == 4 || (cfg == 0 && (a->ks == 3 || M <= 4096))) return cfg;
    return -1;
}

// dry: the routing's checks only, nothing launched; fam (optional): the
// family that runs (RNVP_FAMILY_*) -- rnvp_conv2d_family asks the dispatch
// itself.  Only the families with a dry launcher are told apart; the
// dispatch has a family for every shape that passes the argument checks.
int dispatch_conv(const rnvp_conv_args* a, hipStream_t s, bool dry, int* fam) {
    auto ran = [&](int f, int r) {
        if (fam && r == RNVP_OK) *fam = f;
        return r;
    };
    // forced deep-scale configuration (A/B and parity tests): no fallback
    if (a->variant >= RNVP_VARIANT_DEEP0)
        return ran(RNVP_FAMILY_DEEP, rnvp_deep_launch(a, s, a->variant - RNVP_VARIANT_DEEP0, dry));
    if (a->variant == 0 || a->variant == RNVP_VARIANT_DEEP) {
        const int cfg = rnvp_deep_auto_cfg(a);
        if (cfg >= 0) {
            const int r = rnvp_deep_launch(a, s, cfg, dry);
            if (r != RNVP_E_UNSUPPORTED) return ran(RNVP_FAMILY_DEEP, r);
        }
    }
    const bool tuned = a->variant != 1;
    // bf16 1x1 convs of the wide scales: the register-pipelined stream kernel (conv_s1.hip)
    if (tuned && a->dtype == RNVP_BF16 && a->ks == 1) {
        const int r = rnvp_conv_s1_launch(a, s, dry);
        if (r != RNVP_E_UNSUPPORTED) return ran(RNVP_FAMILY_S1, r);
    }
    if (tuned && rnvp_conv_band_ok(a)) {
        // the persistent band kernel (conv_band.hip) where it applies
        const int r = rnvp_conv_band2_launch(a, s, dry);
        if (r != RNVP_E_UNSUPPORTED) return ran(RNVP_FAMILY_BAND, r);
        if (dry) return ran(RNVP_FAMILY_OTHER, RNVP_OK);
        return rnvp_conv_band1_launch(a, s);
    }
    if (dry) return ran(RNVP_FAMILY_OTHER, RNVP_OK);
    {
        const int r = rnvp_conv_stream_launch(a, s);
        if (r != RNVP_E_UNSUPPORTED) return r;
    }
    if (tuned) {
        const int r = rnvp_conv_halo_launch(a, s);
        if (r != RNVP_E_UNSUPPORTED) return r;
    }
    return rnvp_conv_tiled_launch(a, s);
}

// the whole routing of a checked conv; dry: every check, nothing launched
// (rnvp_conv2d_check, rnvp_conv2d_family)
int route_conv(const rnvp_conv_args* a, hipStream_t s, bool dry, int* fam = nullptr) {
    if (a->bp) {
        const int cfg = bp_cfg_of(a);
        int r, f = RNVP_FAMILY_DEEP;
        if (cfg >= 0) {
            r = rnvp_deep_launch(a, s, cfg, dry);
        } else {
            // the wide scales' streaming 1x1 and band 3x3 (bf16) have the prologue too
            if (a->variant != 0) return RNVP_E_UNSUPPORTED;
            f = RNVP_FAMILY_S1;
            r = rnvp_conv_s1_launch(a, s, dry);
            if (r == RNVP_E_UNSUPPORTED) {
                f = RNVP_FAMILY_BAND;
                r = rnvp_conv_band2_launch(a, s, dry);
            }
        }
        if (fam && r == RNVP_OK) *fam = f;
        return r;
    }
    return dispatch_conv(a, s, dry, fam);
}

}  // namespace

extern "C" int rnvp_conv2d(const rnvp_conv_args* a, void* stream) {
    const int st = conv_args_status(a);
    if (st != RNVP_OK || a->B == 0) return st;
    return route_conv(a, (hipStream_t)stream, false);
}

// the family rnvp_conv2d(a) runs on, as the routing itself reports it (dry)
extern "C" int rnvp_conv2d_family(const rnvp_conv_args* a) {
    const int st = conv_args_status(a);
    if (st != RNVP_OK) return st;
    int fam = RNVP_FAMILY_OTHER;
    const int r = route_conv(a, nullptr, true, &fam);
    return r == RNVP_OK ? fam : r;
}

extern "C" int rnvp_conv2d_check(const rnvp_conv_args* a) {
    const int st = conv_args_status(a);
    if (st != RNVP_OK || a->B == 0) return st;
    return route_conv(a, nullptr, true);
}
