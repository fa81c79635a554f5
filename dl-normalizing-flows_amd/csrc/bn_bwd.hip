// BatchNorm backward apply as a launch of its own (the body, bn_bwd_body in
// conv_common.h, is shared with the kernels that fuse it).
#include "common.h"
#include "conv_common.h"

namespace {

// ---------------------------------------------------------------------------
// BN backward apply
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_bn_bwd(rnvp_bn_bwd_args a) {
    extern __shared__ double dsm[];
    bn_bwd_body<T>(a, dsm, blockIdx.x, gridDim.x);
}

}  // namespace

extern "C" int rnvp_bn_bwd_apply(const rnvp_bn_bwd_args* a, void* stream) {
    if (!a || !a->g || !a->x || !a->dx || !a->sums || a->M < 0 || a->C <= 0 || (a->cs & 7) || a->cs < a->C)
        return RNVP_E_INVALID;
    if (a->sum_shards < 1) return RNVP_E_INVALID;
    if (a->bn.tab && (!a->bn.sums || !al16(a->bn.tab))) return RNVP_E_INVALID;   // a finalized table: train mode
    if (a->dtype != RNVP_F32 && a->dtype != RNVP_BF16) return RNVP_E_INVALID;
    if (!al16(a->g) || !al16(a->x) || !al16(a->dx) || (a->residual && !al16(a->residual))) return RNVP_E_INVALID;
    if (a->M == 0) return RNVP_OK;
    hipStream_t s = (hipStream_t)stream;
    const int CH = a->dtype == RNVP_F32 ? 4 : 8;
    const long long nch = a->M * (a->cs / CH);
    size_t shm = 68 * (size_t)a->cs;   // 4*cs fp64 + 9*cs f32 (see k_bn_bwd)
    // every workgroup first reduces the fp64 statistic shards: 1024 groups
    // (4 per CU) amortise that best (sweep 512-4096, profiles/r2_small_kernel_sweeps.txt)
    if (a->dtype == RNVP_F32) k_bn_bwd<float><<<rnvp_grid(nch, 256, 1024), 256, shm, s>>>(*a);
    else k_bn_bwd<bf16_t><<<rnvp_grid(nch, 256, 1024), 256, shm, s>>>(*a);
    RNVP_LAUNCH_CHECK();
    return RNVP_OK;
}
