// One (dtype, configuration) of the deep-scale conv family per object: compiled
// once per pair with -DDEEP_T=float|bf16_t -DDEEP_CFG=0..6 (Makefile).
#include "conv_deep_launch.h"

template int rnvp_deep_cfg_launch<DEEP_T, DEEP_CFG>(const rnvp_conv_args*, hipStream_t, bool);
#if DEEP_CFG == 0 || DEEP_CFG == 1 || DEEP_CFG == 4 || DEEP_CFG == 5
template GroupKernel rnvp_deep_cfg_group<DEEP_T, DEEP_CFG>(int, bool);
#endif
