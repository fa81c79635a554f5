/*
 * realnvp_hip.h -- C ABI of the MI355X (gfx950) RealNVP coupling-layer engine.
 *
 * The reference (alisher-turubayev/dl-normalizing-flows) has no FFI: its hot
 * path is the Python nn.Module API of flow_realnvp.RealNVP and
 * modules_realnvp.{Checkerboard,Channelwise}AffineCoupling.  This header is
 * the boundary those modules bind to (via ctypes): plain
 * pointers, sizes and a hipStream_t passed as void*.  Every entry point
 *   - is stream-ordered: no host synchronisation, no allocation (HIP-graph
 *     capture safe);
 *   - returns 0 on success, a positive hipError_t from the launch, or a
 *     negative RNVP_E_* code for invalid arguments (nothing is launched then);
 *   - never takes ownership: the caller (PyTorch's caching allocator in the
 *     Python host) owns every buffer, including workspaces.
 *
 * Layouts: "flow" tensors (x, z, log|det J|) are NCHW fp32 exactly as in the
 * reference.  "net" tensors (the s/t ResNet activations) are NHWC with a
 * padded channel stride `cs` (multiple of 8), dtype RNVP_F32 (parity mode)
 * or RNVP_BF16 (perf mode, fp32 accumulation).  Reductions that feed batch
 * statistics accumulate fp64 sums: layout [2*C] = {sum x, sum x^2}.
 */
#ifndef REALNVP_HIP_H
#define REALNVP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { RNVP_F32 = 0, RNVP_BF16 = 1 };
enum { RNVP_OK = 0, RNVP_E_INVALID = -1, RNVP_E_UNSUPPORTED = -2 };

/* ---- version / capabilities ------------------------------------------- */
int rnvp_version(void);
/* sizeof the library's argument structs, in this order: rnvp_bn_src,
 * rnvp_bn_running, rnvp_conv_args, rnvp_wgrad_conv, rnvp_wgrad_group,
 * rnvp_bn_bwd_args, rnvp_wn_desc, rnvp_adam_args, rnvp_coupling_args,
 * rnvp_net_step, rnvp_range, rnvp_link_args, rnvp_step_ctl (-1 past the end).  A binding compares them with
 * its own mirrors at load time: a library built from another header revision
 * is refused instead of reading descriptor tables at the wrong stride.  (The
 * list is closed: later structs report their size next to their entry points,
 * see rnvp_wgrad_multi_struct_size.) */
int rnvp_struct_size(int which);
const char* rnvp_status_string(int status);
/* empty one-lane dispatch: delimits engine launches in PMC traces (profiling only) */
int rnvp_marker(int tag, void* stream);

/* ---- index maps (bit-exact permutations) --------------------------------
 * replace AbstractCoupling.build_mask   modules_realnvp.py:211-226
 *         RealNVP.squeeze/undo_squeeze  flow_realnvp.py:121-135
 *         RealNVP.factor_out/restore    flow_realnvp.py:167-193 (the 0/1
 *         order_matrix conv of 139-165 is the permutation implemented here)
 * Shapes are those of the *larger* tensor: squeeze/undo_squeeze take the
 * [B,C,H,W] un-squeezed shape; factor_out/restore the [B,C,H,W] full shape
 * (on/off are [B,2C,H/2,W/2]). */
int rnvp_checkerboard_mask(float* mask, int size, int config, void* stream);
int rnvp_squeeze(const float* x, float* y, int B, int C, int H, int W, void* stream);
int rnvp_undo_squeeze(const float* y, float* x, int B, int C, int H, int W, void* stream);
int rnvp_factor_out(const float* x, float* on, float* off, int B, int C, int H, int W, void* stream);
int rnvp_restore(const float* on, const float* off, float* x, int B, int C, int H, int W, void* stream);

/* ---- logit transform (utils.py:33-72) ----------------------------------
 * y = logit(((x*255+u)/256*2-1)*c+1)/2), logdet[b] = sum softplus(y)+softplus(-y)-softplus(-logit(c)).
 * u = noise[i] when noise != NULL, else a counter-based Philox4x32-10 uniform
 * in [0,1) keyed by (seed, offset + i), where offset is advanced by
 * (*epoch) * B * n_per_sample when epoch (a device int64, e.g. the optimizer
 * step) is non-NULL -- so a replayed HIP graph draws fresh noise every step.
 * n_per_sample = C*H*W. */
int rnvp_logit_fwd(const float* x, const float* noise, uint64_t seed, uint64_t offset, const long long* epoch,
                   float constraint, float* y, float* logdet, int B, int n_per_sample, void* stream);
int rnvp_logit_inv(const float* x, float* y, float constraint, long long n, void* stream);

/* ---- transforms.ToTensor of a uint8 batch (train.py:65-71) -------------
 * y[i] = x[i] / 255.f (correctly rounded), x and y 16-byte aligned.  Lets the
 * real-data pipeline ship 1 B/pixel over PCIe and convert on the device. */
int rnvp_u8_to_unit(const uint8_t* x, float* y, long long n, void* stream);

/* ---- NCHW fp32 <-> NHWC layout moves (standalone WeightNormConv2d) -----
 * modules_realnvp.py:64-71 called on its own: the operand moves into the
 * engine's NHWC layout (channel stride cs >= C, zero padded; dtype
 * RNVP_F32 / RNVP_BF16) and the result back. */
int rnvp_nchw_to_nhwc(const float* x, void* y, int B, int C, int H, int W, int cs, int dtype, void* stream);
int rnvp_nhwc_to_nchw(const void* x, float* y, int B, int C, int H, int W, int cs, int dtype, void* stream);

/* ---- prior log-prob and per-sample reduction (flow_realnvp.py:329-340) --
 * out[b] = ldj[b] + sum_i (-z_i^2/2 - log(2 pi)/2)       (N(0,1) prior)
 * bwd: gz_i = -z_i * gout[b] */
int rnvp_prior_logprob(const float* z, const float* ldj, float* out, int B, int n_per_sample, void* stream);
int rnvp_prior_logprob_bwd(const float* z, const float* gout, float* gz, int B, int n_per_sample, void* stream);

/* ---- batch-norm statistic sources --------------------------------------
 * Batch sums written by many workgroups are SHARDED to keep fp64 atomic
 * contention bounded: layout [shards][2][C]; a reader adds the shards.
 * rnvp_stat_shards(M) is the shard count the conv kernels use for an M-pixel
 * output (callers size their sum buffers with it). */
typedef struct rnvp_bn_src {
    const double* sums;   /* [shards][2*C] {sum, sum of squares} of the batch, or NULL */
    double count;         /* elements per channel behind sums */
    const float* mean;    /* running mean (used when sums == NULL) */
    const float* var;     /* running var */
    const float* gamma;   /* affine weight, NULL = 1 */
    const float* beta;    /* affine bias, NULL = 0 */
    float eps;
    int shards;           /* >= 1 */
    /* optional finalized table of this BatchNorm (train mode: sums != NULL),
     * written by the running-statistics update of the same forward pass
     * (rnvp_bn_running.tab) -- fp32 [C][4], one 16-byte entry per channel,
     * 16-byte aligned: {mean, rstd} with mean = sum * (1 / count) (what the
     * register tables of the deep-scale and halo kernels form), then {mean,
     * rstd} with mean = sum / count (every other kernel, the apply and the
     * fold); rstd = 1/sqrt(var + eps), var = sum2 / count - mean^2 with the
     * same flavour of division, clamped at 0.  Contract: every float is the
     * fp32 rounding of that float64 expression of the shard sums added in
     * shard order.  A reader loads the pair its own formula would give instead
     * of reducing the shards, and forms scale = gamma * rstd and shift = beta -
     * mean * gamma * rstd in fp32 exactly as it does after its own reduction:
     * the table holds no scale / shift (their fp32 formula is not the
     * rounding of a float64 value, and the backward's ReLU decisions must be
     * the forward's).  NULL: the table is derived from sums (eval mode,
     * forward prologues -- the table is not written yet -- and callers
     * without one). */
    const float* tab;
} rnvp_bn_src;
#define RNVP_BN_TAB_FLOATS(C) (4 * (C))
int rnvp_stat_shards(long long M);

/* running-stat update of nn.BatchNorm2d in train mode, for n BN sites at once.
 * rm = (1-mom) rm + mom mean; rv = (1-mom) rv + mom var*count/(count-1); nbt += 1 */
/* tab (optional): the site's finalized table (rnvp_bn_src.tab layout,
 * RNVP_BN_TAB_FLOATS(C) floats) is written by the same workgroup from the same
 * sums with eps -- once per forward instead of once per workgroup of every
 * backward consumer. */
typedef struct rnvp_bn_running {
    const double* sums; double count; int C; int shards;
    float* rmean; float* rvar; long long* nbt;
    float eps; float* tab;
} rnvp_bn_running;
int rnvp_bn_running_update(const rnvp_bn_running* descs_device, int n, int max_c, float momentum, void* stream);

/* ---- s/t ResNet convolution (MFMA implicit GEMM) -----------------------
 * replaces WeightNormConv2d.forward (modules_realnvp.py:64-71) inside
 * ResidualModule/ResidualBlock (73-194) with the surrounding
 * BatchNorm2d+ReLU fused into the operand load and bias / residual add /
 * skip accumulation / BN statistics fused into the epilogue.
 * y[m, n] (+)= sum_k act(x)[m + tap(k), ci(k)] * w[n, k] (+ bias[n]) (+ residual[m, n])
 * act = relu(bn(x)) when pro_bn_relu, identity otherwise; zero padding is
 * applied AFTER act (as nn.Conv2d pads its input).  k = (ky*ks+kx)*cs_in + ci.
 * epi_relu_bn_bwd (used for the data gradient): the result g is multiplied
 * by [relu(bn(epi_x)) > 0] before being stored, and epi_sums accumulates
 * {sum g, sum g*xhat} per output channel.  out_sums / epi_sums are sharded
 * with rnvp_stat_shards(B*H*W) shards and must be zeroed by the caller.
 * Small grids split K over workgroups when a workspace is given
 * (ws: fp32, >= splits * M * n elements; the epilogue then runs in a second
 * kernel that reduces the splits).
 * variant: 0 = automatic kernel choice per shape; 1 = the generic LDS-tiled
 * implicit GEMM (+ split-K) wherever the streaming kernel does not apply;
 * RNVP_VARIANT_DEEP = the deep-scale family (LDS activation tile + weight
 * ring) with its automatic configuration where it applies;
 * RNVP_VARIANT_DEEP0 + c = that family's configuration c, no fallback
 * (per call: used by the parity tests to cross-check the kernel families). */
#define RNVP_VARIANT_DEEP 2
#define RNVP_VARIANT_DEEP0 16
typedef struct rnvp_conv_args {
    int dtype;
    int B, H, W, ks;
    const void* x; int cs_in; int cin;
    const void* w; int kp;              /* packed weights [n][kp], kp % 64 == 0 */
    void* y; int cs_out; int n;
    const float* bias;
    const void* residual;
    int accumulate;
    int pro_bn_relu; rnvp_bn_src pro;
    double* out_sums;
    int epi_relu_bn_bwd; const void* epi_x; rnvp_bn_src epi; double* epi_sums;
    float* ws; long long ws_elems;      /* split-K workspace (optional) */
    int variant;
    /* optional (NULL: none): the same weights as w in the fragment-major image
     * -- block (n / 16, k / 32) of 512 bf16 at ((n / 16) * kp / 32 + k / 32) * 512,
     * element (n % 16 + 16 * (k % 32 / 8)) * 8 + k % 8 inside it (n padded to
     * 16 rows with zeros).  The bf16 3x3 deep-scale kernels read it instead of
     * w: each weight load of a wave is one contiguous KiB in MFMA lane order. */
    const void* w_frag;
    /* optional BatchNorm-backward prologue (bp = 1; bf16/fp32 data-gradient
     * convs on the deep-scale tiles, bf16 ones on the wide scales' streaming
     * 1x1 and band 3x3 kernels -- see rnvp_conv2d_check): x is the gradient g of
     * BatchNorm bp_bn's OUTPUT (the producing dgrad's relu/BN epilogue
     * output), bp_x that BatchNorm's saved input t (both [M][cs_in]), and the
     * conv's operand is dL/dt = gamma rstd (g - k1 - xhat k2) with
     * k1 = sum g / count, k2 = sum g xhat / count from bp_sums (the producing
     * epilogue's epi_sums, bp_shards shards <= 2) -- rnvp_bn_bwd_apply's
     * formula, formed while the operand tile is staged, so that apply's
     * launch and its dL/dt round trip disappear.  Workgroups of output
     * channel tile 0 store dL/dt to bp_out ([M][cs_in], for the weight
     * gradient); workgroup 0 writes bp_dbeta[c] = sum g and bp_dgamma[c] =
     * sum g xhat (BatchNorm2d's parameter gradients, modules_realnvp.py:36-52). */
    int bp; const void* bp_x; rnvp_bn_src bp_bn; const double* bp_sums; int bp_shards;
    void* bp_out; float* bp_dgamma; float* bp_dbeta;
} rnvp_conv_args;
int rnvp_conv2d(const rnvp_conv_args* a, void* stream);
/* RNVP_OK when rnvp_conv2d(a) would launch (argument checks and the
 * dispatch's own support limits, nothing launched): the host uses it to
 * decide which BatchNorm-backward applies fold into their consumer (bp). */
int rnvp_conv2d_check(const rnvp_conv_args* a);
/* host only, nothing launched: the kernel family rnvp_conv2d(a) would run on
 * (deep-scale tiles, the wide scales' streaming 1x1, their band 3x3, or one of
 * the remaining families), or a negative RNVP_E_* code.  The tests use it to
 * assert that a shape reaches the family it is meant to cover. */
enum { RNVP_FAMILY_OTHER = 0, RNVP_FAMILY_DEEP = 1, RNVP_FAMILY_S1 = 2, RNVP_FAMILY_BAND = 3 };
int rnvp_conv2d_family(const rnvp_conv_args* a);

/* grouped weight gradient: the wgrads of every conv of one coupling's s/t
 * network in ONE launch (they are independent of each other once the
 * coupling's data-gradient chain has run).  Conv c's pixel range is cut into
 * nz slabs; a workgroup owns one [64 n] x [64 k] tile of one slab and adds
 * its fp32 partial into replica z % nrep of ws[nrep][n][kp] (fp32 atomics,
 * <= nz/nrep adders per word; plain stores when nrep == nz); the bias partial
 * of k tile 0 goes to wsb[nrep][n] the same way.  ws / wsb must be zero on
 * entry; the weight-norm backward (rnvp_weight_norm_bwd, nz = nrep) sums the
 * replicas (and re-zeroes them when zero_after).  The library fills m_per_slab / task0 / tk.
 * Replaces the per-conv backward of WeightNormConv2d (modules_realnvp.py:53-59)
 * for the whole ResidualModule. */
#define RNVP_WGRAD_GROUP_MAX 24
typedef struct rnvp_wgrad_conv {
    const void* x; const void* dy;
    float* ws;                          /* [nrep][n][kp] fp32 partial sums */
    float* wsb;                         /* [nrep][n] bias partial sums or NULL */
    rnvp_bn_src pro;
    int cs_in, cin, ks, cs_dy, n, kp, pro_bn_relu, nz, nrep;
    long long m_per_slab;               /* filled by the library */
    int task0, tk, cls;                 /* filled by the library */
} rnvp_wgrad_conv;
typedef struct rnvp_wgrad_group {
    int dtype, B, H, W, n_conv;
    rnvp_wgrad_conv conv[RNVP_WGRAD_GROUP_MAX];
} rnvp_wgrad_group;
/* slab count the grouped wgrad uses for a conv over M pixels, and the
 * replica count (size ws with the latter) */
int rnvp_wgrad_slabs(long long M);
int rnvp_wgrad_replicas(int nz);
int rnvp_conv2d_wgrad_grouped(const rnvp_wgrad_group* g, void* stream);
/* host only, nothing launched: the tap-shared bf16 kernel class conv c of the
 * group runs in (0: 3x3 wide tiles, 1: 1x1 128 x 128, 2: 3x3 up to 32
 * channels, 3: 1x1 up to 64), RNVP_E_UNSUPPORTED when the group takes the
 * generic kernel */
int rnvp_wgrad_class(const rnvp_wgrad_group* g, int c);

/* model-wide weight gradient: the tap-shared bf16 tiles of MANY groups (the
 * deep couplings, whose own launches are each short of work) in one launch per
 * tile class, driven by device-resident tables instead of the by-value group.
 * A table entry is a conv with its own shape and class; the block -> task map
 * is planned on the host once (rnvp_wgrad_multi_plan) and uploaded:
 *   xcd_start[9]      task-list offsets per XCD (block b serves XCD b % 8 and
 *                     takes entry b / 8 of that XCD's list; surplus blocks exit)
 *   tasks[n_task][2]  {conv index, local tile id = (slab * co tiles + co tile)
 *                     * ci tiles + ci tile}
 * The (conv, slab) runs are split over the XCDs by summed cost (stages +
 * a per-workgroup overhead per tile), longest first onto the least loaded
 * XCD; a run's tiles stay adjacent on one XCD (they share the slab's pixels
 * through L2) and every XCD's list is ordered by descending tile cost.
 * Only plain-store convs (nrep == nz) are admitted: every float of ws / wsb
 * is then what the group's own rnvp_conv2d_wgrad_grouped launch writes. */
typedef struct rnvp_wgrad_multi_conv {
    const void* x; const void* dy; float* ws; float* wsb;
    rnvp_bn_src pro;
    int cs_in, cin, cs_dy, n, kp, pro_bn_relu, nz, nrep;
    int B, H, W, cls;
    int tco, tci;                       /* co / ci tiles of the class */
    long long m_per_slab;
} rnvp_wgrad_multi_conv;
typedef struct rnvp_wgrad_multi {
    int cls, ko, n_conv, n_task, grid, lds_bytes;   /* filled by the planner */
    long long xcd_cost[8];                          /* filled by the planner */
    /* device copies of the planner's arrays, set by the caller after upload */
    const rnvp_wgrad_multi_conv* convs;
    const int* xcd_start;
    const int* tasks;
} rnvp_wgrad_multi;
/* host only, nothing launched: the plan of class cls (0 .. 3) over the groups'
 * convs of that class.  convs (conv_cap entries), xcd_start (9 ints) and tasks
 * (2 * task_cap ints) receive the arrays to upload; with convs == NULL only
 * the counts (m->n_conv, m->n_task) are filled.  m->n_conv == 0: the class is
 * absent, nothing to launch.  RNVP_E_UNSUPPORTED: a group is not bf16, is
 * declined by the tap-shared kernel, holds a conv with nrep < nz, or would
 * run in another k order than its own launch (the caller keeps that group's
 * own launch); RNVP_E_INVALID: bad arguments or capacities. */
int rnvp_wgrad_multi_plan(const rnvp_wgrad_group* groups, int n_groups, int cls, rnvp_wgrad_multi_conv* convs,
                          int conv_cap, int* xcd_start, int* tasks, int task_cap, rnvp_wgrad_multi* m);
int rnvp_conv2d_wgrad_multi(const rnvp_wgrad_multi* m, void* stream);
/* sizeof rnvp_wgrad_multi_conv (0) and rnvp_wgrad_multi (1), -1 otherwise: a
 * binding compares them with its mirrors at load, as with rnvp_struct_size */
int rnvp_wgrad_multi_struct_size(int which);

/* batch-norm backward apply (train mode), the second half of BN backward:
 * dx = gamma*rstd*(g - sum_g/M - xhat * sum_gxhat/M) (+ residual) (+= dx if accumulate)
 * also writes dgamma = sum_gxhat, dbeta = sum_g (when non-NULL) */
typedef struct rnvp_bn_bwd_args {
    int dtype; long long M; int C; int cs;
    const void* g; const void* x; rnvp_bn_src bn;
    const double* sums; int sum_shards;  /* the dgrad epilogue's epi_sums */
    void* dx; const void* residual; int accumulate;
    float* dgamma; float* dbeta;
} rnvp_bn_bwd_args;
int rnvp_bn_bwd_apply(const rnvp_bn_bwd_args* a, void* stream);

/* weight normalisation (torch.nn.utils.weight_norm dim=0, modules_realnvp.py:53-59)
 * w = g * v / ||v||, packed into the forward layout wf[co][(ky*ks+kx)*cs_in+ci]
 * and the flipped, transposed data-gradient layout wd[ci][(ky'*ks+kx')*cs_out+co]
 * (w[co][ci][ks-1-ky'][ks-1-kx']).  g == NULL means a plain conv (w = v).
 * bwd: dv = (g/|v|)(dw - (v.dw/|v|^2) v), dg = v.dw/|v| from the packed dw
 * (sum of nz slabs), written at grad_base + dv_off / dg_off (elements;
 * dg_off < 0 = frozen g); dbias = sum of the nz bias partials at db_off;
 * zero_after: leave the slabs zero for the next atomic accumulation. */
typedef struct rnvp_wn_desc {
    const float* v; const float* g;
    void* wf; void* wd; float* norm;
    float* dw;                         /* packed [nz][cout][kp_f] fp32 (bwd), summed over nz */
    long long dv_off; long long dg_off;
    int cout, cin, ks, cs_in, kp_f, cs_out, kp_d;
    int row0;                          /* first global row (prefix sum of cout) */
    int tile0;                         /* first pack tile (prefix sum of rnvp_weight_norm_tiles) */
    int nz;                            /* dw partial slabs (>= 1) */
    float* dbp;                        /* bias partials [nz][cout] or NULL */
    long long db_off;                  /* bias gradient offset (elements) */
    int zero_after;                    /* re-zero dw / dbp after use (atomic accumulation) */
    int blk0;                          /* first row block (prefix sum of rnvp_weight_norm_opt_blocks) */
    /* optional fragment-major copies of wf / wd (rnvp_conv_args.w_frag; 3x3,
     * cs_in resp. cs_out a multiple of 32, rows padded to 16), written beside
     * the row-major images by rnvp_weight_norm_fwd / _transpose, or NULL */
    void* wf_frag; void* wd_frag;
} rnvp_wn_desc;
/* fwd, for any number of convs (a whole model): one launch computes every
 * row norm, one writes both packed images on [32 co] x [32 ci] tiles
 * ([32 co] x [256 ci] for 1x1 convs; total_tiles = sum over the convs of
 * rnvp_weight_norm_tiles(cout, cin, ks), < 0 for an invalid shape).
 * The images' padding must be zero on entry (it is never written). */
int rnvp_weight_norm_tiles(int cout, int cin, int ks);
int rnvp_weight_norm_fwd(const rnvp_wn_desc* descs_device, int n_desc, int total_rows, int total_tiles, int dtype,
                         void* stream);
/* zero0 / zero1: byte ranges (8-byte multiples, 8-byte aligned, may be
 * NULL / 0) zeroed by the same launch -- the caller's batch-statistic sums,
 * left zero for the next step once the coupling's backward has consumed them */
int rnvp_weight_norm_bwd(const rnvp_wn_desc* descs_device, int n_desc, int total_rows, float* grad_base,
                         void* zero0, long long zero0_bytes, void* zero1, long long zero1_bytes, void* stream);

/* Row-local parameter pass (weight-norm backward + Adam + next weight norm).
 * One launch per coupling replaces rnvp_weight_norm_bwd + that coupling's
 * share of rnvp_adam_step + the next step's rnvp_weight_norm_fwd: for every
 * output row co of every conv in the table, with dv_off / dg_off / db_off
 * indexing the adam arenas (param, grad, exp_avg, exp_avg_sq, mask):
 *   from_slabs = 1: dW = sum of the nz slabs, dv / dg / dbias as
 *     rnvp_weight_norm_bwd (also stored into grad); from_slabs = 0: dv / dg /
 *     dbias read from grad (data parallel, after the all-reduce);
 *   Adam (rnvp_adam_update semantics, t = *step + step_add) on the row of v
 *     (mask 1 assumed: the caller checks), g[co] (when dg_off >= 0) and the
 *     bias (db_off >= 0; db_off < 0 = no bias), with their mask bytes;
 *   norm[co] = ||v'||, and the forward packed image (rnvp_weight_norm_fwd
 *     layout) of w' = g' v' / ||v'|| for the next step; the data-gradient
 *     image then follows from rnvp_weight_norm_transpose.
 * blk0: prefix sums of rnvp_weight_norm_opt_blocks(cout, cin, ks) (negative:
 * the row does not fit the kernel's LDS -- use the unfused calls); the block
 * count assumes the packed row layout cs_in == round_up(cin, 8), which every
 * descriptor of this call must have (the binding checks its tables).
 * zero0 / zero1 as rnvp_weight_norm_bwd.  Replaces modules_realnvp.py:53-59
 * (weight_norm) and train.py:134, 200 (Adam) for the s/t convs. */
/* Device-resident step control (learning-rate schedule, gradient-norm
 * clipping, non-finite skip; see "step control" below).  The host writes the
 * configuration with stream-ordered copies -- it is never a captured launch
 * argument, so a replayed HIP graph follows every change -- and
 * rnvp_step_control writes the decisions the Adam kernels read. */
enum { RNVP_DECAY_NONE = 0, RNVP_DECAY_EXP = 1, RNVP_DECAY_COSINE = 2 };
typedef struct rnvp_step_ctl {
    /* configuration, written by the host */
    float base_lr; float warmup_start; long long warmup_steps;
    int decay; double decay_rate; long long decay_steps;   /* fp64: r^u carries the rate's rounding u times */
    float max_norm;                       /* <= 0: no clipping */
    /* written by rnvp_step_control every step */
    float lr, grad_scale, grad_norm; int skip;
    long long n_clipped, n_skipped;
    /* gradient accumulation ("step control" below); a block with accum_steps
     * <= 1 (a zero-filled one included) behaves as one without these fields */
    int accum_steps;                      /* configuration: micro-steps per optimizer step */
    int micro;                            /* device: micro-steps already accumulated in the open optimizer step */
    int hold;                             /* device: set on a held micro-step */
} rnvp_step_ctl;
/* ctl (optional, device): NULL = lr below, gradients as they are.  Non-NULL:
 * the Adam kernels (rnvp_weight_norm_bwd_adam, rnvp_adam_gather,
 * rnvp_adam_range) take the learning rate from ctl->lr instead of lr,
 * multiply the incoming gradient (regulariser included, weight decay not) by
 * ctl->grad_scale -- a scale of exactly 1.0f leaves every bit of the update as
 * without ctl -- and touch no memory at all when ctl->skip is set (except
 * rnvp_weight_norm_bwd_adam's zero0 / zero1 ranges, which are still zeroed;
 * a skipped from_slabs = 1 pass leaves its slabs unconsumed: a caller that
 * can skip runs rnvp_weight_norm_bwd first and passes from_slabs = 0). */
typedef struct rnvp_adam_args {
    float* param; float* grad; float* exp_avg; float* exp_avg_sq; const uint8_t* mask;
    const long long* step; long long step_add;
    float lr, beta1, beta2, eps, weight_decay, reg_coef;
    const rnvp_step_ctl* ctl;
} rnvp_adam_args;
int rnvp_weight_norm_opt_blocks(int cout, int cin, int ks);
int rnvp_weight_norm_bwd_adam(const rnvp_wn_desc* descs_device, int n_desc, int total_blocks, int from_slabs,
                              int dtype, const rnvp_adam_args* adam, void* zero0, long long zero0_bytes,
                              void* zero1, long long zero1_bytes, void* stream);
/* wd from wf (the transposed, flipped data-gradient image from the forward
 * image; bitwise what rnvp_weight_norm_fwd writes for the same weights), on
 * rnvp_weight_norm_fwd's tiles (tile0 / total_tiles) */
int rnvp_weight_norm_transpose(const rnvp_wn_desc* descs_device, int n_desc, int total_tiles, int dtype,
                               void* stream);
/* zero n byte ranges (8-byte multiples and alignment; max_bytes >= every
 * range's size): the batch-statistic sums a deferred parameter pass leaves
 * zero for the next step */
typedef struct rnvp_range { void* p; long long bytes; } rnvp_range;
int rnvp_zero_ranges(const rnvp_range* ranges_device, int n, long long max_bytes, void* stream);
/* Adam on the arena elements idx[0..n) (the parameters outside the convs:
 * BatchNorm affines, coupling scales, ...), rnvp_adam_update semantics */
int rnvp_adam_gather(const rnvp_adam_args* adam, const long long* idx, long long n, void* stream);

/* ---- affine coupling (modules_realnvp.py:239-370) -----------------------
 * kind 0 = CheckerboardAffineCoupling, 1 = ChannelwiseAffineCoupling.
 * Cb = channels seen by in_bn/out_bn: C (ckbd) or C/2 (chan).
 * Net input h0 = relu(cat(bn_in(xm), -bn_in(xm)[, mask])) with xm = x*mask
 * (ckbd, 2C+1 channels) or the "off" half (chan, C channels).  Net output
 * st = [shift | log_rescale] (2*Cb channels). */
/* the coupling's per-channel fp64 reductions are spread over this many
 * shards (workgroup % shards) so no word takes more than ~32 atomic adders */
#ifndef RNVP_COUPLING_SHARDS
#define RNVP_COUPLING_SHARDS 16
#endif
typedef struct rnvp_coupling_args {
    int kind, B, C, H, W, mask_config, coupling_bn, training, dtype;
    float momentum, eps;
    const float* x;                       /* coupling input (reverse: the output) */
    const float* in_gamma; const float* in_beta;
    float* in_rmean; float* in_rvar; long long* in_nbt;
    double* in_sums;                      /* [RNVP_COUPLING_SHARDS][2*Cb] */
    void* h0; int cs_h0;
    const void* st; int cs_st;
    const float* scale; const float* scale_shift;
    float* u;                             /* pre-out_bn value, [B,C,H,W] */
    float* z;                             /* output [B,C,H,W] */
    double* out_sums;                     /* [RNVP_COUPLING_SHARDS][2*Cb] */
    float* out_rmean; float* out_rvar; long long* out_nbt;
    float* ldj_sample;                    /* [B], += */
    float* ldj_full;                      /* [B,C,H,W] or NULL, written */
    /* backward */
    const float* gz;                      /* [B,C,H,W] */
    const float* gl_full;                 /* [B,C,H,W] or NULL */
    const float* gl_sample;               /* [B] used when gl_full == NULL */
    float* gx;                            /* [B,C,H,W] */
    void* gst; int cs_gst;
    double* bwd_sums;                     /* [RNVP_COUPLING_SHARDS][3*Cb] */
    float* g_scale; float* g_scale_shift; /* += */
    const void* gh0; int cs_gh0;
    double* in_bwd_sums;                  /* [RNVP_COUPLING_SHARDS][2*Cb] */
    float* g_in_gamma; float* g_in_beta;  /* written */
    /* optional, forward (rnvp_coupling_out_fwd): running-stat updates of the
     * s/t net's BatchNorms (what rnvp_bn_running_update does), folded into
     * the out launch; net_running is a device table of n_net_running sites
     * with at most net_running_cmax channels */
    const rnvp_bn_running* net_running; int n_net_running; int net_running_cmax;
    /* optional: [RNVP_COUPLING_SHARDS][2] fp64 partials of the scale /
     * scale_shift gradients -- zero on entry to rnvp_coupling_out_bwd, which
     * adds into them (one shard per group of workgroups instead of every
     * workgroup on one address); rnvp_coupling_in_bwd folds them into
     * g_scale / g_scale_shift (+=) and leaves them zero */
    double* gscale_part;
    /* optional, coupling links (rnvp_coupling_out_u, rnvp_coupling_link_fwd /
     * _bwd; see "coupling links" below).  All [RNVP_COUPLING_SHARDS][...] fp64,
     * zeroed on entry to the step that accumulates them:
     *   cls_sums   [nclass][2][C]  sums of u and u^2 per (pixel class, channel),
     *              every channel; pixel classes by nclass: 1 = one class,
     *              2 = (i+j)&1, 4 = (i&1)*2+(j&1) at pixel (i, j)
     *   prior_sums [nclass][2][C]  sums of -z*g_lp[b] and -z^2*g_lp[b] over the
     *              elements the link hands to the prior (factored out / final)
     *   outp_sums  [2][2][C]       sums of gx and gx*x per ((i+j)&1, channel) of
     *              this coupling's direct input gradient (written by its out
     *              part's link backward, read by the previous link's)
     *   in_bwd_ext [2][Cb]         sums of dL/dxa and dL/dxa * xm over the
     *              positions in_bn normalises (the kept squares / the
     *              conditioning half)
     * and two fp32 tables the forward leaves for the backward (written by the
     * link launch that computes them, or rnvp_coupling_in_apply):
     *   out_tab    [2][Cb]         out_bn batch mean, 1/sqrt(var + eps)
     *   in_tab     [4][Cb]         in_bn scale, shift, mean, 1/sqrt(var + eps) */
    int nclass;
    double* cls_sums;
    double* prior_sums;
    double* outp_sums;
    double* in_bwd_ext;
    float* out_tab;
    float* in_tab;
} rnvp_coupling_args;
int rnvp_coupling_in_fwd(const rnvp_coupling_args* a, void* stream);   /* in_sums must be zeroed */
int rnvp_coupling_out_fwd(const rnvp_coupling_args* a, void* stream);  /* out_sums must be zeroed */
int rnvp_coupling_reverse(const rnvp_coupling_args* a, void* stream);  /* z = inverse(x) */
/* backward of rnvp_coupling_reverse (training or eval; the out_bn inverse uses
 * the running statistics, modules_realnvp.py:284-291): from gz = dL/dz and
 * gl_full = dL/dlog_diag_J (or NULL) writes gx's direct part, the net output
 * gradient gst and the scale / scale_shift partials into gscale_part (which
 * rnvp_coupling_in_bwd folds into g_scale / g_scale_shift); the net backward
 * and rnvp_coupling_in_bwd then run as after rnvp_coupling_out_bwd. */
int rnvp_coupling_reverse_bwd(const rnvp_coupling_args* a, void* stream);
int rnvp_coupling_out_bwd(const rnvp_coupling_args* a, void* stream);  /* bwd_sums zeroed; writes gx, gst */
int rnvp_coupling_in_bwd(const rnvp_coupling_args* a, void* stream);   /* in_bwd_sums zeroed; gx += */

/* ---- coupling links (the training step's flow program) ----------------------
 * A link joins coupling a to what consumes its output z (flow_realnvp.py:252-327):
 *   RNVP_LINK_SAME      coupling n with n->x = z (same kind and shape, the
 *                       opposite mask: checkerboard_combo / channelwise_combo,
 *                       flow_realnvp.py:98-116)
 *   RNVP_LINK_SQUEEZE   checkerboard a -> channelwise n, n->x = squeeze(z)
 *                       (flow_realnvp.py:260; squeeze 121-127)
 *   RNVP_LINK_UNFACTOR  channelwise a -> the next scale's checkerboard n,
 *                       (n->x, off) = factor_out(undo_squeeze(z)) (264-267, 167-177):
 *                       n->x channel c = z channel 4c (c < K) / 4(c-K)+3, off
 *                       channel c = z channel 4c+1 / 4(c-K)+2 (K = n->C/2); the
 *                       off half goes to the prior
 *   RNVP_LINK_FINAL     z is the last scale's output: all of it goes to the
 *                       prior (312-327, 336-338)
 * The squeeze / factor-out permutations live in the link's addressing: no
 * permuted copy is made.  The prior log N(0,1) of what the link hands to the
 * prior is added into prior[b] (fp64, flow_realnvp.py:336-338).
 *
 * Forward, per coupling a: rnvp_coupling_out_u(a) (after a's s/t net: the
 * per-class sums of u and the per-sample sum of log_rescale) then
 * rnvp_coupling_link_fwd(a, n, l): z = out_bn(u) (u recomputed from x and the
 * net output), a's log-det constant and running statistics, n->x, n's in_bn
 * statistics in closed form from a's class sums (n->in_sums shard 0; n's in_bn
 * reads positions that are each wholly transformed or wholly kept by a), n's
 * net input h0 and in_bn running statistics.  a->nclass must be
 * rnvp_link_nclass(type, a->kind).
 *
 * Backward, per coupling a (n's backward done first): rnvp_coupling_link_bwd(a,
 * n, l) forms dL/dz of a (n's direct input gradient n->gx + n's in_bn backward
 * from n->gh0, or the prior's -z*g_lp) and runs a's out part with it (a->gx,
 * a->gst, a's scale partials, a->outp_sums) -- the out_bn backward sums it needs
 * are closed forms of n->outp_sums, n->in_bwd_sums, n->in_bwd_ext, n->in_sums and
 * a's class / prior sums; block 0 writes n's in_bn affine gradients.  Then a's
 * net backward and rnvp_coupling_in_bwd(a) with a->in_bwd_ext set (only the
 * reduction pass runs when a->gx is NULL: the first coupling keeps the apply
 * pass for dL/dx).  Requires training, coupling_bn, per-sample log-det. */
enum { RNVP_LINK_SAME = 0, RNVP_LINK_SQUEEZE = 1, RNVP_LINK_UNFACTOR = 2, RNVP_LINK_FINAL = 3 };
typedef struct rnvp_link_args {
    int type;
    const float* g_lp;       /* [B] dL/dlog_prob[b] (the prior's and every log-det's gradient weight) */
    double* prior;           /* [B] += (UNFACTOR, FINAL) */
    float* off;              /* UNFACTOR: [B, n->C, H, W] factored-out half, or NULL (not stored) */
    float* z;                /* FINAL: a's output [B, C, H, W], or NULL (not stored) */
} rnvp_link_args;
int rnvp_link_nclass(int type, int kind);
int rnvp_coupling_out_u(const rnvp_coupling_args* a, void* stream);
int rnvp_coupling_link_fwd(const rnvp_coupling_args* a, const rnvp_coupling_args* n, const rnvp_link_args* l,
                           void* stream);
int rnvp_coupling_link_bwd(const rnvp_coupling_args* a, const rnvp_coupling_args* n, const rnvp_link_args* l,
                           void* stream);
/* only the in part's apply pass (rnvp_coupling_in_fwd without its statistics
 * pass: a->in_sums already hold the batch sums, e.g. from rnvp_flow_in_fwd) */
int rnvp_coupling_in_apply(const rnvp_coupling_args* a, void* stream);
/* the step's input: logit_transform of raw pixels with device Philox noise
 * (rnvp_logit_fwd semantics, logdet[b] += instead of =) fused with the first
 * coupling's in_bn batch sums (first->in_sums +=, NULL = none; first->x must
 * be y).  Spread over every CU (pixel tiles, not one workgroup per sample). */
int rnvp_flow_in_fwd(const float* x, uint64_t seed, const long long* epoch, float constraint, float* y,
                     float* logdet, const rnvp_coupling_args* first, int B, int C, int H, int W, void* stream);
/* end of the forward: lp[b] = prior[b] + ldj[b]; ll_acc[0] += mean_b(lp[b] +
 * logdet[b]) (fp64); prior and ldj are left zero for the next step, and
 * logdet too when zero_logdet */
int rnvp_flow_lp_finish(double* prior, float* ldj, float* logdet, int zero_logdet, float* lp, double* ll_acc, int B,
                        void* stream);

/* ---- regulariser and optimizer ------------------------------------------
 * weight_scale = sum over tensors of sum p^2  (flow_realnvp.py:362-369);
 * out must be zeroed.  bwd: grad_i += 2 * gout * p_i. */
typedef struct rnvp_tensor_ref { float* p; float* g; long long n; } rnvp_tensor_ref;
int rnvp_sumsq_multi(const rnvp_tensor_ref* refs_device, int n_refs, float* out, void* stream);
int rnvp_sumsq_bwd_multi(const rnvp_tensor_ref* refs_device, int n_refs, const float* gout, float coef, void* stream);

/* torch.optim.Adam step (coupled L2 weight decay, train.py:134) over a flat
 * fp32 parameter arena (n % 4 == 0, 16-B aligned).  step is a device int64
 * incremented by this call.  mask (optional, uint8 per element): 0 = frozen
 * (requires_grad=False: parameter and moments untouched, as torch skips
 * params without grad), 1 = trainable, 2 = trainable and regularised, i.e.
 * reg_coef*2*p is added to its gradient (the 5e-5*weight_scale term of
 * train.py:194 for trainable weight_g / scale).  NULL = all trainable. */
int rnvp_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                   long long* step, float lr, float beta1, float beta2, float eps, float weight_decay,
                   const uint8_t* mask, float reg_coef, void* stream);

/* the same update over one range [param, param+n) of the arena WITHOUT
 * touching the step counter: bias corrections use t = *step + step_add.  Lets
 * the optimizer run per parameter group as soon as that group's gradient is
 * final (e.g. per coupling, overlapped with the rest of the backward); the
 * caller advances the counter once per step with rnvp_step_increment. */
int rnvp_adam_update(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                     const long long* step, long long step_add, float lr, float beta1, float beta2, float eps,
                     float weight_decay, const uint8_t* mask, float reg_coef, void* stream);
int rnvp_step_increment(long long* step, void* stream);

/* ---- step control --------------------------------------------------------
 * Decisions taken on the device between the backward and the parameter pass,
 * so that a captured step needs no re-capture for a learning-rate schedule
 * and can bound or refuse its own update.  u = *step is the number of
 * optimizer steps already taken; everything below is evaluated in fp64 and
 * rounded once to fp32.
 *   lr = base_lr * warm(u) * decay(u)
 *   warm(u)  = s + (1 - s) min(u, W) / W  (s = warmup_start, W = warmup_steps;
 *              1 when W == 0): torch's LinearLR(start_factor = s, total_iters = W)
 *   decay(u) = 1 (RNVP_DECAY_NONE) | r^u (RNVP_DECAY_EXP, r = decay_rate:
 *              ExponentialLR) | f + (1 - f)(1 + cos(pi min(u, T) / T)) / 2
 *              (RNVP_DECAY_COSINE, f = decay_rate, T = decay_steps: the closed
 *              form of CosineAnnealingLR with eta_min = f base_lr, held after T)
 *   grad_norm  = sqrt(sum of the partials): the L2 norm of what p.grad holds
 *              after loss.backward() in the reference loop (train.py:192-198),
 *              i.e. with the 5e-5 * weight_scale regulariser's gradient on
 *              mask-2 elements, without Adam's weight decay, frozen elements
 *              (mask 0) and padding excluded
 *   grad_scale = min(1, max_norm / (grad_norm + 1e-6)), exactly 1.0f when the
 *              clip does not bind or max_norm <= 0 (torch.nn.utils.clip_grad_norm_)
 *   skip = 1 and n_skipped += 1 when the sum of squares is not finite;
 *              n_clipped += 1 when grad_scale < 1.
 *
 * rnvp_grad_sumsq_parts(n): the number of partials rnvp_grad_sumsq writes for
 * an n-element arena (1 .. 2048).
 * rnvp_grad_sumsq: partials[b] = sum over workgroup b's share of the elements
 * with mask_i > 0 of (g_i + [mask_i == 2] 2 reg_coef p_i)^2 in fp64 (a NULL
 * mask = all 1).  Reads ad->grad, ad->param, ad->mask, ad->reg_coef; n % 4 ==
 * 0, grad / param 16-byte and mask 4-byte aligned; n_parts must equal
 * rnvp_grad_sumsq_parts(n).  One plain store per workgroup, no atomics: the
 * result is bitwise reproducible.
 * rnvp_step_control (one workgroup): partials == NULL (n_parts ignored) sets
 * lr, grad_scale = 1 and skip = 0 -- it opens a step; otherwise it also adds
 * the partials in a fixed order and sets grad_norm, grad_scale, skip and the
 * counters.  n_parts <= 2048.
 * rnvp_adam_range: rnvp_adam_update over [ad->param, ad->param + n) with the
 * arguments of ad, honouring ad->ctl.
 * rnvp_step_advance: rnvp_step_increment unless ctl->skip.
 *
 * Gradient accumulation (ctl->accum_steps = K > 1): K launches of the same
 * step make one optimizer step, and the device decides which of them applies.
 * rnvp_grad_accumulate takes rnvp_grad_sumsq's place: one pass over the arena
 * (rnvp_grad_sumsq's grid, granules and alignment rules; acc is an n-element
 * fp32 accumulator, 16-byte aligned, zero before the first micro-step) that
 *   while ctl->micro < K - 1 (a held micro-step) stores acc += grad and
 *     writes neither grad nor the partials;
 *   otherwise (the final micro-step) stores grad = (acc + grad) / (float)K
 *     -- a correctly rounded fp32 division -- and acc = 0, and writes the
 *     partials of the new grad, bitwise what rnvp_grad_sumsq writes for it.
 * rnvp_step_control with partials then, while micro < K - 1, sets skip = 1 and
 * hold = 1 and micro += 1 without reading the partials or touching grad_norm
 * and the counters -- the Adam kernels and rnvp_step_advance leave everything
 * as it is, as for any skipped step; otherwise it sets micro = 0, hold = 0 and
 * decides as above from the accumulated gradient's partials (a non-finite
 * value from any micro-step skips the whole optimizer step, counted once).
 * The opening call (partials == NULL) leaves micro and hold alone. */
int rnvp_grad_sumsq_parts(long long n);
int rnvp_grad_sumsq(const rnvp_adam_args* ad, long long n, double* partials, int n_parts, void* stream);
int rnvp_grad_accumulate(const rnvp_adam_args* ad, float* acc, long long n, const rnvp_step_ctl* ctl,
                         double* partials, int n_parts, void* stream);
int rnvp_step_control(rnvp_step_ctl* ctl, const long long* step, const double* partials, int n_parts, void* stream);
int rnvp_adam_range(const rnvp_adam_args* ad, long long n, void* stream);
int rnvp_step_advance(long long* step, const rnvp_step_ctl* ctl, void* stream);

/* ---- weight averaging ------------------------------------------------------
 * The exponential moving average (Polyak average) of the parameter arena, kept
 * by the training step: one launch of its own after the step's last Adam
 * launch, with a device-resident control block of its own (rnvp_adam_args,
 * rnvp_step_ctl and the Adam kernels know nothing of it).
 *
 * rnvp_ema_update, one pass over the arena (12 B / element):
 *   u = *step + step_add   the optimizer steps taken, this one included
 *                          (step_add = 1 before the counter has moved, 0 after)
 *   d = warmup ? fminf(decay, (1 + u) / (10 + u)) : decay       in fp32
 *   e' = e + (1 - d) * (p - e)
 * as three separately rounded IEEE fp32 operations (a subtraction, a
 * multiplication by the fp32 value 1 - d, an addition; never an fma), so an
 * element with p == e keeps its value (and, but for a negative zero, its
 * bits): frozen parameters and the arena's padding need no mask.  d == 0
 * (a decay of 0: no averaging) stores p itself.  With ctl !=
 * NULL and ctl->skip set (a skipped step, or a held micro-step of an
 * accumulating block) the kernel returns before it loads an element and
 * writes nothing, ectl included.  Otherwise one thread stores applied = d and
 * n_updates + 1 with plain stores; no other thread reads a field the kernel
 * writes.  With warm-up off this is torch.optim.swa_utils.
 * get_ema_multi_avg_fn(decay): ema.lerp_(p, 1 - decay).
 * The host writes decay / warmup with stream-ordered copies (0 <= decay < 1 is
 * the writer's responsibility: the library does not read the block on the
 * host).
 *
 * rnvp_ema_swap exchanges two arenas in place (16 B / element): evaluation
 * reads the average through the parameters' own storage, with no temporary.
 *
 * Both are stream-ordered and capture-safe, use no LDS and no atomics, and
 * check their arguments before any HIP call: RNVP_E_INVALID for a NULL ema /
 * param / ectl / step (a / b), n < 0 or n % 4 != 0, arenas that are not
 * 16-byte aligned (ectl, step and ctl: 8-byte), or arenas that overlap
 * (a == b included).  n == 0 is RNVP_OK with nothing launched. */
typedef struct rnvp_ema_ctl {
    float decay;            /* configuration, host-written */
    int warmup;
    float applied;          /* device: the decay the last applied update used */
    int pad;
    long long n_updates;    /* device: updates applied so far */
} rnvp_ema_ctl;
/* sizeof(rnvp_ema_ctl), for a binding's mirror (the list of rnvp_struct_size is closed) */
int rnvp_ema_struct_size(void);
int rnvp_ema_update(float* ema, const float* param, long long n, rnvp_ema_ctl* ectl, const long long* step,
                    long long step_add, const rnvp_step_ctl* ctl /* may be NULL */, void* stream);
int rnvp_ema_swap(float* a, float* b, long long n, void* stream);

/* ---- scoring ---------------------------------------------------------------
 * Per-image log-likelihoods of a dataset (nats; the validation loop of
 * train.py:214-233 without its mean): batches of up to B images, the last one
 * ragged, and the K-draw importance bound log(1/K sum_k p(x + u_k)) over K
 * draws of the uniform dequantisation noise.  One draw of one batch is
 *   rnvp_score_in_fwd -> the eval-mode flow forward (per-sample ldj) -> rnvp_score_finish
 * and a device-resident control block carries everything that changes from one
 * replay to the next, so one captured graph serves a whole pass: the host
 * writes its fields with stream-ordered copies / fills, rnvp_score_finish
 * advances it, and the library never reads it on the host.
 *
 * rnvp_score_in_fwd is rnvp_logit_fwd's transform (logdet[b] += as
 * rnvp_flow_in_fwd: the caller zeroes logdet once, rnvp_score_finish leaves it
 * zero) over chunks of every sample, with noise that belongs to the IMAGE, not
 * to its slot in the batch: with n = C*H*W, element e of row b in draw
 * k = ctl->draw takes the Philox uniform of counter
 *   ((ctl->first + b) * n_draws + k) * n + e
 * so an image's score does not depend on the batch size or on its neighbours.
 * A non-NULL noise ([B][n]) replaces the Philox values of this draw.  Reads
 * ctl, never writes it.  Rows >= n_valid are transformed like any other (their
 * pixels are the caller's; zeros keep every value finite).  A sample is cut
 * into at most 8 chunks, one fp32 atomic each: logdet[b] stays within 10
 * roundings (6e-7 relative; its terms are all positive) of the exact sum.
 *
 * rnvp_score_finish, a row kernel and then a one-workgroup advance:
 *   ll[b] = sum_i (-z_i^2/2 - log(2 pi)/2) + ldj[b] + logdet[b]   in fp64,
 *   stored to lp[b] when lp != NULL (b < n_valid); ldj[b] = logdet[b] = 0
 *   afterwards.
 *   run ([B][2] fp32: running max m, sum s of exp(ll - m)) is reset in draw 0
 *   and updated online; in draw K-1 row b < n_valid is finalised:
 *     score = m + log(s) - log(K)      (ll itself for K == 1)
 *   stored to scores[first + b] when first + b < cap (and left in run[b][0]).
 *   Rows >= n_valid write nothing but the zeroing.
 *   The advance (its own launch behind the rows, which all read the block):
 *   draw = (draw + 1) % K; after the last draw ll_sum += the finalised scores,
 *   one fp64 addition per row in row order (no atomics: two passes over the
 *   same scores give the same bits), n_scored += n_valid, first += n_valid,
 *   and overflow = 1 when first + n_valid > cap (nothing is written past cap,
 *   no error status: the host reads the flag with the results).
 *
 * Both check their arguments before any HIP call: RNVP_E_INVALID for a NULL
 * x / y / logdet / ctl (z / ldj / logdet / run / ctl), a pointer that is not
 * 4-byte (ctl: 8-byte) aligned, B < 0, C / H / W <= 0 or C*H*W > 2^31 - 1
 * (n_per_sample <= 0).  B == 0 is RNVP_OK with nothing launched.  1 <=
 * n_valid <= B and n_draws >= 1 are the writer's responsibility. */
typedef struct rnvp_score_ctl {
    float* scores;          /* host: destination of the pass, cap floats (device memory) */
    long long cap;          /* host */
    long long first;        /* global index of row 0 of the running batch; device-advanced */
    long long n_scored;     /* images finalised in this pass; device */
    double ll_sum;          /* sum of their scores, fp64, added in row order; device */
    int n_valid;            /* host: rows of the running batch that are images, 1..B */
    int n_draws;            /* host: K >= 1 */
    int draw;               /* 0..K-1; device-advanced */
    int overflow;           /* device: set when first + n_valid > cap */
} rnvp_score_ctl;
/* sizeof(rnvp_score_ctl), for a binding's mirror (the list of rnvp_struct_size is closed) */
int rnvp_score_struct_size(void);
int rnvp_score_in_fwd(const float* x, const float* noise /* may be NULL */, uint64_t seed, const rnvp_score_ctl* ctl,
                      float constraint, float* y, float* logdet, int B, int C, int H, int W, void* stream);
int rnvp_score_finish(const float* z, float* ldj, float* logdet, float* run, float* lp /* may be NULL */,
                      rnvp_score_ctl* ctl, int B, int n_per_sample, void* stream);

/* ---- latents ---------------------------------------------------------------
 * What a trained flow is used for besides scoring: draws from the prior that
 * belong to the SAMPLE (not to its slot in the batch), the end of a decode
 * into fp32 or bytes, interpolation between latents.  As in "scoring" one
 * device-resident control block carries what changes between replays, so one
 * captured graph serves every batch of every call: the host writes the block
 * with stream-ordered copies / fills, rnvp_latent_out advances it, the
 * library never reads it on the host.  (Encoding needs no entry point of its
 * own: rnvp_score_in_fwd on a private rnvp_score_ctl with n_draws = 1,
 * followed by the eval-mode forward.)
 *
 * rnvp_latent_draw: z[b][e] = ctl->temperature * g over [B][n], g a standard
 * normal from ONE Philox4x32-10 call with counter ((first + b) * n + e, 0, 0)
 * -- the 64-bit index in the first two words, low word first -- and key seed
 * (low, high), as the uniform noise of rnvp_logit_fwd.  Of its four output
 * words w0..w3:
 *   u1 = ((w0 >> 8) + 1) * 2^-24   in (0, 1]
 *   u2 = (w1 >> 8) * 2^-24         in [0, 1)
 *   g  = sqrtf(-2 logf(u1)) * cosf(2 pi u2)       (|g| <= 5.77)
 * in fp32 with the precise library functions.  An element is a function of
 * (seed, its global index, temperature) alone: any batch size, any later call
 * gives the same value.  Reads ctl, never writes it.
 *
 * rnvp_latent_out, a row kernel and then a one-workgroup advance: x is the
 * inverse flow's output [B][n]; v = rnvp_logit_inv's value (the same fp32
 * operations).  Row b < n_valid with 0 <= first + b < cap is stored at row
 * first + b of dst (rows of n elements) as
 *   RNVP_OUT_F32       v itself, unclamped (fp32; dst 4-byte aligned)
 *   RNVP_OUT_U8_ROUND  (uint8) floor(clamp(255 v + 0.5, 0, 255)), the product
 *                      and the sum rounded separately: torch's
 *                      mul(255).add(0.5).clamp(0, 255).to(uint8), which is
 *                      torchvision.utils.save_image's rule (train.py:259)
 *   RNVP_OUT_U8_FLOOR  min(255, floor(256 clamp(v, 0, 1))): the exact inverse
 *                      of the dequantisation (k + u) / 256, 0 <= u < 1
 * Byte rows may start at any address (n need not be a multiple of 4): aligned
 * 4-byte words with single bytes at both ends.  Rows >= n_valid, and rows
 * past cap, store nothing.  The advance (its own launch behind the rows,
 * which all read the block): overflow = 1 when first + n_valid > cap (no
 * error status: the host reads the flag with the results), n_done += the rows
 * stored, first += n_valid.
 *
 * rnvp_latent_mix: a, b [P][n] endpoint latents, t a DEVICE array of T floats,
 * out [P][T][n]; out[p][j] = wa a[p] + wb b[p], the two products and the sum
 * rounded separately in fp32 (so a weight pair (1, 0) returns a[p] itself),
 * the weights formed in fp64 and rounded to fp32 once:
 *   RNVP_MIX_LERP   wa = 1 - t, wb = t                       (ws may be NULL)
 *   RNVP_MIX_SLERP  per pair a.b, |a|^2, |b|^2 in fp64 into ws (3 P doubles,
 *                   caller-owned; the call zeroes what it needs zeroed);
 *                   c = clamp(a.b / (|a| |b|), -1, 1); the lerp weights when
 *                   1 - |c| < 1e-9 or a norm is zero; otherwise Om = acos(c),
 *                   wa = sin((1 - t) Om) / sin Om, wb = sin(t Om) / sin Om
 * The sums are per-workgroup partials: a pair of up to 16384 elements is one
 * workgroup that stores its sums (no atomic, the same bits every time), a
 * longer one at most 8 workgroups with one fp64 atomic each per sum.
 *
 * All three are stream-ordered, capture-safe, allocate nothing, and check
 * their arguments before any HIP call: RNVP_E_INVALID for a NULL z / x / ctl
 * (a / b / t / out; ws with RNVP_MIX_SLERP), a pointer that is not 4-byte
 * (ctl, ws: 8-byte) aligned, B / P / T / n < 0, a B * n (P * T * n) beyond
 * 2^63 - 1, P * T > 2^31 - 1, or an unknown mode.  A zero size is RNVP_OK
 * with nothing launched.  0 <= n_valid <= B, first >= 0 and temperature >= 0
 * are the writer's responsibility. */
enum { RNVP_OUT_F32 = 0, RNVP_OUT_U8_ROUND = 1, RNVP_OUT_U8_FLOOR = 2 };
enum { RNVP_MIX_LERP = 0, RNVP_MIX_SLERP = 1 };
typedef struct rnvp_latent_ctl {
    void* dst;              /* host: destination of the finished rows, cap rows of n elements (fp32 or uint8) */
    long long cap;          /* host */
    long long first;        /* global index of row 0 of the running batch; device-advanced */
    long long n_done;       /* rows stored so far; device */
    float temperature;      /* host: the prior's standard deviation (rnvp_latent_draw) */
    int n_valid;            /* host: rows of the running batch that are real, 0..B */
    int overflow;           /* device: set when first + n_valid > cap */
    int pad;
} rnvp_latent_ctl;
/* sizeof(rnvp_latent_ctl), for a binding's mirror (the list of rnvp_struct_size is closed) */
int rnvp_latent_struct_size(void);
int rnvp_latent_draw(float* z, uint64_t seed, const rnvp_latent_ctl* ctl, int B, long long n, void* stream);
int rnvp_latent_out(const float* x, rnvp_latent_ctl* ctl, float constraint, int B, long long n, int mode,
                    void* stream);
int rnvp_latent_mix(const float* a, const float* b, const float* t, float* out, int P, int T, long long n, int mode,
                    double* ws /* RNVP_MIX_SLERP: 3 P doubles */, void* stream);

/* ---- net steps ------------------------------------------------------------
 * One s/t-net step as a table entry (rnvp_net_group): a conv (rnvp_conv2d
 * semantics) or a BatchNorm-backward apply (rnvp_bn_bwd_apply semantics).
 * grad_base-relative dgamma_off / dbeta_off (elements, < 0 = not written)
 * locate a BN step's affine gradients. */
enum { RNVP_STEP_CONV = 0, RNVP_STEP_BN_BWD = 1 };
typedef struct rnvp_net_step {
    int kind;
    rnvp_conv_args conv;
    rnvp_bn_bwd_args bn;
    long long dgamma_off, dbeta_off;
    /* filled by rnvp_net_group_prepare */
    int cfg, nc, shards, xa, xb, tiles;
} rnvp_net_step;

/* ---- grouped 1x1 convs --------------------------------------------------
 * Up to RNVP_NET_GROUP_MAX INDEPENDENT 1x1 convs of one net (same pixels; no
 * conv reads what another writes) in ONE launch: the workgroups of all of
 * them share the grid, so one conv's memory waits overlap another's MFMAs
 * and the kernel boundaries between them disappear.  Used for the skip convs
 * of ResidualModule (modules_realnvp.py:184-189): each core_skips[i] forward
 * runs beside the next block's first 1x1, and the data gradients of
 * in_skip + every core_skips[i] (all read d out) run as one launch.
 * Steps are rnvp_net_step with kind RNVP_STEP_CONV (rnvp_conv2d semantics,
 * with or without the BN prologue).  rnvp_net_group_prepare (host) validates
 * and fills the derived fields (RNVP_E_UNSUPPORTED: no grouped form -- launch
 * them one by one); rnvp_net_group launches the filled HOST table: the
 * members travel by value in the kernel arguments (pointers read from the
 * argument segment address global memory; read from a device table they
 * would be generic, flat operations).  The table may be reused or freed as
 * soon as the call returns (stream capture records the arguments). */
#define RNVP_NET_GROUP_MAX 8
int rnvp_net_group_prepare(rnvp_net_step* steps_host, int n, int* klass, int* grid, int* lds_bytes);
int rnvp_net_group(const rnvp_net_step* steps_host, int n, int dtype, int klass, int grid, int lds_bytes,
                   void* stream);

/* misc */
int rnvp_fill_f64(double* p, long long n, double v, void* stream);

#ifdef __cplusplus
}
#endif
#endif
