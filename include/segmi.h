/* segmi.h -- C ABI of libsegmi.so: the MI355X (gfx950) hot path behind segmantic's
 * `segmantic-unet train / train-config / predict` surface.
 *
 * The reference (dyollb/segmantic) is pure Python and has no FFI of its own: its arithmetic is
 * delegated to torch.nn / MONAI / SimpleITK.  Each entry point
 * below therefore cites the reference *call site* whose third-party operator it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - every function returns 0 on success, a negative SEGMI_E* code on failure;
 *    segmi_last_error() returns a thread-local message for the last failure.
 *  - all pointers are DEVICE pointers unless the name ends in _host; nothing is allocated or
 *    freed behind the caller's back, no ownership is transferred.
 *  - `stream` is a hipStream_t (0 = default stream); every call is asynchronous on it.
 *  - activations are NDHWC ("channels last"): element (n,z,y,x,c) of a view lives at
 *    data[(((n*d + z)*h + y)*w + x)*ld + c]; ld >= c allows concat-by-offset views.
 *  - dtype: SEGMI_F32 (exact-f32 MFMA path, parity mode), SEGMI_BF16 (bf16 storage,
 *    f32 accumulation) or SEGMI_F16 (IEEE fp16 storage, f32 accumulation).  Every entry point
 *    that takes SEGMI_BF16 takes SEGMI_F16 with the same semantics and the same kernel family;
 *    "bf16" below stands for either 16-bit format unless it says otherwise.
 */
#ifndef SEGMI_H_
#define SEGMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGMI_VERSION 1

enum { SEGMI_F32 = 0, SEGMI_BF16 = 1, SEGMI_F16 = 2 };
enum { SEGMI_OK = 0, SEGMI_EINVAL = -1, SEGMI_EUNSUPPORTED = -2, SEGMI_ELAUNCH = -3,
       SEGMI_EDATA = -4 /* the data cannot be processed (an empty or constant N4 fit set) */ };

/* NDHWC activation view */
typedef struct segmi_act {
  void* data;
  int32_t n, d, h, w; /* batch and spatial extents            */
  int32_t c;          /* channels of this view                */
  int32_t ld;         /* elements between consecutive voxels  */
} segmi_act;

int segmi_version(void);
const char* segmi_last_error(void);
/* A HIP stream restricted to `cus_enabled` compute units (a multiple of 8: the first cus_enabled / 8 CUs
 * of every XCD; hipExtStreamCreateWithCUMask).  For the weight-gradient stream of a training step, which
 * the reference leaves to autograd's single stream (monai_unet.py:345): the persistent weight-gradient
 * kernels then cannot take every CU away from the dependent chain of the main stream. */
int segmi_stream_create_cumask(int cus_enabled, void** stream_out);
int segmi_stream_destroy(void* stream);

/* ---------------------------------------------------------------- weights -------------- */
/* Fragment-packed weights: the layout the MFMA kernels stream as B/A operands.
 * kind: 0 = Conv3d forward            (src = torch Conv3d weight [Cout][Cin][k][k][k])
 *       1 = Conv3d stride-1 dgrad     (same src; flipped taps, channels transposed)
 *       2 = transposed-conv kernel    (src = torch ConvTranspose3d weight [Cin][Cout][3][3][3],
 *                                      or a stride-2 Conv3d weight for its dgrad)
 * cin/cout are those of the *source* tensor's role in the kernel that will consume the pack
 * (see DESIGN.md "weight packs").  scale (nullable, f32[cout_k]) folds a per-output-channel
 * factor (eval-mode BatchNorm) into the weights.
 * Replaces: weight handling inside torch.nn.Conv3d / ConvTranspose3d reached from
 * src/segmantic/seg/monai_unet.py:114-124,221-222. */
int64_t segmi_wpack_bytes(int dtype, int kind, int cin_k, int cout_k, int ksize);
int segmi_wpack(int dtype, int kind, const float* w_src, const float* scale, int cin_k,
                int cout_k, int ksize, void* packed, void* stream);

/* Batched form: one launch re-packs every convolution of a network after an optimiser step
 * (the per-step equivalent of torch re-reading .weight in each Conv3d.forward/backward).
 * `descs_host[ndesc]` is validated on the host on every call; when `upload` != 0 it is copied
 * (stream-ordered) into `descs_dev` (device, ndesc * sizeof(segmi_wpack_desc) bytes) first,
 * otherwise `descs_dev` must already hold the same table from an earlier call. */
typedef struct segmi_wpack_desc {
  const float* w_src;  /* device f32 source weight                                   */
  const float* scale;  /* device f32[cout_k] or NULL                                 */
  void* packed;        /* device destination, segmi_wpack_bytes(...) bytes            */
  int32_t kind, cin_k, cout_k, ksize;
  /* kind 0: output channels >= cout_split come from a second source [cout_k - cout_split][cin_k][taps] (the pair
   * pack of segmi_conv3d_fwd_split_act out of two separate parameter tensors); kind 2: INPUT channels >= cout_split
   * come from the second source [cin_k - cout_split][cout_k][27] (the paired input gradient of those two
   * convolutions: one transposed convolution over their concatenated output gradients); NULL = one source */
  const float* w_src2;
  int32_t cout_split, reserved;
} segmi_wpack_desc;
int segmi_wpack_batch(int dtype, const segmi_wpack_desc* descs_host, int ndesc,
                      segmi_wpack_desc* descs_dev, int upload, void* stream);

/* ---------------------------------------------------------------- convolution ---------- */
/* Conv3d k in {1,3}, stride in {1,2}, pad (k-1)/2, fused epilogue:
 *   v = conv(in) + bias ; stats += (v, v^2) ; v = prelu(v) ; v += residual ; out = v
 * bias f32[cout] nullable; prelu_alpha device f32* nullable; residual nullable;
 * stats_partials nullable: f32[segmi_conv3d_stats_rows(...)][2][cout] per-workgroup partial
 * sums of v and v^2 over valid voxels (deterministic; reduced by segmi_bn_finalize).
 * MFMA path needs cin % 16 == 0 and cout % 16 == 0 with a kind-0/1 pack; otherwise pass
 * packed = NULL and w_src = torch-layout f32 weights for the direct kernel.
 * Replaces torch.nn.Conv3d under monai UNet, src/segmantic/seg/monai_unet.py:114-124,341. */
int segmi_conv3d_stats_rows(int dtype, const segmi_act* in, const segmi_act* out, int ksize,
                            int stride);
/* Optional input transform of a convolution (forward and weight gradient): the consumer applies the
 * PRODUCER layer's BatchNorm-apply + PReLU, in' = prelu(in * scale[c] + shift[c]) rounded to the
 * storage type, while it stages its input, so the normalised activation is never written to HBM
 * (zero padding stays zero; an identity residual `residual == in` adds in').  scale / shift: device
 * f32[cin] as written by segmi_bn_finalize; prelu_alpha: device f32* or NULL.  Bit-identical to
 * running segmi_bn_act_fwd first.  segmi_conv3d_in_affine_ok() says whether the layer's kernels
 * implement it (bf16 z-marching ring forward + MFMA weight gradient); pass NULL otherwise.
 * Replaces the separate ADN pass between two torch modules of monai UNet, monai_unet.py:114-124. */
typedef struct segmi_in_affine {
  const float* scale;
  const float* shift;
  const float* prelu_alpha;
} segmi_in_affine;
/* Finalisation of a BatchNorm reduction carried out BY THE LAUNCH THAT PRODUCES THE PARTIAL ROWS: the
 * workgroup that finishes last folds the rows in a fixed order (f64) and writes the per-channel
 * results, so that no separate segmi_bn_finalize / segmi_bn_act_bwd_finalize launch sits on the
 * dependent chain of the stream (csrc/fin_tail.h; ~40 launches per training step).  Deterministic:
 * the fold order depends on the table shape only.  Same argument meaning as the separate calls.
 * Replaces the statistics half of torch.nn.BatchNorm3d forward / backward under monai ADN,
 * monai_unet.py:114-124, 345. */
typedef struct segmi_bn_fin {       /* = the arguments of segmi_bn_finalize */
  double count;                     /* voxels per channel (N*D*H*W of the conv output) */
  const float* gamma;               /* nullable = 1 */
  const float* beta;                /* nullable = 0 */
  float* running_mean;              /* nullable */
  float* running_var;               /* nullable */
  float momentum, eps;
  float* mean;
  float* invstd;
  float* scale;
  float* shift;
} segmi_bn_fin;
typedef struct segmi_bn_bwd_fin {   /* = the arguments of segmi_bn_act_bwd_finalize */
  double count;
  float* dgamma;                    /* nullable */
  float* dbeta;                     /* nullable */
  float* dalpha;                    /* nullable */
  float* coef;                      /* f32[2][c] for segmi_bn_act_bwd_apply */
} segmi_bn_bwd_fin;
/* Optional epilogue of an INPUT-GRADIENT convolution (segmi_conv3d_fwd with a kind-1 pack) whose
 * output `out` is the gradient g flowing into a training-mode BatchNorm + PReLU: with x = that
 * layer's forward input (the raw output of its producer conv, same extents as `out`) the kernel
 * also accumulates the three per-channel sums that segmi_bn_act_bwd_reduce would compute from
 * (g, x) in a separate 2-tensor pass -- sum dz, sum dz*xhat, sum g*z[z<=0] -- taken of the STORED
 * (rounded) gradient, one partial row per workgroup: partials f32 [rows][3][c] with rows =
 * segmi_conv3d_stats_rows(in, out, ksize, stride); feed them to segmi_bn_act_bwd_finalize.
 * segmi_conv3d_bn_bwd_sums_ok() says whether the layer's kernel implements it (bf16 z-marching
 * ring, 16 -> 16 channels); pass NULL otherwise.  Replaces autograd's separate BatchNorm / PReLU
 * backward reductions under monai ADN, monai_unet.py:114-124, 345. */
typedef struct segmi_bn_bwd_sums {
  const segmi_act* x;
  const float* mean;
  const float* invstd;
  const float* gamma;        /* nullable = 1 */
  const float* beta;         /* nullable = 0 */
  const float* prelu_alpha;  /* nullable = no activation */
  float* partials;
  const segmi_bn_bwd_fin* fin;   /* nullable: also finalise in this launch (then no segmi_bn_act_bwd_finalize) */
} segmi_bn_bwd_sums;
int segmi_conv3d_bn_bwd_sums_ok(int dtype, const segmi_act* in, const segmi_act* out, int ksize,
                                int stride);
/* Which forward kernel family segmi_conv3d_fwd() runs for this layer shape: a static string such as
 * "conv_ring2_kernel<bf16, CK=16, NT=1>" (reports / benchmarks label their roofline line with it). */
const char* segmi_conv3d_fwd_kernel_name(int dtype, const segmi_act* in, const segmi_act* out,
                                         int ksize, int stride);
int segmi_conv3d_in_affine_ok(int dtype, const segmi_act* in, const segmi_act* out, int ksize,
                              int stride);
int segmi_conv3d_fwd(int dtype, const segmi_act* in, const segmi_act* out, const void* packed,
                     const float* w_src, int w_kind, const float* bias,
                     const float* prelu_alpha, const segmi_act* residual,
                     float* stats_partials, int ksize, int stride, const segmi_in_affine* in_tf,
                     const segmi_bn_bwd_sums* bn_bwd /* nullable */,
                     const segmi_bn_fin* stats_fin /* nullable; needs stats_partials */, void* stream);
/* Inference, full-resolution decoder of monai UNet as ONE launch (csrc/dectop.hip):
 *   h = PReLU(ConvTranspose3d(k3, s2, p1, op1; 32 -> 16)(in) with BatchNorm folded), out = Conv3d(k3; 16 -> 16)(h) + bias + h
 * i.e. `up` layer "model.2.0" followed by the conv-only ResidualUnit "model.2.1" (monai_unet.py:114-124), whose
 * 16-channel intermediate then never reaches HBM.  Bit-identical to segmi_convT3d_fwd + segmi_conv3d_fwd.
 * up_frag: bf16 [27][64][8]: tap (kd*3+kh)*3+kw, lane (g, co), W_T[ci = 8g .. 8g+7][co][tap] * bn_scale[co];
 * up_bias: f32[16] folded bias; up_alpha: PReLU slope; conv_packed: kind-0 segmi_wpack of the 16 -> 16 conv.
 * segmi_dectop_ok(): bf16, in [N,D,H,W,32], out [N,2D,2H,2W,16] with 2D % 4 == 0, 2H % 16 == 0, 2W % 16 == 0. */
int segmi_dectop_ok(int dtype, const segmi_act* in, const segmi_act* out);
int segmi_dectop_fwd(int dtype, const segmi_act* in, const segmi_act* out, const void* up_frag,
                     const float* up_bias, const float* up_alpha,
                     int up_alpha_in_unit_range /* caller asserts 0 <= *up_alpha <= 1: PReLU as max(v, slope v), same bits */,
                     const void* conv_packed, const float* conv_bias, void* stream);
/* The first ResidualUnit of the network convolves its (<= 4 channel) input twice with the same
 * geometry: subunit 0 (k3, stride s) and the residual convolution (k3, stride s).  One launch
 * stages the input once and produces both:  out_a = prelu_a(conv_a(in) + bias_a) with optional
 * statistics of the pre-activation values (rows as segmi_conv3d_stats_rows(in, out_a)),
 * out_b = conv_b(in) + bias_b.  w_a / w_b are torch-layout f32 [cout][cin][27].
 * segmi_conv3d_pair_ok() says whether the layer qualifies (1) or needs two segmi_conv3d_fwd (0).
 * Replaces the two torch.nn.Conv3d of monai ResidualUnit, monai_unet.py:114-124. */
/* Window views (inference): sample n of `in` is not a slice of a dense batch but the (d, h, w) block that starts
 * offset[n] elements into a larger single-channel volume (`in->data` = the volume, row / plane strides in
 * elements), with ZERO padding at the block's own borders -- the windows of MONAI's sliding_window_inference
 * (monai_unet.py:354-356, 637-639, 665) read in place, instead of being gathered into a batch first.  <= 32
 * windows per call; offsets and strides multiples of 4 elements. */
typedef struct segmi_windows {
  int32_t count;
  int32_t row_stride;
  int64_t plane_stride;
  int64_t offset[32];
} segmi_windows;
int segmi_conv3d_pair_ok(int dtype, const segmi_act* in, const segmi_act* out_a,
                         const segmi_act* out_b);
/* The same pairing for MFMA layers (the stride-2 first subunit + residual convolution of the deeper
 * ResidualUnits, inference): ONE convolution whose fragment pack holds both weight sets
 * (segmi_wpack of the concatenated [2c][cin][27] weight, per-channel scale = folded BatchNorm for the
 * first c outputs, 1 for the rest) writes 2c channels, PReLU only on the first `act_channels`:
 *   out[..., :act_channels] = prelu(conv_a(in) + bias[:c]) ; out[..., act_channels:] = conv_b(in) + bias[c:]
 * Consumers read the two halves as channel-slice views (ld = 2c).  Same bits as the two calls.
 * Training (round 4; replaces the two torch convolutions of a ResidualUnit's first subunit and residual path,
 * monai_unet.py:341 through monai.networks.blocks.ResidualUnit): prelu_alpha = NULL, `bias_b` = the second
 * convolution's bias (nullable: then bias holds all 2c values), `stats_partials` / `stats_fin` = BatchNorm statistics
 * rows [segmi_conv3d_stats_rows][2][act_channels] of the FIRST act_channels outputs and their finalisation in the
 * same launch; the pack comes from a segmi_wpack_desc with two sources (w_src2 / cout_split). */
int segmi_conv3d_split_act_ok(int dtype, const segmi_act* in, const segmi_act* out, int ksize,
                              int stride);
int segmi_conv3d_fwd_split_act(int dtype, const segmi_act* in, const segmi_act* out,
                               const void* packed, const float* bias, const float* prelu_alpha,
                               int act_channels, int ksize, int stride,
                               const float* bias_b /* nullable */, float* stats_partials /* nullable */,
                               const segmi_bn_fin* stats_fin /* nullable; needs stats_partials */, void* stream);
int segmi_conv3d_fwd_pair(int dtype, const segmi_act* in, const segmi_act* out_a, const float* w_a,
                          const float* bias_a, const float* prelu_alpha_a, float* stats_partials_a,
                          const segmi_act* out_b, const float* w_b, const float* bias_b, int stride,
                          const segmi_bn_fin* stats_fin_a /* nullable; needs stats_partials_a */,
                          const segmi_windows* windows /* nullable: `in` samples are window views */,
                          void* stream);

/* ConvTranspose3d k3 s2 p1 (output extent 2*in or 2*in-1 per dim, taken from `out`),
 * same fused epilogue.  Also the dgrad of a stride-2 Conv3d.
 * Replaces torch.nn.ConvTranspose3d, src/segmantic/seg/monai_unet.py:114-124. */
int segmi_convT3d_stats_rows(int dtype, const segmi_act* in, const segmi_act* out);
int segmi_convT3d_fwd(int dtype, const segmi_act* in, const segmi_act* out, const void* packed,
                      const float* w_src, const float* bias, const float* prelu_alpha,
                      const segmi_act* residual, float* stats_partials,
                      const segmi_bn_fin* stats_fin /* nullable; needs stats_partials */, void* stream);

/* Weight gradient of a Conv3d (k, stride as forward): dw[co][ci][tap] (torch layout, f32) and
 * db[co] (nullable) from x (forward input) and dy (grad of the conv output).  Two-stage
 * deterministic reduction through `workspace` (>= segmi_conv3d_wgrad_workspace bytes).
 * The ConvTranspose3d weight gradient is the same call with x := dy_T, dy := x_T (stride 2).
 * Replaces autograd's conv backward reached from manual_backward,
 * src/segmantic/seg/monai_unet.py:345. */
int64_t segmi_conv3d_wgrad_workspace(int dtype, const segmi_act* x, const segmi_act* dy,
                                     int ksize, int stride, int cus);
int segmi_conv3d_wgrad(int dtype, const segmi_act* x, const segmi_act* dy, float* dw,
                       float* db, int ksize, int stride, void* workspace,
                       const segmi_in_affine* in_tf /* transform of x, nullable */, int cus, void* stream);
/* `cus`: how many compute units the weight-gradient kernels size their grid (and their partial slabs: pass the same
 * value to the workspace query) for -- a multiple of 8 in [8, 256]; <= 0 = the whole chip.  Their workgroups hold a
 * CU exclusively, so a caller that runs them on a side stream beside its dependent chain -- what autograd's single
 * stream cannot do, monai_unet.py:345 -- sizes them for part of the chip.  A per-call argument since round 4 (no
 * process-wide state); the environment variable SEGMI_WGRAD_CUS overrides it for A/B runs.  segmi_wgrad_cus(cus)
 * returns the count a call with that argument would use. */
int segmi_wgrad_cus(int cus);
/* bias gradient only: db[c] = sum over voxels of dy */
int segmi_bias_grad(int dtype, const segmi_act* dy, float* db, void* workspace, void* stream);

/* ---------------------------------------------------------------- norm + activation ---- */
/* BatchNorm3d (training statistics) + PReLU, MONAI ADN "NDA" ordering.
 * Replaces torch.nn.BatchNorm3d / PReLU under monai ADN, monai_unet.py:114-124. */
int segmi_bn_stats_rows(const segmi_act* x);
int segmi_bn_stats(int dtype, const segmi_act* x, float* stats_partials, void* stream);
/* partials f32[rows][2][c] -> mean, invstd, scale = gamma*invstd, shift = beta - mean*scale;
 * running_mean/var (nullable) updated with `momentum` and the unbiased variance. */
int segmi_bn_finalize(const float* stats_partials, int rows, int c, double count,
                      const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float momentum, float eps, float* mean,
                      float* invstd, float* scale, float* shift, void* stream);
/* eval mode: scale/shift from running statistics */
int segmi_bn_eval_affine(int c, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps,
                         float* scale, float* shift, void* stream);
/* y = prelu(drop(x*scale + shift)) + residual   (alpha nullable -> identity, residual nullable).
 * MONAI ADN "NDA" dropout (the `dropout` key of the config, monai_unet.py:107,119): with
 * dropout_p > 0 an element is kept iff hash(dropout_seed, logical NDHWC element index) >> 8 >=
 * dropout_p * 2^24 and kept values are scaled by 1 / (1 - p); the mask is never stored, the two
 * backward passes recompute it from the same seed.  dropout_p = 0 (eval, default): identity. */
int segmi_bn_act_fwd(int dtype, const segmi_act* x, const segmi_act* y, const float* scale,
                     const float* shift, const float* prelu_alpha, const segmi_act* residual,
                     float dropout_p, uint32_t dropout_seed, void* stream);
/* backward of y = prelu(drop(bn(x))):  pass 1 reduces, finalize, pass 2 writes dx.
 * red_partials f32[rows][3][c]: sum dz, sum dz*xhat, sum dy*z*[z<=0]  (dz = dy*prelu'(z)*mask) */
int segmi_bn_act_bwd_rows(const segmi_act* x);
int segmi_bn_act_bwd_reduce(int dtype, const segmi_act* dy, const segmi_act* x,
                            const float* mean, const float* invstd, const float* gamma,
                            const float* beta, const float* prelu_alpha, float* red_partials,
                            float dropout_p, uint32_t dropout_seed,
                            const segmi_bn_bwd_fin* fin /* nullable: finalise in this launch */, void* stream);
int segmi_bn_act_bwd_finalize(const float* red_partials, int rows, int c, double count,
                              const float* gamma, const float* invstd, float* dgamma,
                              float* dbeta, float* dalpha, float* coef, void* stream);
/* The three calls above as ONE launch for small tensors (<= 32 MB, <= 256 channels in multiples of 4, no
 * dropout): the workgroups reduce, the last one finalises and publishes the coefficients, all apply
 * (a grid-wide hand-off through device-scope atomics; csrc/norm_act.hip).  red_partials: f32
 * [segmi_bn_act_bwd_fused_rows(x)][3][c].  Same results as the three calls up to the f32 summation order of the
 * partial rows.  Replaces autograd's BatchNorm / PReLU backward under monai ADN, monai_unet.py:114-124, 345.
 * Residency: a workgroup of this launch holds a whole CU and waits on it for the last one, so the launch uses at
 * most as many workgroups as the device holds at once (occupancy query x compute units; _ok returns 0 on a device
 * that cannot hold one) and at most `max_wgs` (> 0): a caller that runs CU-exclusive kernels on another stream
 * (segmi_conv3d_wgrad with `cus`) passes the CUs they leave free; <= 0 = the device's capacity.
 * segmi_bn_act_bwd_fused_wgs: the workgroup count a call would launch.  A waiting workgroup gives up after a
 * bounded number of polls (about a second), writes NaN gradients and counts the expiry; segmi_fused_timeouts(reset)
 * returns the count from host-visible memory WITHOUT a device sync (expiries of launches that have executed so far)
 * -- a non-zero value means gradients of this process are poisoned (the reference stops on a non-finite
 * loss, monai_unet.py:512-518 `check_finite`); the Python engine raises.  segmi_fused_test_hook: tests only --
 * a poll bound (0 = default) and `no_publish` (the finalising workgroup withholds the flag: every waiter expires). */
int segmi_bn_act_bwd_fused_ok(int dtype, const segmi_act* dy, const segmi_act* x, const segmi_act* dx);
int segmi_bn_act_bwd_fused_rows(const segmi_act* x);
int segmi_bn_act_bwd_fused_wgs(int dtype, const segmi_act* x, int max_wgs);
int segmi_bn_act_bwd_fused(int dtype, const segmi_act* dy, const segmi_act* x, const segmi_act* dx,
                           const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* prelu_alpha, float* red_partials, const segmi_bn_bwd_fin* fin,
                           int max_wgs, void* stream);
unsigned segmi_fused_timeouts(int reset);
int segmi_fused_test_hook(unsigned poll_limit, int no_publish);
int segmi_bn_act_bwd_apply(int dtype, const segmi_act* dy, const segmi_act* x,
                           const segmi_act* dx, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, const float* prelu_alpha,
                           const float* coef, float dropout_p, uint32_t dropout_seed, void* stream);
/* segmi_bn_act_bwd_apply fused into the k3 stride-2 convolution that consumes its result -- the input gradient
 * of a decoder level's ConvTranspose3d (monai UNet up layer, monai_unet.py:114-124; backward of :345): the
 * convolution computes dx = apply(dy, x) while it stages its halo tile, feeds the bf16-rounded values to its
 * MFMAs and writes dx once (for the weight gradient): same bits as the two calls, one pass over dx less.
 * bf16, 16 channels, out->c in {16, 32, 64}, out->w >= 16, no dropout; `packed`: segmi_wpack of the
 * convolution (kind 0, as segmi_conv3d_fwd takes it).  dx must not alias dy or x. */
int segmi_bn_act_bwd_apply_conv_ok(int dtype, const segmi_act* dy, const segmi_act* x, const segmi_act* dx,
                                   const segmi_act* out);
int segmi_bn_act_bwd_apply_conv(int dtype, const segmi_act* dy, const segmi_act* x, const segmi_act* dx,
                                const float* mean, const float* invstd, const float* gamma, const float* beta,
                                const float* prelu_alpha, const float* coef, const segmi_act* out,
                                const void* packed, void* stream);

/* elementwise helpers on NDHWC views */
int segmi_add(int dtype, const segmi_act* a, const segmi_act* b, const segmi_act* out,
              void* stream);                       /* out = a + b (b nullable -> copy)        */
int segmi_cast_copy(int src_dtype, const segmi_act* src, int dst_dtype, const segmi_act* dst,
                    void* stream);                 /* dtype / ld converting copy              */
int segmi_nchw_to_ndhwc(const float* src, int dst_dtype, const segmi_act* dst, void* stream);
int segmi_ndhwc_to_nchw(int src_dtype, const segmi_act* src, float* dst, void* stream);

/* ---------------------------------------------------------------- loss + optimiser ----- */
/* MONAI DiceLoss(to_onehot_y=True, softmax=True), monai_unet.py:128,344.
 * labels: f32[n*d*h*w] integer-valued class ids.  partials f32[segmi_dice_chunks()][n][3][k]
 * (the count includes a tail of rows that is no longer read or written: it remains only so that buffers
 * sized by it stay large enough); n * k <= 2389 (the finalisation's LDS); coef f32[n][2][k] receives the
 * backward coefficients; loss f32[1]. */
int segmi_dice_chunks(const segmi_act* logits);
int segmi_softmax_dice_fwd(int dtype, const segmi_act* logits, const float* labels,
                           float* partials, float* coef, float* loss, float smooth_nr,
                           float smooth_dr, void* stream);
/* backward: dlogits = grad_scale * dLoss/dlogits.  bias_grad (nullable, f32[k]): also the channel
 * sums of dlogits -- the bias gradient of the layer that produced the logits -- folded into the same
 * pass; it needs `scratch` = the forward's `partials` buffer (free again after the forward). */
int segmi_softmax_dice_bwd(int dtype, const segmi_act* logits, const float* labels,
                           const float* coef, float grad_scale, const segmi_act* dlogits,
                           float* scratch, float* bias_grad, void* stream);

/* Dice + cross-entropy on the same two passes:
 *   loss = lambda_dice * Dice + lambda_ce * CE
 *   Dice: the term above; include_background = 0 drops class 0 after the softmax (mean over n * (k - 1);
 *         k = 1 is then refused).
 *   CE:   torch cross_entropy(logits, labels, weight = class_weight, reduction = "mean") over all voxels of the
 *         batch: sum_v w[y_v] * (-log p_{v,y_v}) / W with W = sum_v w[y_v] (batch-global; W = 0 gives NaN as in
 *         torch).  -log p is formed as log sum_j exp(x_j - m) - (x_y - m), never as the log of a stored
 *         probability.  lambda_ce = 0 switches the term off (no NaN from W = 0 then).
 *   A voxel whose label lies outside [0, k) contributes to neither CE nor W (nor to the Dice target sums).
 * class_weight: nullable DEVICE f32[k] (NULL = ones), entries finite and >= 0 (not checked on the device);
 * lambda_dice, lambda_ce: finite and >= 0; n * k <= 1792 (the finalisation's LDS).  partials f32[segmi_dice_ce_chunks()][n][4][k]; coef f32[n][3][k]
 * receives the backward coefficients: the Dice pair scaled by lambda_dice (zero for an excluded background)
 * and c_k = lambda_ce * w_k / W; loss f32[1].  The lambdas, the weights and include_background reach the
 * backward through coef alone:
 *   dlogits_j = scale * [ lambda_dice * (Dice term) + c_y * (p_j - [j = y]) ],  scale = grad_scale or amp[0].
 * scratch / bias_grad as for segmi_softmax_dice_bwd (scratch = the forward's 4-row partials buffer).  With
 * lambda_dice = 1, lambda_ce = 0, include_background = 1 loss and dlogits are those of segmi_softmax_dice_fwd /
 * _bwd bit for bit. */
int segmi_dice_ce_chunks(const segmi_act* logits);
int segmi_softmax_dice_ce_fwd(int dtype, const segmi_act* logits, const float* labels, float* partials,
                              float* coef, float* loss, float smooth_nr, float smooth_dr, float lambda_dice,
                              float lambda_ce, int include_background, const float* class_weight, void* stream);
int segmi_softmax_dice_ce_bwd(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                              float grad_scale, const segmi_act* dlogits, float* scratch, float* bias_grad,
                              void* stream);
/* ... with the loss scale read from amp[0] on the device (see "dynamic loss scaling" below) */
int segmi_softmax_dice_ce_bwd_amp(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                  const float* amp, const segmi_act* dlogits, float* scratch, float* bias_grad,
                                  void* stream);

/* Tversky / focal Tversky on the Dice passes.  With I, P, T the per-(n, k) sums of the Dice
 * forward (intersection, sum p, sum t; softmax over all k classes):
 *   TI = (I + smooth_nr) / (I + alpha (P - I) + beta (T - I) + smooth_dr)
 *   loss = mean over the included (n, k) of (1 - TI)^exponent
 * alpha weighs false positives, beta false negatives (MONAI's TverskyLoss); include_background = 0 drops class 0
 * after the softmax (mean over n * (k - 1); k = 1 is then refused).  alpha, beta: finite, >= 0, alpha + beta > 0;
 * exponent in (0, 3] (0.75 is the focal Tversky loss with gamma = 4/3); n * k <= 1792.  Term and coefficients are
 * formed in f64 on the f64 sums.  Where 1 - TI <= 0 (possible only through rounding or smooth_nr > smooth_dr) the
 * term AND its gradient coefficients are 0.  With alpha = beta = 0.5, exponent = 1 and both smooths s / 2 the value is
 * the Dice loss with smooth s.
 * partials f32[segmi_dice_ce_chunks()][n][3][k]; coef f32[n][2][k] receives {d loss / d I, d loss / d P} (zero for an
 * excluded background); loss f32[1].  The backward is the Dice backward on that pair (same kernels, same scratch /
 * bias_grad rule with scratch = this forward's partials): dlogits = scale * dLoss/dlogits, scale = grad_scale or
 * amp[0].  A label outside [0, k) is in no class row. */
int segmi_softmax_tversky_fwd(int dtype, const segmi_act* logits, const float* labels, float* partials, float* coef,
                              float* loss, float smooth_nr, float smooth_dr, float alpha, float beta, float exponent,
                              int include_background, void* stream);
int segmi_softmax_tversky_bwd(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                              float grad_scale, const segmi_act* dlogits, float* scratch, float* bias_grad,
                              void* stream);
int segmi_softmax_tversky_bwd_amp(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                  const float* amp, const segmi_act* dlogits, float* scratch, float* bias_grad,
                                  void* stream);

/* Dice + focal cross-entropy on the Dice + cross-entropy passes:
 *   loss = lambda_dice * Dice + lambda_focal * Focal
 *   Focal = sum_v w[y_v] * q_v^gamma * nll_v / W,  nll_v = -log p_{v,y_v} as segmi_softmax_dice_ce_fwd forms it,
 *           q_v = 1 - p_{v,y_v} formed as the sum of the other probabilities (q = 0 contributes 0), W = sum_v w[y_v]
 *           batch-global: the cross-entropy term's normaliser (W = 0 gives NaN; lambda_focal = 0 switches the term off).
 * gamma: 0 or in [1, 5].  gamma = 0 runs the Dice + cross-entropy kernels themselves: loss and dlogits are those of
 * segmi_softmax_dice_ce_fwd / _bwd with lambda_ce = lambda_focal bit for bit.  f32 uses powf / logf, the 16-bit types
 * the hardware log2 / exp2.  Buffers, class_weight, include_background, the label rule and n * k <= 1792 as for
 * segmi_softmax_dice_ce_fwd (partials f32[segmi_dice_ce_chunks()][n][4][k], coef f32[n][3][k]).  The backward needs
 * the same gamma; per voxel it adds  scale * g_v * c_y * (p_j - [j = y]),  g_v = q^gamma + gamma q^(gamma-1) nll_v p_y,
 * with nll_v recomputed. */
int segmi_softmax_dice_focal_fwd(int dtype, const segmi_act* logits, const float* labels, float* partials,
                                 float* coef, float* loss, float smooth_nr, float smooth_dr, float lambda_dice,
                                 float lambda_focal, float gamma, int include_background, const float* class_weight,
                                 void* stream);
int segmi_softmax_dice_focal_bwd(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                 float gamma, float grad_scale, const segmi_act* dlogits, float* scratch,
                                 float* bias_grad, void* stream);
int segmi_softmax_dice_focal_bwd_amp(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                     float gamma, const float* amp, const segmi_act* dlogits, float* scratch,
                                     float* bias_grad, void* stream);

/* torch.optim.Adam / SGD semantics over one flat f32 arena, monai_unet.py:292-304,346, and
 * adabelief_pytorch.AdaBelief(rectify=False, fixed_decay=False), monai_unet.py:305-314.
 * Hyper-parameters are doubles, as the Python optimisers hold them: derived scalars (1 - beta,
 * lr / bias_correction, ...) are formed in double and rounded to f32 once, like torch's scalar
 * arguments.  grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). */
int segmi_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    float* max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                    double eps, double weight_decay, int64_t step, float grad_scale,
                    void* stream);
int segmi_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, double lr,
                   double momentum, double weight_decay, int first_step, float grad_scale,
                   void* stream);
int segmi_adabelief_step(float* param, const float* grad, float* exp_avg, float* exp_avg_var,
                         int64_t n, double lr, double beta1, double beta2, double eps,
                         double weight_decay, int weight_decouple, int64_t step,
                         float grad_scale, void* stream);

/* ---------------------------------------------------------------- dynamic loss scaling - */
/* fp16 training with torch.amp.GradScaler semantics, every piece of state in device memory (no host
 * synchronisation per step).  amp: f32[3] = {scale, found_inf, skipped steps}; growth_tracker: int32[1]; step: int64[1],
 * the optimiser's count of APPLIED updates (a skipped step does not advance it, as GradScaler skips
 * optimizer.step()).  Per step: segmi_softmax_dice_bwd_amp (dlogits scaled by amp[0]) -> backward
 * (+ gradient all-reduce) -> segmi_amp_check_finite over the whole f32 gradient arena -> a *_step_amp
 * update -> segmi_amp_update_scale.
 * segmi_amp_check_finite: amp[1] = 1 when any grad[i] is Inf or NaN (it never clears it).
 * *_step_amp: as the plain updates with the gradient multiplied by grad_scale and by 1/amp[0] (formed in
 *   double, rounded to f32 once), bias corrections / SGD's first-step rule from step[0] + 1; when amp[1] != 0
 *   params and moments are left bit-untouched.
 * segmi_amp_update_scale: torch._amp_update_scale_ (found_inf: scale *= backoff, tracker = 0; else
 *   tracker + 1, and at growth_interval scale *= growth when that stays finite, tracker = 0); a skipped step
 *   adds 1 to amp[2], an applied one adds 1 to step[0] (step nullable); then amp[1] = 0 for the next step. */
int segmi_softmax_dice_bwd_amp(int dtype, const segmi_act* logits, const float* labels,
                               const float* coef, const float* amp, const segmi_act* dlogits,
                               float* scratch, float* bias_grad, void* stream);
int segmi_amp_check_finite(const float* grad, int64_t n, float* amp, void* stream);
int segmi_amp_update_scale(float* amp, int32_t* growth_tracker, int64_t* step, double growth_factor,
                           double backoff_factor, int growth_interval, void* stream);
int segmi_adam_step_amp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        float* max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                        double eps, double weight_decay, const float* amp, const int64_t* step,
                        float grad_scale, void* stream);
int segmi_sgd_step_amp(float* param, const float* grad, float* momentum_buf, int64_t n, double lr,
                       double momentum, double weight_decay, const float* amp, const int64_t* step,
                       float grad_scale, void* stream);
int segmi_adabelief_step_amp(float* param, const float* grad, float* exp_avg, float* exp_avg_var,
                             int64_t n, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int weight_decouple, const float* amp,
                             const int64_t* step, float grad_scale, void* stream);

/* ---------------------------------------------------------------- sliding window ------- */
/* MONAI sliding_window_inference, monai_unet.py:354-356,637-639,665.
 * starts_host: int32[nwin][3] (z,y,x) window origins in the (padded) image. */
int segmi_sw_gather(int dtype_src, const segmi_act* image, int img_index,
                    const int32_t* starts_host, int nwin, int dst_dtype,
                    const segmi_act* windows, void* stream);
/* acc[z,y,x,k] += w * pred ; cnt[z,y,x] += w  for each window in order (deterministic).
 * importance nullable (constant 1) else f32[roi_d*roi_h*roi_w]. cnt nullable. */
int segmi_sw_scatter_add(int dtype, const segmi_act* pred, const int32_t* starts_host,
                         int nwin, const float* importance, const segmi_act* acc, float* cnt,
                         void* stream);
/* logits = acc / cnt (in place, nullable skip) and labels = argmax_k (first max wins).
 * label_bytes in {1,2,4}. */
int segmi_sw_finalize(const segmi_act* acc, const float* cnt, int write_logits, void* labels,
                      int label_bytes, void* stream);
/* Deferred form of the same blend (same reference call sites): the caller keeps EVERY window
 * prediction of the dense schedule, `cache` = [win_hi - win_lo][rd][rh][rw][ldp >= k] of `dtype`
 * (slot = window index - win_lo; window index = (iz*ny + iy)*nx + ix over the per-dimension origin
 * lists, first dimension slowest -- MONAI's dense_patch_slices order).  One pass sums, per output
 * voxel, the covering windows in ascending window index (the f32 addition order of the
 * reference's sequential `out[slice] += w * pred`), then
 *   normalize != 0: out_logits = sum / count (nullable), labels = argmax_k (nullable)
 *   normalize == 0: out_logits = sum, out_count = count (partial result of a window shard).
 * Origins are host arrays in un-padded image coordinates (may be negative); at most 64 per
 * dimension (SEGMI_EUNSUPPORTED beyond: use the streaming segmi_sw_scatter_add).
 * out_logits: f32 [d][h][w][ldo >= k]; out_count: f32 [d][h][w]; label_bytes in {1,2,4}. */
int segmi_sw_blend(int dtype, const void* cache, int k, int ldp, const int32_t* starts_z, int nz,
                   const int32_t* starts_y, int ny, const int32_t* starts_x, int nx, int win_lo,
                   int win_hi, int rd, int rh, int rw, const float* importance, int d, int h, int w,
                   float* out_logits, int ldo, float* out_count, void* labels, int label_bytes,
                   int normalize, void* stream);
/* Which kernel segmi_sw_blend takes for these arguments (launches nothing; both go through one choice):
 * "sw_blend2_kernel<dt, G=g>" (at most two covering windows per dimension, every load issued up front),
 * "sw_blend_kernel<dt, G=g>" (generic) or "sw_blend_scalar_kernel<dt, G=1>" (one channel per lane, labels from a
 * second pass); G = channels per lane.  "invalid" for arguments segmi_sw_blend refuses outright.  The string is
 * thread-local and valid until the thread's next call. */
const char* segmi_sw_blend_kernel_name(int dtype, const void* cache, int k, int ldp, const int32_t* starts_z, int nz,
                                       const int32_t* starts_y, int ny, const int32_t* starts_x, int nx, int rd,
                                       int rh, int rw, const float* out_logits, int ldo);
/* AsDiscrete(argmax=True), monai_unet.py:129-134,622,673 */
int segmi_argmax(int dtype, const segmi_act* logits, void* labels, int label_bytes,
                 void* stream);
/* per-class overlap counts for DiceMetric (monai_unet.py:136-138): counts i64[k][3] =
 * |pred==c & true==c|, |pred==c|, |true==c| ; labels are int32 */
int segmi_label_counts(const int32_t* pred, const int32_t* truth, int64_t n, int k,
                       int64_t* counts, void* stream);

/* ---------------------------------------------------------------- test-time augmentation */
/* Mirror test-time augmentation and uncertainty read-out (no counterpart in the
 * reference, the definitions are this project's).  2 <= K <= 512 everywhere.
 *
 * One pass: `logits` f32 [1][d][h][w][K] (ld >= K) is the network's result on the volume mirrored along
 * the spatial axes whose bit is set in flip_mask (bit 0 = d, 1 = h, 2 = w).  For output voxel v the
 * source voxel is u, u_a = n_a - 1 - v_a on the mirrored axes; with m = max_c l_c, e_c = expf(l_c - m),
 * s = e_0 + e_1 + ... (ascending c) and p_c = e_c / s, acc[v][c] = p_c when `first`, else acc + p_c.
 * acc: dense f32 [d][h][w][K].  One read of the logits and one read-modify-write of acc per pass; the
 * caller fixes the pass order, so repeated runs are bit-identical. */
int segmi_tta_accumulate(const segmi_act* logits, int flip_mask, float* acc, int first, void* stream);
/* scores: non-negative f32, k channels (the accumulator, or what the inverse pre-processing chain made
 * of it: all-zero voxels outside the crop, border voxels that sum to less than the pass count).  Per
 * voxel s = sum_c scores_c (ascending c); s == 0: label 0, confidence 1, entropy 0, probabilities
 * (1, 0, ...); otherwise q_c = scores_c / s, label = first maximum of q (the rule of segmi_argmax),
 * confidence = q_label, entropy = -(sum_c q_c logf(q_c)) / logf(k) with 0 log 0 = 0, summed in ascending
 * c and clamped to [0, 1].  labels: label_bytes 1 (k <= 256) or 4.  confidence, entropy (f32 per voxel)
 * and probs_out (k channels, ld >= k) may each be NULL; probs_out may be `scores` itself. */
int segmi_tta_finalize(const segmi_act* scores, int k, void* labels, int label_bytes, float* confidence,
                       float* entropy, const segmi_act* probs_out, void* stream);
/* Per label c < k: counts[c] (device i64) = voxels with that label, sums[c] (device f64) = the f64 sum
 * of values over them (labels >= k are skipped; label_bytes 1 or 4; k <= 512).  Deterministic: fixed
 * per-wave order, fixed-order fold by the workgroup that finishes last (csrc/fin_tail.h protocol on f64
 * rows); repeated calls are bit-identical.  The partial tables live in library-owned device memory
 * (4 per device, handed out round-robin: at most 4 calls of one device may be in flight on DIFFERENT
 * streams; calls on one stream are unlimited). */
int segmi_label_means(const void* labels, int label_bytes, const float* values, int64_t n, int k, double* sums,
                      int64_t* counts, void* stream);

/* ---------------------------------------------------------------- image ops ------------ */
/* ITK ResampleImageFilter replacement, src/segmantic/image/processing.py:49-120.
 * index_map_host: 12 doubles, row-major 3x4 affine taking an output index (x,y,z,1) to the
 * continuous input index (x,y,z).  pixel: 0=f32 1=u8 2=i16 3=i32 4=u16.  Arrays are [z][y][x].
 * interp: 0 = linear, 1 = nearest (outside the input buffer -> default_value, as ITK); +2 = border
 * padding: the continuous index is clamped to the buffer first (MONAI Spacingd's padding_mode=
 * "border", monai_unet.py:173-174 and its inverse under Invertd, :615-621); +4 (with 1 only) =
 * nearest rounds x.5 to the even index (torch grid_sample / MONAI mode="nearest") instead of up (ITK). */
int segmi_resample3d(int pixel, const void* src, int sx, int sy, int sz, void* dst, int dx,
                     int dy, int dz, const double* index_map_host, int interp,
                     double default_value, void* stream);
/* The two high-quality interpolators of the resampler (csrc/resample_hq.hip).  Arrays,
 * pixel codes, index_map_host, the inside test -0.5 <= c < n - 0.5, `border` (0 / 1: clamp the continuous index
 * to [0, n-1] first), default_value and the saturate-then-truncate output cast are those of segmi_resample3d; an
 * axis of extent 1 (the 2-D case) is accepted everywhere.  The evaluate and vote kernels launch at most
 * SEGMI_RESAMPLE_HQ_GRID_CAP workgroups of 256 threads and stride over the rest of the output. */
#define SEGMI_RESAMPLE_HQ_GRID_CAP 2048
/* Cubic B-spline (sitkBSpline), in two steps so that one coefficient volume serves several output grids.
 * segmi_bspline_prefilter: native pixels -> float64 coefficients `coef` (device, [sz][sy][sx], the
 * segmi_bspline_workspace(sx, sy, sz) = 8 sx sy sz bytes): the separable recursive filter with pole sqrt(3) - 2 and
 * gain 6 per axis, along x, then y, then z, whole-sample mirror boundaries, the causal start taken from the mirror
 * sum over the whole line (lines longer than 57 samples: its first 56 terms, the rest lying below 2^-106 of the
 * line's largest sample); a line of length 1 is copied.  What scipy.ndimage.spline_filter(order=3, mode="mirror")
 * computes. */
int64_t segmi_bspline_workspace(int sx, int sy, int sz);
int segmi_bspline_prefilter(int pixel, const void* src, int sx, int sy, int sz, double* coef, void* stream);
/* segmi_resample3d_bspline: evaluates `coef` at every output voxel.  Per axis f = floor(c), t = c - f, weights
 * (1-t)^3/6, (3t^3-6t^2+4)/6, (-3t^3+3t^2+3t+1)/6, t^3/6 on taps f-1 .. f+2 folded by the whole-sample mirror
 * (period 2(n-1); extent 1: every tap is sample 0); the 64 products are summed in f64, x innermost and z outermost,
 * and cast to `pixel`.  Equals scipy.ndimage.map_coordinates(order=3, mode="mirror") in float64. */
int segmi_resample3d_bspline(const double* coef, int sx, int sy, int sz, int pixel, void* dst, int dx, int dy, int dz,
                             const double* index_map_host, int border, double default_value, void* stream);
/* Label-Gaussian (sitkLabelGaussian) as an exact integer vote.  sigma_xyz_host: 3 doubles, the Gaussian's sigma per
 * axis (x, y, z) in input voxels, each > 0; alpha > 0; radius R = ceil(alpha * sigma) per axis, refused beyond 8.
 * Per axis i0 = floor(c + 0.5), taps i in [i0 - R, i0 + R] that lie in [0, n-1], weight
 * w(i) = 0.5 (erf(((i + 0.5) - c) inv) - erf(((i - 0.5) - c) inv)) with inv = 1 / (sigma sqrt 2), quantised to
 * q(i) = floor(w(i) 2^18 + 0.5).  A voxel weighs qz qy qx; a label's score is the int64 sum over the window's voxels
 * that carry it; the output is the label with the largest score, the smallest label value among equal scores.
 * f32 labels are compared as numbers (NaN is not supported).  Any number of distinct labels per window. */
int segmi_resample3d_label_gaussian(int pixel, const void* src, int sx, int sy, int sz, void* dst, int dx, int dy,
                                    int dz, const double* index_map_host, const double* sigma_xyz_host, double alpha,
                                    int border, double default_value, void* stream);
/* NormalizeIntensityd(channel_wise=True), monai_unet.py:164: in-place (x-mean)/std per channel
 * of a [c][nvox] f32 array.  workspace >= segmi_normalize_workspace(c, nvox) bytes. */
int64_t segmi_normalize_workspace(int c, int64_t nvox);
int segmi_normalize_intensity(float* x, int c, int64_t nvox, void* workspace, void* stream);
/* on-device patch sampler: copies `count` roi-sized crops (origins in starts_host, int32
 * [count][4] = n,z,y,x) of image (f32 -> dst dtype) and label (f32) volumes; per-axis flips
 * from flips_host (uint8[count], bit0=z bit1=y bit2=x).  monai_unet.py:193-217. */
int segmi_crop_patches(const segmi_act* image, const float* label, const int32_t* starts_host,
                       const uint8_t* flips_host, int count, int dst_dtype,
                       const segmi_act* out_image, float* out_label, void* stream);
/* The same sampler with the spatial augmentation of monai_unet.py:181-191 (RandRotated about the
 * three axes, RandZoomd keep_size) composed into the gather: a patch voxel goes (flip, crop origin)
 * -> index in the augmented volume -> index_map_host (12 doubles, row-major 3x4, (x,y,z,1) ->
 * continuous source index) -> image trilinear with border clamping, label nearest; positions
 * outside the augmented volume's extent (the SpatialPadd region) are 0. */
int segmi_warp_crop_patches(const segmi_act* image, const float* label, const int32_t* starts_host,
                            const uint8_t* flips_host, int count, const double* index_map_host,
                            int dst_dtype, const segmi_act* out_image, float* out_label,
                            void* stream);
/* segmi_warp_crop_patches with a smooth non-rigid deformation composed into the same gather (DESIGN.md
 * section 18).  The field lives in the index space of the augmented volume: a patch voxel goes (flip, crop
 * origin) -> integer augmented index a -> a' = a + u(a) -> index_map_host (as above; NULL = identity) ->
 * image trilinear with border clamping, label nearest; the SpatialPadd region is decided on the integer a
 * and written as 0.  u is a uniform cubic B-spline, tensor product over the three axes: `control` is a
 * DEVICE array of f32 displacements in voxels laid out [3][n0][n1][n2] (component and grid axes both in
 * (z, y, x) order).  For an axis of extent dim > 1: t = i (n - 3) / (dim - 1), k = min(floor(t), n - 4),
 * f = t - k, and the four uniform cubic B-spline basis functions of f weigh control points k .. k+3, so the
 * volume spans the n - 3 interior spans exactly.  An axis of extent 1 uses t = 0 and its displacement
 * component is 0.  4 <= n0, n1, n2 and n0 * n1 * n2 <= 4096 (the grid is staged in LDS, 48 KB at most):
 * SEGMI_EINVAL otherwise.  1..16 crops per call; allocates nothing and does not synchronise; the control array
 * must stay valid until the kernel has run on `stream`. */
int segmi_elastic_warp_crop_patches(const segmi_act* image, const float* label, const int32_t* starts_host,
                                    const uint8_t* flips_host, int count, const double* index_map_host,
                                    const float* control, int n0, int n1, int n2, int dst_dtype,
                                    const segmi_act* out_image, float* out_label, void* stream);
/* Intensity augmentation of monai_unet.py:205-208 on `count` dense f32 NDHWC patches
 * [count][rd][rh][rw][c], in place, in the reference's order: RandAdjustContrastd (gamma),
 * RandHistogramShiftd (nctrl floating control points in [0,1] per patch, ascending),
 * RandBiasFieldd (20 degree-3 Legendre coefficients per patch).  Each *_on_host (uint8[count],
 * nullable = skip the transform) selects the patches a transform applies to; the random draws
 * are the caller's.  workspace >= segmi_intensity_workspace(count) bytes. */
int64_t segmi_intensity_workspace(int count);
int segmi_intensity_augment(float* patches, int count, int rd, int rh, int rw, int c,
                            const uint8_t* contrast_on_host, const float* gamma_host,
                            const uint8_t* hist_on_host, const float* ctrl_host, int nctrl,
                            const uint8_t* bias_on_host, const float* coef_host, void* workspace,
                            void* stream);
/* k-space augmentation of monai_unet.py:209-210 on the same patch layout, channel-wise, in place:
 * RandGibbsNoised (spectrum outside radius (1-alpha)*max(shape)*sqrt(2)/2 of the centred k-space
 * zeroed) then RandKSpaceSpikeNoised (one bin at spike_loc_host int32[count][3] = (z,y,x) of the
 * centred k-space set to magnitude exp(2.5 * mean log|K| * (0.95 + 0.15 * spike_u)), phase kept).
 * flips_host (uint8[count], bit0=z bit1=y bit2=x; nullable = none): the patch was flipped BEFORE
 * this call while the reference flips after it (RandFlipd last): the Gibbs mask is evaluated at the
 * mirrored bin; spike_loc_host must already be mirrored by the caller.
 * 3-D DFT of any extents <= 512 (direct per-axis transform in LDS; only selected patches are
 * transformed).  workspace >= segmi_kspace_workspace(count, rd, rh, rw) bytes. */
int64_t segmi_kspace_workspace(int count, int rd, int rh, int rw);
int segmi_kspace_augment(float* patches, int count, int rd, int rh, int rw, int c,
                         const uint8_t* gibbs_on_host, const float* gibbs_alpha_host,
                         const uint8_t* spike_on_host, const int32_t* spike_loc_host,
                         const float* spike_u_host, const uint8_t* flips_host, void* workspace,
                         void* stream);
/* The `augment_degrade` training augmentation (not in the reference) on the same patch
 * layout [count][rd][rh][rw][c], in the order noise, blur, brightness, lowres; one draw per patch is shared by
 * its channels.  Each *_on_host (uint8[count], nullable = skip the transform) selects the patches of a transform;
 * the draws are the caller's.
 *   noise      : x[e] += sqrt(variance) * g(seed, e), e = ((z*rh + y)*rw + x)*c + ch the element index in its
 *                patch, seed_host uint32[count].  g is Box-Muller over a counter hash, k = 2e + j (j = 0, 1) in
 *                uint32 arithmetic: h = k*0x9E3779B1 ^ seed; h ^= h>>16; h *= 0x7feb352d; h ^= h>>15;
 *                h *= 0x846ca68b; h ^= h>>16; u1 = ((h_0>>8) + 1) 2^-24, u2 = (h_1>>8) 2^-24,
 *                g = sqrt(-2 ln u1) cos(2 pi u2).  variance_host >= 0.
 *   blur       : separable Gaussian over the spatial axes of extent > 1, sigma_host in voxels,
 *                R = floor(4 sigma + 0.5) <= 8, w_k = exp(-k^2 / (2 sigma^2)) normalised to sum 1 (computed here in
 *                double, used as f32), scipy's `reflect` border for any R, also R larger than the extent.
 *   brightness : x *= multiplier_host.
 *   lowres     : coarse_host int32[count][3] = the coarse extents m (z, y, x), 1 <= m <= extent.  Nearest
 *                down, linear up, as one gather: coarse sample j is the fine voxel src(j) = floor((2j+1) n / (2m));
 *                fine voxel i has t = clamp((i + 0.5) m/n - 0.5, 0, m-1), j0 = min(floor(t), max(m-2, 0)),
 *                f = t - j0 and the value (1-f) v[src(j0)] + f v[src(min(j0+1, m-1))] along that axis, tensor
 *                product over the axes.  An axis with m == n passes through; m == n on every axis leaves the
 *                patch's bits as they are.
 * Blur and lowres are out of place (patches <-> workspace); the noise is added where the first step loads, the
 * brightness multiplies where the last step stores; a patch with neither takes one in-place pass.  Only
 * selected patches are touched; nothing is launched when no flag is set.  1..16 patches per call, each of fewer
 * than 2^31 elements; lowres takes extents with rd + rh + rw <= 4096.  Allocates nothing and does not
 * synchronise.  workspace >= segmi_degrade_workspace(count, rd, rh, rw, c) bytes; it may be NULL only when no
 * patch is selected for blur or lowres.  SEGMI_EINVAL names what is out of range.  Non-finite inputs are not
 * supported. */
int64_t segmi_degrade_workspace(int count, int rd, int rh, int rw, int c);
int segmi_degrade_augment(float* patches, int count, int rd, int rh, int rw, int c,
                          const uint8_t* noise_on_host, const float* variance_host, const uint32_t* seed_host,
                          const uint8_t* blur_on_host, const float* sigma_host,
                          const uint8_t* bright_on_host, const float* multiplier_host,
                          const uint8_t* lowres_on_host, const int32_t* coarse_host, void* workspace,
                          void* stream);

/* ---------------------------------------------------------------- model ensembles ------ */
/* Combination of `models` (<= 16) predictions over n elements, monai_unet.py:848-1004.
 * *_host arguments are HOST arrays (of device pointers / scalars).
 *  mean  : MeanEnsembled with weights: out = mean_e(logits_e * w_e / mean(w)) (f32, n = K * voxels)
 *  vote  : VoteEnsembled on int32 label volumes: most frequent label, ties -> smallest label
 *  select: segmantic SelectBestEnsemble (seg/transforms.py:15-88): for each (tissue, model) pair in
 *          order, out[labels[model] == tissue] = tissue; unclaimed voxels are 0. */
int segmi_ensemble_mean(const float* const* logits_host, const float* weights_host, int models,
                        int64_t n, float* out, void* stream);
int segmi_ensemble_vote(const int32_t* const* labels_host, int models, int64_t n, int32_t* out,
                        void* stream);
int segmi_ensemble_select(const int32_t* const* labels_host, int models, const int32_t* tissue_host,
                          const int32_t* model_host, int pairs, int64_t n, int32_t* out,
                          void* stream);

/* ---------------------------------------------------------------- STAPLE label fusion --- */
/* Multi-label STAPLE (Warfield et al. 2004, as ITK's MultiLabelSTAPLEImageFilter) over `raters` (1 .. 16) label
 * volumes of n < 2^31 voxels each, read in place as label_bytes in {1 (uint8), 2 (int16), 4 (int32)}, labels in
 * 0 .. num_classes - 1 (2 .. 64 classes).  DESIGN.md section 22 is the definition: posteriors in fixed point
 * (Q = 2^24), integer sums S[r][l][s], theta = S / T in f64, the E-step in f64 operation by operation, so the
 * result is the same bits for every launch shape.  labels_host: HOST table of device pointers.  prior_host
 * (nullable): HOST f64[num_classes], positive and finite, used as given; NULL = label frequencies over all
 * raters.  Under a given prior so small that every product of a voxel's E-step rounds to 0, the voxel is dropped:
 * q = 0 for every label, nothing added to sums, posterior 0, label 0.  Outputs on the device: out (dtype of the inputs), sums i64 [raters][L][L] of the last M-step, prior
 * f64 [L], posterior (nullable) f32 [L][n] = q / Q of the last E-step.  info_host: HOST i32[4] = iterations,
 * converged, rater index of an input label outside 0 .. L-1 (-1: none) and that label's value; when such a
 * label exists it indexes no table, out and posterior are not written and the caller raises.  The stop flag
 * stays on the device; the host reads the state back once per 16 iterations (ceil(iterations / 16)
 * synchronisations per call, one more to fetch an offending label). */
int64_t segmi_staple_workspace_bytes(int raters, int num_classes);
/* "lds" when the per-workgroup S table of raters * L * L i64 fits the 48 KB LDS table, "global" when the
 * passes add into the global table directly; "" for shapes segmi_staple refuses.  segmi_staple launches by
 * the same choice. */
const char* segmi_staple_table_name(int raters, int num_classes);
int segmi_staple(const void* const* labels_host, int raters, int label_bytes, int64_t n, int num_classes,
                 const double* prior_host, int max_iterations, double tolerance, void* out, int64_t* sums,
                 double* prior, float* posterior, int32_t* info_host, void* workspace, size_t ws_bytes,
                 void* stream);

/* ---------------------------------------------------------------- patch-based label fusion ---------- */
/* Intensity-weighted fusion of `atlases` (1 .. 16) atlases on the grid of a target of [d][h][w] voxels, d*h*w < 2^31
 * (2-D: d == 1).  DESIGN.md section 25 is the definition: 8-bit intensities, integer patch distances, the weight a
 * lookup in a caller-supplied table, integer scores, so the result is the same bits for every launch shape.
 *
 * segmi_quantise_u8: dst[i] = clamp(floor((src[i] - (float)lo) * scale + 0.5f), 0, 255) in float32, every operation
 * rounded on its own, scale = (float)(255.0 / (hi - lo)); NaN gives 0.  lo < hi, both finite, scale finite.
 *
 * segmi_patch_fusion: target_q u8 [d][h][w]; atlas_q_host / atlas_labels_host: HOST tables of device pointers to the
 * quantised atlas images (u8) and the label maps (label_bytes in {1 (uint8), 2 (int16), 4 (int32)}, labels in
 * 0 .. num_classes - 1, 2 .. 64 classes).  patch_radius / search_radius: HOST i32[3] (z, y, x), each 0 .. 3; on an
 * axis of extent 1 both are taken as 0.  adaptive 1: den = max(smallest distance among the voxel's candidates,
 * npatch * h2); adaptive 0: den = npatch * h2; h2 in 1 .. 65025.  table: DEVICE u32[1024], entries above 65536 are
 * read as 65536.  Outputs on the device: out (dtype of the label maps), and the nullable best u32 [d][h][w] (the
 * winner's score), total u32 [d][h][w] (the sum of the scores) and scores u32 [num_classes][d][h][w].  info_host:
 * HOST i32[2] = atlas index of an input label outside 0 .. num_classes - 1 (-1: none; the first such voxel, then the
 * first atlas) and that label's value; when such a label exists no output is written and the caller raises.  One
 * synchronisation per call (one more to fetch an offending label). */
int segmi_quantise_u8(const float* src, int64_t n, double lo, double hi, uint8_t* dst, void* stream);
int64_t segmi_patch_fusion_workspace_bytes(int atlases, int num_classes);
/* "lds_scores_tile_8x8x8" when the score table of the classes fits next to the staged tiles of an 8 x 8 x 8 tile
 * (num_classes <= 18), "lds_scores_tile_2x8x8" above; "" for arguments segmi_patch_fusion refuses.
 * segmi_patch_fusion launches by the same choice. */
const char* segmi_patch_fusion_variant_name(int num_classes, const int32_t* patch_radius, const int32_t* search_radius);
int segmi_patch_fusion(const uint8_t* target_q, const void* const* atlas_q_host, const void* const* atlas_labels_host,
                       int atlases, int label_bytes, int d, int h, int w, int num_classes, const int32_t* patch_radius,
                       const int32_t* search_radius, int adaptive, int h2, const uint32_t* table, void* out,
                       uint32_t* best, uint32_t* total, uint32_t* scores, int32_t* info_host, void* workspace,
                       size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- registration ---------- */
/* Kernels of rigid / affine registration by mutual information (segmantic_amd/image/registration.py).  DESIGN.md
 * section 23 is the definition.  Volumes are [z][y][x]; `pixel` as in segmi_resample3d (0 f32, 1 u8, 2 i16,
 * 3 i32, 4 u16).
 *
 * Pyramid level: dst [sz/fz][sy/fy][sx/fx] f32 = mean of each fx * fy * fz block (tail samples dropped), the
 * block summed in f64 with x innermost and z outermost, divided by the count, rounded to f32.  Factors 1 .. 8.
 * Grid-stride under SEGMI_BIN_SHRINK_GRID_CAP workgroups of 256 (segmi_fixed_bins launches under the same cap). */
#define SEGMI_BIN_SHRINK_GRID_CAP 2048
int segmi_bin_shrink(int pixel, const void* src, int sx, int sy, int sz, int fx, int fy, int fz, float* dst,
                     void* stream);
/* out[e] = clamp(floor((image[e] - lo) * ((bins-1) / (hi-lo)) + 0.5), 0, bins-1) in f64, as u8; 255 ("ignore this
 * sample") where mask_mean (nullable, f32, same extent) is below 0.5.  bins in {16, 32, 64}; hi > lo. */
int segmi_fixed_bins(const float* image, const float* mask_mean, int64_t n, double lo, double hi, int bins,
                     uint8_t* out, void* stream);
/* Joint histograms out i64 [candidates][bins][bins] (fixed bin, moving bin) of 1 .. 32 candidates in one launch.
 * index_maps_host: HOST f64 [candidates][12], fixed index (x,y,z,1) -> continuous moving index (x,y,z).  A fixed
 * voxel with bin < bins counts for a candidate when 0 <= c <= n-1 on all three moving axes (no default value, no
 * border clamp); the moving value is the f64 trilinear interpolation of segmi_resample3d; b = clamp((val - mlo) *
 * mscale, 0, bins-1), i = min(floor(b), bins-2), q = floor((b - i) * 2^16 + 0.5); 2^16 - q goes to cell
 * (fixed bin, i) and q to (fixed bin, i+1), so sum / 2^16 is the number of samples that counted.  Fixed bins
 * of bins .. 254 are skipped as 255 is.  out is cleared by the call.
 * Launch shape: at most SEGMI_JOINT_HIST_GRID_CAP workgroups of 256 stride over the fixed voxels, times one grid
 * row per group of segmi_joint_histogram_group(bins) candidates (32 / 8 / 2 at 16 / 32 / 64 bins; 0 for any other
 * bins): a workgroup holds one 32-bit LDS table per candidate of its group, shared by its four waves, and flushes
 * it into out with device-scope integer atomics every 128 trips of its stride loop (at most 2^31 per counter). */
#define SEGMI_JOINT_HIST_GRID_CAP 1024
#define SEGMI_JOINT_HIST_MAX_CANDIDATES 32
int segmi_joint_histogram_group(int bins);
int segmi_joint_histogram(const uint8_t* fixed_bins, int fx, int fy, int fz, int pixel, const void* moving, int mx,
                          int my, int mz, const double* index_maps_host, int candidates, int bins, double mlo,
                          double mscale, int64_t* out, void* stream);

/* ---------------------------------------------------------------- deformable registration ---------- */
/* Kernels of B-spline free-form deformable registration (segmantic_amd/image/registration.py, csrc/deformable.hip).
 * DESIGN.md section 24 is the definition.  A control grid is DEVICE f64 [3][nz][ny][nx]: the displacement in mm
 * along the fixed image's array axes, components in (x, y, z) order.  segmi_ffd_grid says where a launch's voxels
 * sit in it: voxel j of an axis of the launch grid l is the full-resolution fixed index i = j f + 0.5 (f - 1) of an
 * image of extent d (l f <= d, f in 1 .. 8), and the grid of n >= 4 points spans [0, d - 1] with n - 3 spans:
 * t = (i (n - 3)) / (d - 1), k = min(floor(t), n - 4), cubic B-spline weights of t - k on points k .. k + 3 (an axis
 * of extent 1: t = 0 and a zero displacement component).  At most SEGMI_FFD_MAX_CONTROL_POINTS points in all.
 * index_map_host: HOST f64 [12], launch index (x,y,z,1) -> continuous moving index of the affine part;
 * r_host: HOST f64 [9], row-major, a millimetre of displacement -> moving index units.  `pixel` as segmi_resample3d. */
typedef struct {
  int32_t lx, ly, lz; /* the launch's voxel grid */
  int32_t dx, dy, dz; /* the full-resolution fixed extent */
  int32_t fx, fy, fz; /* pyramid factors of the launch grid */
  int32_t nx, ny, nz; /* control points */
} segmi_ffd_grid;
#define SEGMI_FFD_MAX_CONTROL_POINTS 32768
#define SEGMI_FFD_MAX_CANDIDATES 8
#define SEGMI_FFD_HIST_GRID_CAP 1024     /* workgroups of 256 striding over the voxels, per candidate group */
#define SEGMI_FFD_GRADIENT_GRID_CAP 8    /* workgroups of 256 striding over the batches of ONE control cell */
#define SEGMI_FFD_JACOBIAN_GRID_CAP 1024
#define SEGMI_FFD_WARP_GRID_CAP 1024
/* one sample adds at most 2^15 * 2^15 * 2^12 = 2^42 to an int64 gradient entry: 2^20 samples leave a bit to spare */
#define SEGMI_FFD_GRADIENT_MAX_SUPPORT 1048576
/* segmi_joint_histogram (same table, weights, inside test and LDS flush discipline) for 1 .. 8 candidate control
 * grids control [candidates][3][nz][ny][nx]: sample position c = index_map (x,y,z,1) + R u.  With all-zero grids the
 * table equals segmi_joint_histogram's of index_map bit for bit.  out i64 [candidates][bins][bins], cleared here. */
int segmi_ffd_joint_histogram(const uint8_t* fixed_bins, const segmi_ffd_grid* grid, const double* control,
                              int candidates, int pixel, const void* moving, int mx, int my, int mz,
                              const double* index_map_host, const double* r_host, int bins, double mlo, double mscale,
                              int64_t* out, void* stream);
/* Integer gradient of the metric by the control values, out i64 [3][nz][ny][nx] (cleared here).  qd: DEVICE i32
 * [bins][bins-1], |qd| <= 2^15.  Per counted sample whose bin coordinate b is not clamped (0 < b < bins-1):
 * qd[fixed bin][floor(b)] * G_a * Wq goes to component a of each of the 64 support points, G_a =
 * rint(clamp((sum_r g_r R[r][a]) * gscale, -1, 1) * 2^15) with g the derivative of the trilinear value by the moving
 * index, Wq = rint(((w_z w_y) w_x) * 2^12).  One workgroup per control cell and batch stride; one 64-bit atomic per
 * support point, component and workgroup.  Refuses a grid whose control point's support holds more than
 * SEGMI_FFD_GRADIENT_MAX_SUPPORT voxels of the launch grid. */
int segmi_ffd_gradient(const uint8_t* fixed_bins, const segmi_ffd_grid* grid, const double* control, int pixel,
                       const void* moving, int mx, int my, int mz, const double* index_map_host, const double* r_host,
                       int bins, double mlo, double mscale, double gscale, const int32_t* qd, int64_t* out,
                       void* stream);
/* det(I + du/ds) at every voxel of the launch grid, s in mm along the fixed array axes; inv_spacing_host: HOST f64
 * [3] = 1 / control spacing in mm (0 on an axis of extent 1).  folded: DEVICE i64 [1], voxels with det <= 0;
 * min_jacobian: DEVICE f64 [1]; det_map: nullable DEVICE f32 [lz][ly][lx]. */
int segmi_ffd_jacobian(const segmi_ffd_grid* grid, const double* control, const double* inv_spacing_host,
                       int64_t* folded, double* min_jacobian, float* det_map, void* stream);
/* Resample moving onto the full-resolution fixed grid (factors 1, l = d) through the transform: position as in
 * segmi_ffd_joint_histogram, then segmi_resample3d's inside test, linear (nearest = 0) or nearest (1, half up)
 * taps, default value and output cast.  dst (nullable): the moving pixel type, [dz][dy][dx].  displacement
 * (nullable): f32 [3][dz][dy][dx] = direction_host (HOST f64 [9], the fixed direction matrix) times u, in mm. */
int segmi_ffd_warp(const segmi_ffd_grid* grid, const double* control, int pixel, const void* moving, int mx, int my,
                   int mz, const double* index_map_host, const double* r_host, int nearest, double default_value,
                   void* dst, const double* direction_host, float* displacement, void* stream);

/* ---------------------------------------------------------------- evaluation ----------- */
/* Segmentation evaluation (src/segmantic/seg/evaluation.py:5-125 and scripts/evaluate_segmentations.py).
 * Label volumes are read in place as label_bytes in {1 (uint8), 2 (int16), 4 (int32)}, [d][h][w]
 * (a 2-D input is d = 1 with spatial_dims = 2).  Boxes are half-open (z0 z1 y0 y1 x0 x1).
 *
 * Per-label bounding box of pred==c OR truth==c and the two voxel counts, in one pass over both
 * volumes (k <= 1024; an absent label gets the empty box 0 0 0 0 0 0).  Replaces the full-volume
 * SimpleITK filters of evaluation.py:18-26: every voxel outside the box is background of both
 * masks, so distance maps over the box are exact. */
int segmi_label_boxes(const void* pred, const void* truth, int label_bytes, int d, int h, int w, int k,
                      int32_t* boxes /* [k][6] */, int64_t* counts /* [k][2] pred, truth */, void* stream);
/* Workspace of segmi_edt_sq / segmi_edt_sample for a box of bd x bh x bw voxels. */
int64_t segmi_edt_workspace_bytes(int bd, int bh, int bw);
/* Exact squared Euclidean distance (physical, spacing per array axis z y x) from every voxel of the box
 * to the nearest feature voxel of `label`: feature 0 = labels == label, 1 = its contour (voxels of the
 * label with a face neighbour -- 6 in 3-D, 4 in 2-D -- that is not, outside the volume = background).
 * dist_sq: f32 [bd][bw][bh] (x before y: the layout of the last pass); +inf when the box holds no
 * feature.  The contour map is signed as SignedMaurerDistanceMap(insideIsPositive=False): voxels of
 * the label carry the sign bit.  Unit spacing is bit-exact.  box and spacing_zyx are HOST arrays.
 * Replaces sitk.BinaryContour + sitk.SignedMaurerDistanceMap, evaluation.py:18-26,61-66. */
int segmi_edt_sq(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int label,
                 int feature, const int32_t* box, const float* spacing_zyx, float* dist_sq, void* workspace,
                 size_t ws_bytes, void* stream);
/* Distances of the query voxels (query 0 = labels == label, 1 = its contour, inside the box) on a
 * distance map of segmi_edt_sq: a contour query takes |dist_sq|, a foreground query clamps dist_sq <= 0
 * (inside the target) to 0.  stats f64[4] = count, sum, sum of squares, max of the distances,
 * finalised inside the launch in a fixed order (repeated calls are bit-identical).  values (nullable):
 * the squared distances are appended at values[*n_values ...] and *n_values (device) advanced; their
 * order varies between runs, the caller zeroes the counter and sizes values for every query voxel.
 * Replaces the masking and numpy statistics of evaluation.py:28-47,71-92. */
int segmi_edt_sample(const float* dist_sq, const void* labels, int label_bytes, int d, int h, int w,
                     int spatial_dims, int label, int query, const int32_t* box, double* stats, float* values,
                     int64_t* n_values, void* workspace, size_t ws_bytes, void* stream);
/* Exact order statistics of n (device) non-negative f32 values: out[i] = the value of rank ranks[i]
 * (device i64, clamped to [0, n-1]; NaN when n == 0), 1 <= n_ranks <= 4.  Radix select over the bit
 * patterns (11 + 11 + 10 bits); the passes keep their state on the device.
 * Replaces np.median of evaluation.py:44,88 and MONAI's percentile Hausdorff. */
int64_t segmi_select_workspace_bytes(int n_ranks);
int segmi_select_f32(const float* values, const int64_t* n, const int64_t* ranks, int n_ranks, float* out,
                     void* workspace, size_t ws_bytes, void* stream);
/* cm i64[k][k], cm[truth][pred] voxel counts (k <= 4096; labels outside [0, k) are not counted).
 * Replaces confusion_matrix, evaluation.py:96-125. */
int segmi_confusion_counts(const void* pred, const void* truth, int label_bytes, int64_t n, int k,
                           int64_t* cm, void* stream);


/* ---------------------------------------------------------------- label clean-up ------- */
/* Connected components of a label map and the clean-up transforms built on them (MONAI's
 * KeepLargestConnectedComponent / RemoveSmallObjects / FillHoles, which are CPU loops over classes), plus
 * MapLabels of src/segmantic/seg/transforms.py:91-127.  Label volumes are read in place as label_bytes in
 * {1 (uint8), 2 (int16), 4 (int32)}, [d][h][w] (a 2-D input is d = 1 with spatial_dims = 2); n = d*h*w
 * must be < 2^31.  connectivity c in 1 .. spatial_dims: neighbours differ by at most 1 along every axis
 * and along at most c axes (scipy.ndimage.generate_binary_structure).  A component is a maximal set of
 * voxels of ONE value linked by neighbour steps; with_background = 0 leaves the voxels equal to 0 outside
 * every component, 1 labels the 0-regions too.  No function synchronises with the host.
 *
 * One workspace serves every function below. */
int64_t segmi_cc_workspace_bytes(int d, int h, int w);
/* root[v] = linear index of the first voxel (raster order z, y, x) of v's component, -1 for voxels outside
 * every component.  Union-find that links towards the smaller index, in three launches (tile-local in
 * LDS, tile seams, flatten); parent[v] <= v always holds and atomics only lower parents, so every loop
 * terminates without waiting for another workgroup and the result does not depend on scheduling. */
int segmi_cc_label(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int connectivity,
                   int with_background, int32_t* root /* [n] */, void* workspace, size_t ws_bytes, void* stream);
/* size[r] = voxel count of the component rooted at r, 0 at every other index. */
int segmi_cc_sizes(const int32_t* root, int64_t n, int32_t* size /* [n] */, void* stream);
/* comp[v] = canonical number 1 .. n_comp of v's component (numbered in raster order of the first voxels),
 * 0 outside; *n_comp (device) = the count.  Count / scan of partials / number / gather launches. */
int segmi_cc_compact(const int32_t* root, int64_t n, int32_t* comp /* [n] */, int32_t* n_comp, void* workspace,
                     size_t ws_bytes, void* stream);
/* Keep, per class, the num_components (1 .. 8) largest components, ordered by (size descending, first voxel
 * ascending); the other voxels of the class become 0.  applied_host: HOST list of the classes treated
 * (n_applied = 0: all), other classes are copied.  independent = 0: root / size come from the union mask of
 * the applied classes (root = -1 elsewhere) and the kept components keep their per-voxel class.  Classes
 * index a table of 256 (uint8) or 65536 entries; values outside it are copied.  out: dtype of labels. */
int segmi_cc_keep_largest(const void* labels, int label_bytes, int64_t n, const int32_t* root, const int32_t* size,
                          const int32_t* applied_host, int n_applied, int independent, int num_components,
                          void* out, void* workspace, size_t ws_bytes, void* stream);
/* Voxels of components with size < min_size become 0. */
int segmi_cc_remove_small(const void* labels, int label_bytes, int64_t n, const int32_t* root, const int32_t* size,
                          int min_size, void* out, void* stream);
/* root: labelled with with_background = 1 under the same connectivity.  A 0-component with no voxel on the
 * array border whose neighbouring non-zero voxels all carry one value L is filled with L when L is applied
 * (n_applied = 0: every label).  Label values must lie in 0 .. 65535. */
int segmi_cc_fill_holes(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int connectivity,
                        const int32_t* root, const int32_t* applied_host, int n_applied, void* out, void* workspace,
                        size_t ws_bytes, void* stream);
/* out[i] = lut[in[i]] (lut: device i64 [lut_len]); in_bytes / out_bytes in {1 (uint8), 2 (int16), 4 (int32),
 * 8 (int64)}.  The caller guarantees 0 <= in[i] < lut_len; an index outside the table writes 0 and reads
 * nothing.  Replaces lookup[img] of transforms.py:104-107. */
int segmi_map_labels(const void* in, int in_bytes, int64_t n, const int64_t* lut, int lut_len, void* out,
                     int out_bytes, void* stream);

/* ---------------------------------------------------------------- label morphology ------ */
/* Exact Euclidean feature transform and label morphology by a physical radius.
 * Label volumes are read in place as label_bytes in {1 (uint8), 2 (int16), 4 (int32)}, [d][h][w] with
 * d * h * w < 2^31 (a 2-D input is d = 1 with spatial_dims = 2).  spacing_zyx: HOST f64[3], per array axis.
 * Squared distances are f64: with one spacing s for every axis (the z entry is ignored for a 2-D input)
 * double(dz^2 + dy^2 + dx^2) * (s * s), the sum in i64 (bit-exact); otherwise
 * ((sz dz)^2 + (sy dy)^2) + (sx dx)^2 formed product by product in this order, so mirrored offsets give
 * bit-identical values.
 *
 * Workspace of the feature transform for a box of bd x bh x bw voxels. */
int64_t segmi_feature_transform_workspace_bytes(int bd, int bh, int bw);
/* index[bd][bh][bw] (plain z y x layout over the box) = linear index (z * h + y) * w + x, in the full
 * volume, of the feature voxel of the box nearest to each voxel of the box; -1 when the box holds no feature.
 * Among equally near features the smallest linear index wins (z, then y, then x).  Feature predicate by
 * mode: 0 value != 0, 1 value == 0, 2 value == label, 3 value != label, 4 table[value] != 0 (table: DEVICE
 * bytes [65536]; values outside 0 .. 65535 are no features).  box: HOST half-open (z0 z1 y0 y1 x0 x1), NULL =
 * the whole volume; extents up to 2^20.  dist (nullable) f32 [bd][bh][bw]: the squared distance to that
 * feature rounded to f32, or with dist_sqrt != 0 the f32 rounding of its f64 square root; +inf when there is
 * no feature.  Three launches (x, y, z), no host synchronisation. */
int segmi_feature_transform(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int mode,
                            int label, const uint8_t* table, const int32_t* box, const double* spacing_zyx,
                            int32_t* index, float* dist, int dist_sqrt, void* workspace, size_t ws_bytes,
                            void* stream);
/* out[v] = labels[index[v]] where labels[v] == 0, index[v] >= 0 and the squared distance between v and
 * index[v] is <= double(radius) * double(radius) (radius = +inf: no limit); labels[v] elsewhere.  index:
 * whole-volume result of the feature transform.  out: dtype of labels, must not alias labels. */
int segmi_morph_gather(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims,
                       const int32_t* index, const double* spacing_zyx, double radius, void* out, void* stream);
/* Erosion select: out[v] = 0 for every voxel v of the box with labels[v] == label whose nearest feature
 * index[v - box] (box-shaped result of the feature transform over the same box, mode 3) lies within the
 * radius (squared distance <= radius * radius); other voxels of out are not written: the caller fills out
 * with a copy of labels first.  keep (nullable, dtype of labels): voxels with keep[v] != 0 are never
 * zeroed (closing keeps what was labelled before the dilation).  box: HOST, NULL = the whole volume. */
int segmi_morph_erode_select(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int label,
                             const int32_t* box, const int32_t* index, const double* spacing_zyx, double radius,
                             const void* keep, void* out, void* stream);
/* planes[a][v] = coordinate a of the voxel index[v] (a = z, y, x; y, x with spatial_dims = 2): the layout
 * of scipy's return_indices.  -1 in every plane where index[v] is -1.  planes: i32 [spatial_dims][d*h*w]. */
int segmi_morph_index_planes(const int32_t* index, int d, int h, int w, int spatial_dims, int32_t* planes,
                             void* stream);

/* ---------------------------------------------------------------- label surfaces -------- */
/* Discrete surface nets of the selected labels of a label volume (scripts/visualize_label_surfaces.py of the
 * reference, which uses VTK's discrete flying edges; DESIGN.md section 14 defines the output).  Label volumes
 * are read in place as label_bytes in {1, 2, 4}, [d][h][w], with (d+1)(h+1)(w+1) < 2^31.  selected: 1 .. 65535
 * label values in 1 .. 65535, strictly ascending.  Work is confined to every label's bounding box: the boxes
 * are computed on the device, read back by the caller (host synchronisation 1) and handed, as HOST arrays, to
 * workspace_bytes / count / emit, which must all see the same selected / boxes.  No function synchronises.
 *
 * boxes i32 [n_sel][6] (device): half-open z0 z1 y0 y1 x0 x1 of labels == selected[l]; absent: 0 0 0 0 0 0. */
int segmi_surface_boxes(const void* labels, int label_bytes, int d, int h, int w, const int32_t* selected /* device */,
                        int n_sel, int32_t* boxes, void* stream);
/* 0 when the arguments are invalid or the boxes hold 2^31 chunks (64 cells along x) or more */
int64_t segmi_surface_workspace_bytes(int d, int h, int w, const int32_t* selected_host, const int32_t* boxes_host,
                                      int n_sel);
/* Classify the cells of every label box and scan the per-chunk vertex / face counts into the workspace.
 * starts i32 [n_sel + 2][2] (device): (first vertex, first face) of every label in the concatenated outputs,
 * then the totals (V, F), then (overflow flag, 0): the flag is 1, and the totals 0, when V or F passed
 * 2^31 - 1.  Reading starts is host synchronisation 2; it sizes the outputs of emit. */
int segmi_surface_count(const void* labels, int label_bytes, int d, int h, int w, const int32_t* selected_host,
                        const int32_t* boxes_host, int n_sel, int32_t* starts, void* workspace, size_t ws_bytes,
                        void* stream);
/* After count, on the same workspace.  offsets f32 [V][3]: cell-local vertex offsets (x, y, z) in [0, 1];
 * cells i32 [V][3]: the vertex's cell (x, y, z), index coordinate = (cell - 1) + offset; neighbours i32 [V][6]
 * (nullable): numbers, in the concatenated output, of the -x +x -y +y -z +z neighbours, -1 = none;
 * faces i32 [F][3], numbered within their label. */
int segmi_surface_emit(const void* labels, int label_bytes, int d, int h, int w, const int32_t* selected_host,
                       const int32_t* boxes_host, int n_sel, int64_t n_vertices, int64_t n_faces, float* offsets,
                       int32_t* cells, int32_t* neighbours, int32_t* faces, void* workspace, size_t ws_bytes,
                       void* stream);
/* `iterations` Jacobi sweeps o' = clamp(o + relaxation (m - o), 0, 1) over the offsets (ping-pong with scratch
 * f32 [V][3]; offsets is clobbered), then vertices f32 [V][3] (x, y, z) = origin + Direction (spacing o index),
 * evaluated in f64 and rounded once.  geometry_host: HOST f64 [15] = origin xyz, direction row-major, spacing xyz. */
int segmi_surface_relax(float* offsets, float* scratch, const int32_t* cells, const int32_t* neighbours,
                        int64_t n_vertices, int iterations, float relaxation, const double* geometry_host,
                        float* vertices, void* stream);
/* measures f64 [n_sel][2] (device) = (area, signed volume 1/6 sum p0 . (p1 x p2)) of every label's mesh, from the
 * vertices and faces as emitted; f64 sums in a fixed order (bit-identical on repeated calls).
 * workspace: n_sel * 32 * 2 doubles, rounded up to 256 bytes. */
int segmi_surface_measure(const float* vertices, const int32_t* faces, const int32_t* starts, int n_sel,
                          double* measures, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- mesh decimation -------- */
/* Round-based edge collapse over independent sets (DESIGN.md section 14 defines the output; the reference runs
 * vtkDecimatePro, whose output is not defined).  A batch of n_meshes meshes is concatenated: vertices f32 [V][3],
 * faces i32 [F][3] numbered within their mesh, starts i32 [n_meshes + 2][2] (device) in the layout of
 * segmi_surface_count.  1 <= V < 2^31, 1 <= 3 F < 2^31, every face index must lie inside its mesh (the caller
 * checks), and a mesh holds fewer than 2^23 vertices (the claim key keeps 23 bits for the vertex).  Inputs are
 * never written.  No function synchronises.  0 when the arguments are invalid. */
int64_t segmi_decimate_workspace_bytes(int64_t n_vertices, int64_t n_faces, int n_meshes);
/* Working copy of the faces, mesh of every vertex, live i32 [n_meshes] (device) = faces per mesh. */
int segmi_decimate_init(const int32_t* faces, const int32_t* starts, int n_meshes, int64_t n_vertices, int64_t n_faces,
                        int32_t* live, void* workspace, size_t ws_bytes, void* stream);
/* Round `round` (0, 1, ...; the quadrics are built in round 0) for every mesh with live > targets (device i32
 * [n_meshes]); live is updated.  Reading live is the caller's one device-to-host copy per round: it stops when
 * every mesh is at its target or did not change. */
int segmi_decimate_round(const float* vertices, const int32_t* starts, const int32_t* targets, int n_meshes,
                         int64_t n_vertices, int64_t n_faces, int round, int32_t* live, void* workspace, size_t ws_bytes,
                         void* stream);
/* out_starts i32 [n_meshes + 2][2] (device): starts of the live vertices / faces, the totals, (0, 0). */
int segmi_decimate_compact_count(const int32_t* starts, int n_meshes, int64_t n_vertices, int64_t n_faces,
                                 int32_t* out_starts, void* workspace, size_t ws_bytes, void* stream);
/* After compact_count: live vertices (bit copies) and faces in their original relative order, renumbered within
 * their mesh; out_kept i32 [V']: the input number, within its mesh, of every output vertex. */
int segmi_decimate_compact_emit(const float* vertices, const int32_t* starts, int n_meshes, int64_t n_vertices,
                                int64_t n_faces, float* out_vertices, int32_t* out_faces, int32_t* out_kept,
                                void* workspace, size_t ws_bytes, void* stream);


/* ---------------------------------------------------------------- Nyul standardisation -- */
/* Nyul-Udupa histogram standardisation, src/segmantic/seg/nyul_normalize.py.  x: contiguous f32
 * [segments][seg_len] (one segment per channel, or the whole tensor as one); mask = x != 0 when
 * nonzero, else every value.  2 <= n_quantiles <= 64.
 * Landmarks of each segment: quantiles_host (HOST f64, sorted, in [0, 1]) of the masked values by
 * linear interpolation between exact order statistics (-0.0 == +0.0), out landmarks f32 [segments]
 * [n_quantiles] and counts i64 [segments] (masked values, NaN included).  Ranks and lerp follow
 * torch.quantile's f32 arithmetic for counts <= 2^24 and numpy.quantile's f64 arithmetic above; a
 * segment holding a masked NaN, or none, gets NaN landmarks.  Segmented, masked, multi-rank radix
 * select (11 + 11 + 10 bits) with its state in the workspace: no host round trip.
 * Replaces torch.quantile(img[mask], quantiles) of nyul_normalize.py:66-68. */
int64_t segmi_nyul_workspace_bytes(int segments, int n_quantiles);
int segmi_nyul_landmarks(const float* x, int segments, int64_t seg_len, int nonzero,
                         const double* quantiles_host, int n_quantiles, float* landmarks, int64_t* counts,
                         void* workspace, size_t ws_bytes, void* stream);
/* In place, every masked value of a segment whose counts entry is non-zero (counts nullable = all):
 * y = m[i]*x + b[i], i = clip(#{landmarks < x} - 1, 0, L-2), m[i] = (s[i+1]-s[i]) / (xp[i+1]-xp[i]),
 * b[i] = s[i] - m[i]*xp[i] in f32, each operation rounded (no FMA); standard_scale_host HOST f32 [L].
 * Duplicate landmarks give the reference's Inf / NaN.  Replaces interp1d + img[mask] = ... of
 * nyul_normalize.py:28-43,70. */
int segmi_nyul_apply(float* x, int segments, int64_t seg_len, int nonzero, const float* landmarks,
                     const int64_t* counts, const float* standard_scale_host, int n_quantiles, void* stream);

/* ---------------------------------------------------------------- vertebra landmarks -- */
/* Landmark transforms of src/segmantic/detect/transforms.py.  Volumes are [C][d][h][w] = [C][z][y][x];
 * points and boxes are reported in (x, y, z) order, as the reference's MONAI arrays [C][x][y][z] give them.
 * Per-label centroid sums of a label volume (uint8 / int16 / int32 by label_bytes) in one read:
 * sums i64 [k + 1][4] = (count, sum x, sum y, sum z) of labels 0 .. k (k <= 255); *flag (device i32) is
 * set when a label lies outside [0, k].  Both are zeroed by the call.  Exact integer sums.
 * Replaces the per-label torch.where + np.average of VertHeatMap, transforms.py:264-272. */
int segmi_label_centroids(const void* labels, int label_bytes, int d, int h, int w, int k, int64_t* sums,
                          int32_t* flag, void* stream);
/* The vertebra heatmap out f32 [k + 1][d][h][w], written once, in closed form from the centroid sums and
 * flag of segmi_label_centroids (read on the device: no host round trip).  params: device i32 words
 * [0] = k, [1] = table stride S, [2] = gamma (f32 bits), [3] = 0, [4 + L] = tail t_L of label L (256
 * words), then f32 tables [k + 1][S] from word 260: row L holds MONAI's gaussian_1d(sigma_L, 4.0, "erf")
 * at -t_L .. t_L.  Channel L of a present label: centre c = floor(mean index), P = k_L[z - c_z] *
 * k_L[y - c_y] * (smooth_3d ? k_L[x - c_x] : x == c_x) on the clipped support, then (P - min P) /
 * (max P - min P) * gamma with min / max over the channel; channel 0, absent labels, constant channels
 * and every channel when the flag is set are 0.
 * Replaces the one-hot + GaussianSmooth + ScaleIntensity loop of VertHeatMap, transforms.py:256-281. */
int segmi_vert_heatmap(const int32_t* params, int k, const int64_t* sums, const int32_t* flag, int d, int h,
                       int w, int smooth_3d, float* out, void* stream);
/* Per channel of x f32 [c][d][h][w] (d h w < 2^32): keys u64 [c] = orderable(max) << 32 | (0xFFFFFFFF -
 * ((x h + y) d + z)) of the first maximum in (x, y, z) lexicographic order (-0.0 == +0.0; 0 when the
 * channel holds only NaN); nan i32 [c] = 1 when the channel holds a NaN.  Both are zeroed by the call.
 * Replaces the numpy max + np.where(== max) of ExtractVertPosition, transforms.py:198-202. */
int segmi_channel_argmax(const float* x, int c, int d, int h, int w, uint64_t* keys, int32_t* nan,
                         void* stream);
/* Half-open box of the voxels > 0 in any channel of x [c][d][h][w] (f32 when is_float, else uint8 /
 * int16 / int32 by dtype_bytes): box i32 [6] = (x0, y0, z0, x1, y1, z1); NaN and -0.0 are not positive;
 * no positive voxel gives six zeros.
 * Replaces generate_spatial_bounding_box of BoundingBoxd, transforms.py:231. */
int segmi_positive_bbox(const void* x, int dtype_bytes, int is_float, int c, int d, int h, int w, int32_t* box,
                        void* stream);

/* ---------------------------------------------------------------- MRI / CT preprocessing -- */
/* src/segmantic/image/modality.py: N4 bias-field correction, its Otsu mask and shrink, and the CT
 * median / clamp / scale.  Volumes are contiguous [nz][ny][nx] (2-D: nz = 1).
 * Otsu: bins equal bins over [min, max] of the finite values of x (n values), bin = min(floor((v - min) / w),
 * bins - 1); counts i64 [bins] (nullable) and stats f64 [4] = {min, w, threshold, finite count}, both device;
 * threshold = min + (k + 1) w for the first k maximising the between-class variance.  2 <= bins <= 512. */
int64_t segmi_otsu_workspace_bytes(int bins);
int segmi_otsu(const float* x, int64_t n, int bins, int64_t* counts, double* stats, void* workspace,
               size_t ws_bytes, void* stream);
/* One gather: output voxel j of each axis takes input voxel j f + o, ns = max(1, n / f), o = floor(((n - 1) -
 * (ns - 1) f) / 2 + 0.5).  Mask: mask (u8, nullable) at that voxel, else outside / inside by v > otsu_stats[2]
 * (nullable: every voxel is 1).  Outputs (each nullable): the shrunk image, the shrunk mask, and
 * log(v) where mask == 1, v > 0 and v finite, NaN elsewhere (the N4 fit set, f64). */
int segmi_n4_shrink(const float* x, int nz, int ny, int nx, int fz, int fy, int fx, const uint8_t* mask,
                    const double* otsu_stats, int inside, int outside, float* out_img, uint8_t* out_mask,
                    double* out_log, void* stream);
/* N4 on a grid of log values (NaN: not in the fit set): levels fitting levels of (control_points - 3) 2^l
 * spans per axis of size > 1, iterations_host[l] iterations at most, stopping early when the CV of exp(old -
 * new field) is <= threshold.  Writes the final lattice f64 [Lz][Ly][Lx] (L = 1 on axes of size 1, else
 * (control_points - 3) 2^(levels-1) + 3), the field on the grid f64 (nullable), elapsed_host[levels] and
 * cv_host (HOST).  One 8-byte device-to-host read per iteration.  SEGMI_EDATA when the fit set has fewer
 * than 2 voxels or one log value. */
int64_t segmi_n4_workspace_bytes(int nz, int ny, int nx, int control_points, int levels, int bins);
int segmi_n4_fit(const double* logimg, int nz, int ny, int nx, const int* iterations_host, int levels,
                 int control_points, int bins, double fwhm, double noise, double threshold, double* lattice,
                 double* field, int* elapsed_host, double* cv_host, void* workspace, size_t ws_bytes, void* stream);
/* One sharpening of the finite values of u: E f64 [bins] and each value's sharpened value (NaN elsewhere).
 * Workspace: segmi_n4_workspace_bytes(nz, ny, nx, 4, 1, bins). */
int segmi_n4_sharpen(const double* u, int nz, int ny, int nx, int bins, double fwhm, double noise, double* E,
                     double* sharpened, void* workspace, size_t ws_bytes, void* stream);
/* One B-spline BA fit of the finite values of r at `spans` spans per axis into lattice (overwritten).
 * Workspace: segmi_n4_workspace_bytes(nz, ny, nx, spans + 3, 1, 2). */
int segmi_n4_bspline_fit(const double* r, int nz, int ny, int nx, int spans, double* lattice, void* workspace,
                         size_t ws_bytes, void* stream);
/* Exact cubic subdivision of a lattice: each axis of L > 1 control points becomes 2 (L - 3) + 3. */
int segmi_n4_refine(const double* coarse, int lz, int ly, int lx, double* fine, void* stream);
/* The lattice's field over an nz x ny x nx index range (u = i / (N - 1) m per axis), f32: out = x / exp(field)
 * when x is given, else the field. */
int segmi_n4_evaluate(const double* lattice, int lz, int ly, int lx, const float* x, float* out, int nz, int ny,
                      int nx, void* stream);
/* scale_clamp_ct: radius-1 median with replicate borders, clamp to [-1100, 3100], (v + 1100) * fl(255 / 4200) in f32
 * with each operation rounded.  out must not alias x. */
int segmi_ct_scale(const float* x, int nz, int ny, int nx, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGMI_H_ */
