/*
 * fdsr.h -- C ABI of libfdsr_hip.so, the MI355X (gfx950) engine behind the
 * FastDiffSR 20-step sampling path.
 *
 * The reference (Meng-333/FastDiffSR) is pure Python and has no FFI of its
 * own; the drop-in boundary is the duck-typed netG surface that
 * FastDiffSR/model/model.py (class DDPM) calls.  Each entry point below names
 * the reference interface it stands behind (file:line under
 * /root/reference/FastDiffSR/).  The Python facade in fastdiffsr_amd/
 * (diffusion.py, unet.py) binds these with ctypes and re-exposes the
 * reference's class/method names; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success or a negative FDSR_E_* code; nothing
 *    throws across the ABI; fdsr_last_error() gives the message.
 *  - tensors at the boundary are fp32, NCHW, contiguous, DEVICE pointers
 *    (the layout the reference's tensors have, LRHR_dataset.py:113-119);
 *    weights are handed over as HOST pointers in the reference checkpoint
 *    layout (Conv2d [Cout,Cin,kh,kw], Linear [out,in]) and repacked inside.
 *  - the caller owns every tensor and the workspace; the library owns its
 *    packed weights and captured graphs.  One handle per device; a handle is
 *    not thread-safe.  All work is stream-ordered on `stream` and asynchronous:
 *    the execution entry points do not synchronise the device, with one exception: the first
 *    fdsr_sample after the weights or the schedule changed builds the noise-embedding table for
 *    all T levels (one small launch + a stream synchronise).  Loading weights, fdsr_set_schedule
 *    and fdsr_set_seed are host-synchronous copies.
 *  - H and W must be multiples of 2^(n_mults-1) (three stride-2 stages => 8).
 */
#ifndef FDSR_H_
#define FDSR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDSR_OK 0
#define FDSR_E_INVALID (-1)   /* bad argument / unsupported configuration  */
#define FDSR_E_KEY (-2)       /* unknown checkpoint key or shape mismatch  */
#define FDSR_E_STATE (-3)     /* weights / schedule missing                */
#define FDSR_E_WORKSPACE (-4) /* workspace too small or misaligned         */
#define FDSR_E_HIP (-5)       /* HIP runtime error (see fdsr_last_error)   */
#define FDSR_E_SATURATED (-6) /* f16x3: a raw conv input left the f16 range (fdsr_check_saturation) */

#define FDSR_MAX_MULTS 8

typedef struct fdsr_engine* fdsr_handle;

/* Hyper-parameters of unet.UNet(...) exactly as networks.define_G passes them
 * (model/networks.py:94-104; ctor model/fastdiffsr_modules/unet.py:224-297). */
typedef struct fdsr_config {
  int32_t in_channel;    /* 6 = cat(cond SR image, x_t)                    */
  int32_t out_channel;   /* 3                                              */
  int32_t inner_channel; /* 64                                             */
  int32_t norm_groups;   /* 32                                             */
  int32_t n_mults;
  int32_t channel_mults[FDSR_MAX_MULTS]; /* {1,2,4,4}                      */
  int32_t res_blocks;    /* 2                                              */
  float dropout;         /* 0.2; identity in eval (sampling) mode          */
  int32_t image_size;    /* FastDiffSR: informational.  SR3 variant: attention is placed where the
                            resolution (image_size halved per level) is in attn_res (ddpm_modules/unet.py:183) */
  int32_t variant;       /* FDSR_VARIANT_FASTDIFFSR (model/fastdiffsr_modules), _SR3 (model/ddpm_modules) or _TESR (model/tesr_modules) */
  int32_t n_attn_res;
  int32_t attn_res[FDSR_MAX_MULTS];
} fdsr_config;
#define FDSR_VARIANT_FASTDIFFSR 0
#define FDSR_VARIANT_SR3 1
#define FDSR_VARIANT_GDP 3   /* model/gdp_modules: the guided-diffusion UNet (scale-shift-norm ResBlocks, up/down ResBlocks, multi-head attention); inner_channel = model_channels, attn_res = attention_resolutions (downsample rates); predicts x_0; input cat[x, cond] */
#define FDSR_VARIANT_TESR 2  /* model/tesr_modules: FastDiffSR's blocks and noise-level embedding, SR3's SelfAttention placement, sampler returns x_0 */

/* Per-timestep scalars the reverse process reads (diffusion.py:109-155; only
 * these five buffers + the fp64 sqrt_alphas_cumprod_prev list are used by
 * p_sample, :157-190).  All arrays have n_timestep entries, index = t. */
typedef struct fdsr_schedule {
  int32_t n_timestep;
  const float* noise_level;      /* fp32(sqrt_alphas_cumprod_prev[t+1])  :169-170 */
  const float* sqrt_recip;       /* sqrt_recip_alphas_cumprod[t]         :157-159 */
  const float* sqrt_recipm1;     /* sqrt_recipm1_alphas_cumprod[t]                 */
  const float* coef1;            /* posterior_mean_coef1[t]              :161-165 */
  const float* coef2;            /* posterior_mean_coef2[t]                        */
  const float* sigma;            /* exp(0.5*posterior_log_variance_clipped[t]) :190 */
} fdsr_schedule;

/* -- lifetime ------------------------------------------------------------ */
/* unet.UNet.__init__ + GaussianDiffusion.__init__ (unet.py:224, diffusion.py:78). */
int fdsr_create(const fdsr_config* cfg, fdsr_handle* out);
void fdsr_destroy(fdsr_handle h);
/* Message of the last failing call on this handle (or the global one if h==NULL). */
const char* fdsr_last_error(fdsr_handle h);
/* "gfx950 f32-mfma ..." build string. */
const char* fdsr_version(void);

/* -- checkpoint schema: nn.Module.state_dict()/load_state_dict (model.py:135,159) */
int fdsr_num_weights(fdsr_handle h);
/* idx-th tensor of the UNet schema (keys without the 'denoise_fn.' prefix), in
 * state_dict order.  live=0 for the 22 never-executed `<blk>.conv` layers
 * (unet.py:212) that exist only in checkpoints. */
int fdsr_weight_info(fdsr_handle h, int idx, char* key, int key_cap,
                     int64_t shape[4], int* ndim, int* live);
/* Hand over one checkpoint tensor (host pointer, reference layout). */
int fdsr_load_weight(fdsr_handle h, const char* key, const float* host,
                     const int64_t* shape, int ndim);
/* 1 when every live tensor has been loaded. */
int fdsr_weights_complete(fdsr_handle h);

/* GaussianDiffusion.set_new_noise_schedule (diffusion.py:109-155). */
int fdsr_set_schedule(fdsr_handle h, const fdsr_schedule* s);

/* -- execution ------------------------------------------------------------ */
/* Bytes of device scratch fdsr_unet_forward / fdsr_sample need for this shape. */
int fdsr_workspace_bytes(fdsr_handle h, int batch, int height, int width, size_t* bytes);

/* UNet.forward(x, noise_level) (unet.py:299-323), eval mode.
 *   x_nchw      [B,in_channel,H,W]   noise_level [B]   eps_nchw [B,out_channel,H,W] */
int fdsr_unet_forward(fdsr_handle h, const float* x_nchw, const float* noise_level,
                      float* eps_nchw, int batch, int height, int width,
                      void* workspace, size_t workspace_bytes, void* hip_stream);

/* SR3 variant: same entry point; noise is [T+1,B,3,H,W] (a draw exists for t = 0 too and is masked, ddpm_modules/
 * diffusion.py:189-196), the network sees the integer time, and out is x_0 itself (no res2img, :226-227).
 *
 * GaussianDiffusion.p_sample_loop, conditional branch (diffusion.py:192-221),
 * batched as B independent B=1 runs (the reference crashes for B>=2, :215-216).
 *   cond_nchw [B,3,H,W]        the bicubic-upsampled LR image (x_in)
 *   noise     [T,B,3,H,W]      noise[0] = x_T (`randn(shape)` :207), noise[k] =
 *                              the `randn_like` of step t = T-k (:189), k=1..T-1;
 *                              or NULL: the engine draws the same planes itself inside the
 *                              loop (Philox4x32-10 + Box-Muller keyed by fdsr_set_seed and a
 *                              per-call counter, see fdsr_set_seed) -- the throughput mode; parity runs pass noise
 *   out_nchw  [B,3,H,W]        res2img(x_0, cond) (:214, :275-281) == ret_img[-1]
 *   traj_nchw [T,B,3,H,W] or NULL: x_t after every step (t = T-1..0), for
 *                              continous=True frames and parity tests.
 * flags: FDSR_SAMPLE_GRAPH replays the 20-step loop as one captured hipGraph; hip_stream must then be a
 *        created stream (capture cannot run on the NULL stream: FDSR_E_INVALID). */
#define FDSR_SAMPLE_GRAPH 1
int fdsr_sample(fdsr_handle h, const float* cond_nchw, const float* noise,
                float* out_nchw, float* traj_nchw, int batch, int height, int width,
                void* workspace, size_t workspace_bytes, void* hip_stream, int flags);

/* Long schedules (the siblings' own T = 1000 / 2000): fdsr_sample with the per-step inputs on the device.
 * A small step-prologue kernel before every step reads a step counter held by the handle, copies the
 * noise-embedding row and the posterior scalars of t = T-1-k into handle-owned buffers and advances the
 * counter; so every step launches the same kernels with the same arguments.  Same arithmetic as
 * fdsr_sample: out and the frames it keeps are bitwise equal to fdsr_sample's.
 *   cond_nchw, noise, out_nchw  as fdsr_sample (the noise layout is unchanged: [T+1,...] for SR3 / GDP,
 *                              [T,...] otherwise, or NULL for the engine's own draws)
 *   traj_nchw [S,B,3,H,W] or NULL, S = ceil(T / traj_every) = the number of t in [0, T) with
 *                              t % traj_every == 0: x_t after those steps, t descending
 *                              (traj_every = 1 is fdsr_sample's full trajectory; the reference's
 *                              continous=True keeps traj_every = 1 | (T / 10))
 *   opts                       NULL = {0, 1}; chunk_steps: steps per captured graph (0: the library's
 *                              default, at most 32 and a divisor of T where one lies in [16, 32])
 * flags: FDSR_SAMPLE_GRAPH captures three graphs -- the prologue (input packing, counter reset), one chunk of
 *        chunk_steps steps and, when chunk_steps does not divide T, the remainder -- and replays the chunk
 *        T / chunk_steps times, so the graph size is O(chunk_steps), not O(T).  The cache rules are
 *        fdsr_sample's (key: pointers, shape and opts; at most 8 entries; dropped on a weight, schedule or
 *        precision change).  Refused (FDSR_E_INVALID) with live dropout (fdsr_set_training) and under the
 *        bf16_f16x3_steps debug option, whose precision depends on the step.
 * Memory: beyond the workspace (fdsr_workspace_bytes is unchanged) the handle keeps 5*T + TE floats and
 *        a few bytes of step state.  The step counter is handle state: calls on one handle must be ordered
 *        on one stream, which is the handle's contract anyway. */
typedef struct fdsr_sample_opts {
  int32_t chunk_steps;   /* 0: library default */
  int32_t traj_every;    /* >= 1 */
} fdsr_sample_opts;
int fdsr_sample_stepwise(fdsr_handle h, const float* cond_nchw, const float* noise,
                         float* out_nchw, float* traj_nchw, int batch, int height, int width,
                         void* workspace, size_t workspace_bytes, void* hip_stream, int flags,
                         const fdsr_sample_opts* opts);

/* Seed of the engine-side noise (resets the per-call counter): the same seed and call order give
 * the same images, whatever the batch split or launch geometry.  The reference draws from torch's
 * global generator (diffusion.py:189, :207); its stream is not reproduced, so parity is defined on
 * explicit noise only. */
/* The generator is Philox4x32-10 (Salmon et al., SC'11); 32-bit counter words (c0, c1, c2, c3) and key words (k0, k1):
 *   sampler noise, plane p      counter (i lo, i hi, p, calls lo)          key (seed lo, seed hi ^ calls hi)     i = n*H*W + pixel
 *   the same, tile-addressed    the same with i = (y0[n] + y)*scene_w + (x0[n] + x) and `calls` left as it stands (fdsr_set_noise_tiles)
 *   self-drawn training target  the first row with p = 0 (fdsr_train_grads_pairs, noise == NULL)
 *   dropout keep bytes          counter (quad lo, quad hi, slot, step)     key (seed lo ^ 0x44524F50, seed hi)   quad = NHWC element / 4
 * `calls` is zeroed by fdsr_set_seed; every fdsr_sample / fdsr_sample_stepwise that draws its own noise (a replayed graph too: the
 * counter lives on the device) and every training step that draws its own target adds one BEFORE drawing; fdsr_randn reads it.
 * Plane 0 is x_T, plane k + 1 the noise of step k.  `slot` is the index of the residual block in network order, `step` the count of
 * training-mode forwards since fdsr_set_seed / fdsr_set_dropout_seed (the first is 1); word e of quad q decides element 4q + e:
 * keep = word >= min(floor(p * 2^32), 2^32 - 1) with p the fp32 fdsr_config.dropout.
 * Normals: the uniform of an output word w is ((float)(w >> 8) + 0.5f) * 2^-24 in fp32, which lies in (0, 1] (the sum rounds to even
 * above 2^23: w >> 8 == 0xFFFFFF gives exactly 1, w >> 8 == 0 gives 2^-25); z0 = r0 cos(2 pi u1), z1 = r0 sin(2 pi u1),
 * z2 = r1 cos(2 pi u3), r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2) with logf / sqrtf / sincospif: finite everywhere, |z| <= 5.887,
 * within 7.7e-7 (measured; test bar 7.1e-6) of the fp64 evaluation on the same uniforms.
 * Both streams count positions of the GLOBAL batch: i and quad start at a shard's first image when the caller states it (debug option
 * "drop_image_offset"), for the dropout masks and for the self-drawn training target -- data-parallel ranks under one seed then draw
 * the slices of the single-process draw; without it every rank draws images [0, N).  fdsr_randn never applies the offset. */
int fdsr_set_seed(fdsr_handle h, uint64_t seed);
/* Plane `plane` ([B,3,H,W] fp32, device) of the noise drawn under the current call counter
 * (plane 0 = x_T, plane k = step t = T-k).  For tests of the generator. */
int fdsr_randn(fdsr_handle h, float* dst_nchw, int batch, int height, int width, int plane, void* hip_stream);
/* Tile-addressed noise: the images of a call are tiles of one scene, and the engine draws for each pixel the number the scene's
 * own noise field holds there -- without the field.
 *   origins_dev [n_tiles][2] int32 on the device, (y0, x0) of image i of a call in a scene `scene_w` pixels wide; NULL: off.
 * While a table is set, every normal that fdsr_sample / fdsr_sample_stepwise draw themselves (noise == NULL: x_T and the per-step
 * noise) and every fdsr_randn is addressed by the pixel's place in the scene,
 *   i = (y0[n] + y) * scene_w + (x0[n] + x)       (64-bit; image n, pixel (y, x) of the call)
 * in place of i = n*H*W + pixel of the table above; planes, key and `calls` are as there.  Such a sampling call does NOT add one to
 * `calls`: it draws under the counter as it stands, so after fdsr_set_seed every group of tiles draws under calls = 0, the value
 * under which fdsr_randn(h, dst, 1, SH, SW, p) with no table writes plane p of the whole scene's field.  The tile at (y0, x0)
 * therefore receives the crop [y0 : y0 + H, x0 : x0 + W] of that field bit for bit, and two tiles see the same numbers in the pixels
 * they share, whatever T and the scene's size.
 * The table is read when the kernels run, as the fdsr_scene_* tables are: keep it alive, and a captured graph stays valid while the
 * caller rewrites the same buffer between replays (the graph caches key on the pointer and scene_w, so setting or clearing a table
 * captures anew).  A call of more than n_tiles images is FDSR_E_INVALID: the kernels read entries [0, batch) and no others.
 * The origins address a counter, not memory: one outside the scene cannot fault, it only draws other numbers.
 * Not affected: an explicit `noise` array, the self-drawn training target (fdsr_train_grads_pairs), the dropout masks. */
int fdsr_set_noise_tiles(fdsr_handle h, const int32_t* origins_dev, int n_tiles, int scene_w);

/* Arithmetic of the convolutions (everything else is fp32 in every mode):
 *   FDSR_PREC_F32    exact fp32 on v_mfma_f32_32x32x2_f32 (default)
 *   FDSR_PREC_F16X3  fp32-grade: operands split hi/lo into two f16, three f16 MFMAs per product,
 *                    fp32 accumulate (stays inside the 1e-3 parity bound)
 *   FDSR_PREC_BF16   one bf16 MFMA per product and bf16 activations in HBM (BASELINE config 3; judged on
 *                    PSNR delta).  Needs 16-aligned channel counts (FDSR_E_INVALID otherwise); the SR3 / TESR / GDP variants
 *                    run their attention on bf16 MFMA kernels (fp32 scores and softmax). */
#define FDSR_PREC_F32 0
#define FDSR_PREC_F16X3 1
#define FDSR_PREC_BF16 2
/*   FDSR_PREC_F16    (round 6) one f16 MFMA per product -- the hi plane of the f16x3 weight forms against un-split f16 activations --
 *                    and f16 activations in HBM: the bf16 mode's bytes and MFMA rate with 11 mantissa bits instead of 8.  Stores
 *                    saturate at +-65504.  Judged on PSNR like bf16 (|delta| stays above 1e-3); every variant (the siblings' attention
 *                    kernels have f16 twins of their bf16 forms); sampling only. */
#define FDSR_PREC_F16 3
int fdsr_set_precision(fdsr_handle h, int mode);

/* -- val-loop helper ------------------------------------------ */
/* Metrics.tensor2img (core/metrics.py:16-42): clamp to [lo,hi], map to [0,1], *255, round half to
 * even, uint8.  src [B,C,H,W] fp32 device, dst [B,H,W,C] uint8 device; saves the fp32 D2H copy of
 * DDPM.get_current_visuals (model/model.py:97-111).  h may be NULL. */
int fdsr_tensor2img_u8(fdsr_handle h, const float* src_nchw, uint8_t* dst_nhwc, int batch, int channels,
                       int height, int width, float lo, float hi, void* hip_stream);

/* The per-image metric sums of the evaluation loop (sr_mfe.py:313-345: skimage.measure compare_mse / compare_psnr /
 * compare_ssim(multichannel=True) and Metrics.calculate_ergas, core/metrics.py:147-152; FDSR_SSIM_GAUSS11 adds the 11x11
 * Gaussian-window SSIM of core/metrics.py:103-145), on uint8 images that are already on the device -- the SR batch never
 * crosses PCIe as fp32 and the host does no per-pixel work.
 *   test / truth [B,H,W,C] uint8 device (C = 1..4);  out_dev [B][FDSR_METRIC_FIELDS] fp64 device:
 *     [0] sum (test - truth)^2      [1] sum test            -- exact integers
 *     [2] sum of the SSIM map, uniform 7x7 window (skimage defaults: sample covariance, K1 .01, K2 .03, L 255), interior
 *         positions of every channel                          [3] number of those positions
 *     [4], [5] the same for the 11x11 Gaussian window (sigma 1.5, "valid" part)      [6], [7] zero
 * The caller forms MSE = [0]/(H*W*C), PSNR, ERGAS = 100*sqrt(MSE / mean(test)^2 / C) / scale and SSIM = [2]/[3] with the
 * reference's scalar formulas (fastdiffsr_amd/metrics.py does).  Fixed-order reductions: reruns are bitwise identical.
 * h may be NULL. */
#define FDSR_METRIC_FIELDS 8
#define FDSR_SSIM_UNIFORM7 1
#define FDSR_SSIM_GAUSS11 2
int fdsr_image_metrics_workspace_bytes(int batch, int height, int width, size_t* bytes);
int fdsr_image_metrics_u8(fdsr_handle h, const uint8_t* test_nhwc, const uint8_t* truth_nhwc, int batch, int height,
                          int width, int channels, int flags, double* out_dev, void* workspace, size_t workspace_bytes,
                          void* hip_stream);

/* -- LPIPS, the fifth val metric (core/metrics.py:154-163 calculate_lpips: lpips.LPIPS(net='alex'), v0.1 heads) ----
 * An object of its own, independent of fdsr_handle: the torchvision AlexNet `features` convolutions and the five linear
 * heads, in fp32 on the device.  fdsr_lpips_load takes exactly these host fp32 tensors, in the checkpoint layouts:
 *   features.{0,3,6,8,10}.weight  [64,3,11,11] [192,64,5,5] [384,192,3,3] [256,384,3,3] [256,256,3,3]
 *   features.{0,3,6,8,10}.bias    [64] [192] [384] [256] [256]
 *   lin{0..4}.model.1.weight      [1,C,1,1], C = 64, 192, 384, 256, 256
 * Any other name or shape: FDSR_E_KEY.  Loading is a host-synchronous copy.
 * fdsr_lpips_u8 scores test_a (and test_b unless NULL) against truth, all [B,H,W,3] uint8 device images, as the reference
 * does: ToTensor() in [0,1] (NOT mapped to [-1,1]), ScalingLayer, AlexNet relu1..relu5, channel-normalised squared
 * differences weighted by the heads, spatial means.  The truth features are computed once for both tests.
 *   out_dev [n_tests][B][6] fp64 device: (LPIPS, then the five per-layer terms, retPerLayer).
 * Exact-fp32 MFMA convolutions, fp64 distances, fixed-order reductions: reruns are bitwise identical, an image's value does
 * not depend on B or its position in the batch, identical images give exactly 0.  H, W >= 32 (FDSR_E_INVALID below);
 * FDSR_E_STATE if any of the 15 tensors is missing; FDSR_E_WORKSPACE if the workspace (sized for two tests, 256-byte
 * aligned) is too small.  Stream-ordered, no implicit synchronisation.  Messages: fdsr_last_error(NULL). */
typedef struct fdsr_lpips_obj* fdsr_lpips;
int fdsr_lpips_create(fdsr_lpips* out);
int fdsr_lpips_load(fdsr_lpips l, const char* name, const float* host_f32, const int64_t* shape, int ndim);
int fdsr_lpips_workspace_bytes(fdsr_lpips l, int batch, int height, int width, size_t* bytes);
int fdsr_lpips_u8(fdsr_lpips l, const uint8_t* truth_nhwc, const uint8_t* test_a_nhwc, const uint8_t* test_b_nhwc_or_null,
                  int batch, int height, int width, double* out_dev, void* workspace, size_t workspace_bytes, void* hip_stream);
void fdsr_lpips_destroy(fdsr_lpips l);

/* -- FID features (FastDiffSR/FID.py: pytorch_fid.fid_score.calculate_fid_given_paths, dims=2048) -----------------
 * An object of its own: pytorch_fid's InceptionV3(output_blocks=[3], resize_input=True, normalize_input=True,
 * use_fid_inception=True) in fp32 on the device.  fdsr_fid_load takes the checkpoint's own tensors
 * (pt_inception-2015-12-05-6726825d.pth, torchvision names), host fp32:
 *   <module>.conv.weight [Cout,Cin,KH,KW]   <module>.bn.{weight,bias,running_mean,running_var} [Cout]
 * for the 94 BasicConv2d of the pool3 path (470 tensors; metrics.FID_TENSORS lists them).  fc.* and AuxLogits.* are not
 * taken: any other name or shape is FDSR_E_KEY.  When the last of a layer's five tensors arrives the library folds the
 * BN into the convolution in fp64 (w' = w g / sqrt(var + 1e-3), b' = beta - mean g / sqrt(var + 1e-3)) and rounds to fp32.
 * fdsr_fid_features_u8: [B,H,W,3] uint8 device images (any H, W >= 1: every size is resized to 299 x 299 as pytorch_fid
 * does, u8 / 255 -> bilinear -> 2x - 1) ->
 *   module = -1   out_dev [B][2048] fp32: the pool3 features
 *   module = k    out_dev: the raw NHWC fp32 output of module k, [B][S][S][C]:
 *                  k  module         S    C      k  module      S    C      k  module      S    C
 *                  0  Conv2d_1a_3x3  149   32    6  MaxPool_2   35  192   12  Mixed_6c   17  768
 *                  1  Conv2d_2a_3x3  147   32    7  Mixed_5b    35  256   13  Mixed_6d   17  768
 *                  2  Conv2d_2b_3x3  147   64    8  Mixed_5c    35  288   14  Mixed_6e   17  768
 *                  3  MaxPool_1       73   64    9  Mixed_5d    35  288   15  Mixed_7a    8 1280
 *                  4  Conv2d_3b_1x1   73   80   10  Mixed_6a    17  768   16  Mixed_7b    8 2048
 *                  5  Conv2d_4a_3x3   71  192   11  Mixed_6b    17  768   17  Mixed_7c    8 2048
 *   module = -2   out_dev [B][299][299][3]: the normalised network input (the resize stage)
 * Exact-fp32 MFMA convolutions (no split-K, no atomics), fixed-order pools: reruns are bitwise identical, an image's output
 * does not depend on B or on its position in the batch.  FDSR_E_INVALID for B < 1, H < 1, W < 1 or a module outside
 * [-2, 17]; FDSR_E_STATE if any of the 470 tensors is missing; FDSR_E_WORKSPACE if the workspace (256-byte aligned) is too
 * small.  Stream-ordered, no implicit synchronisation.  Messages: fdsr_last_error(NULL). */
typedef struct fdsr_fid_obj* fdsr_fid;
int fdsr_fid_create(fdsr_fid* out);
int fdsr_fid_load(fdsr_fid f, const char* name, const float* host_f32, const int64_t* shape, int ndim);
int fdsr_fid_workspace_bytes(fdsr_fid f, int batch, int height, int width, size_t* bytes);
int fdsr_fid_features_u8(fdsr_fid f, const uint8_t* img_nhwc, int batch, int height, int width, int module, float* out_dev,
                         void* workspace, size_t workspace_bytes, void* hip_stream);
void fdsr_fid_destroy(fdsr_fid f);

/* -- SwinIR (MSI_SR_model/model/swinir.py: GeneratorResNet) inference ---------------------------------------------------
 * An object of its own, independent of fdsr_handle: upsampler 'pixelshuffle', resi_connection '1conv', patch_size 1, no
 * absolute position embedding, three input channels, eval mode.  Exact fp32, NHWC inside: every Linear and every 3x3
 * convolution is one GEMM kernel on v_mfma_f32_32x32x2_f32 (a k-ordered chain per output, no split-K, no atomics), LayerNorm
 * over channels (eps 1e-5) one wave per token, shifted-window attention one workgroup per (image, window) with the roll, the
 * window partition, the relative-position bias and the -100 region mask folded in.  Reruns are bitwise identical and an
 * image's result depends neither on B nor on its position in the batch.
 *   fdsr_swinir_create           validates the configuration without touching the device.  FDSR_E_INVALID outside the envelope:
 *                                window_size 8; head_dim = embed_dim / num_heads[i] an integer <= 32; embed_dim <= 512;
 *                                1..FDSR_SWINIR_MAX_LAYERS layers of depth >= 1; upscale 2, 3, 4 or 8; img_range > 0.
 *   fdsr_swinir_load             a host fp32 tensor under the reference's state_dict name and shape (conv_first.weight,
 *                                layers.0.residual_group.blocks.1.attn.relative_position_bias_table, ...); the buffers
 *                                relative_position_index and attn_mask are functions of the geometry and are not taken.  Any
 *                                other name or shape: FDSR_E_KEY.  Host-synchronous; drops every captured graph.
 *   fdsr_swinir_workspace_bytes  for a batch of height x width inputs.  FDSR_E_INVALID where the input cannot be reflect-padded
 *                                to a multiple of the window (F.pad's rule: the padding is smaller than the side).
 *   fdsr_swinir_forward          x_nchw [B][3][H][W] fp32 in [0, 1] -> out_nchw [B][3][H upscale][W upscale].  flags:
 *                                FDSR_SWINIR_GRAPH replays the forward as one captured, linear hipGraph (hip_stream must be a
 *                                created stream); one graph is kept per (B, H, W), captured anew when x, out or the workspace
 *                                move.  Stream-ordered otherwise.
 *   fdsr_swinir_debug_tensor     runs the forward up to a named tap and copies it out as NHWC [B][dims3[0]][dims3[1]][dims3[2]] at
 *                                the padded size: conv_first, patch_embed.norm, layers.I.blocks.J.attn / .mlp (a block after its
 *                                attention / MLP residual), layers.I (an RSTB's output), conv_after_body, upsample.K (after the
 *                                K-th pixel shuffle).  Unknown name: FDSR_E_KEY; capacity_floats too small: FDSR_E_INVALID.
 *   fdsr_swinir_to_u8            the reference's save_img1: (x * 255) clamped to [0, 255], truncated; NCHW fp32 -> NHWC uint8.
 * FDSR_E_STATE if a tensor is missing; FDSR_E_WORKSPACE if the workspace (256-byte aligned) is too small.  Messages:
 * fdsr_last_error(NULL). */
#define FDSR_SWINIR_MAX_LAYERS 8
#define FDSR_SWINIR_GRAPH 1
typedef struct fdsr_swinir_config {
  int32_t embed_dim;
  int32_t n_layers;                          /* len(depths) == len(num_heads), 1..FDSR_SWINIR_MAX_LAYERS */
  int32_t depths[FDSR_SWINIR_MAX_LAYERS];
  int32_t num_heads[FDSR_SWINIR_MAX_LAYERS];
  int32_t window_size;
  int32_t mlp_hidden;                        /* int(embed_dim * mlp_ratio) */
  int32_t upscale;
  int32_t patch_norm;                        /* 0: no LayerNorm in patch_embed */
  float img_range;
  float mean[3];
} fdsr_swinir_config;
typedef struct fdsr_swinir_obj* fdsr_swinir;
int fdsr_swinir_create(const fdsr_swinir_config* cfg, fdsr_swinir* out);
int fdsr_swinir_load(fdsr_swinir s, const char* name, const float* host_f32, const int64_t* shape, int ndim);
int fdsr_swinir_workspace_bytes(fdsr_swinir s, int batch, int height, int width, size_t* bytes);
int fdsr_swinir_forward(fdsr_swinir s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                        size_t workspace_bytes, void* hip_stream, int flags);
int fdsr_swinir_debug_tensor(fdsr_swinir s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                             size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream);
int fdsr_swinir_to_u8(const float* src_nchw, uint8_t* dst_nhwc, int batch, int height, int width, void* hip_stream);
void fdsr_swinir_destroy(fdsr_swinir s);

/* -- HAT (MSI_SR_model/model/hat.py: GeneratorResNet) inference ------------------------------------------------------------
 * An object of its own, in the shape of fdsr_swinir: upsampler 'pixelshuffle', resi_connection '1conv', patch_size 1, no
 * absolute position embedding, three input channels, eval mode.  Exact fp32, NHWC inside, on the GEMM / LayerNorm kernels of
 * the SwinIR family plus: attention over 16 x 16 windows (256 keys, shift 8 and the -100 region mask on odd blocks) and the
 * overlapping cross-attention (256 queries against the 24 x 24 = 576 keys around the window, zero k and v outside the image),
 * one workgroup per (image, window, head, 32 queries) with the full score rows in LDS; the CAB's two 3x3 convolutions, its
 * channel-attention gate from fixed-order partial sums over the padded map, and conv_scale folded into proj's epilogue.
 * Reruns are bitwise identical and an image's result depends neither on B nor on its position in the batch.
 *   fdsr_hat_create           validates the configuration without touching the device.  FDSR_E_INVALID outside the envelope:
 *                             window_size 16; overlap_win_size 24 (overlap_ratio 0.5); head_dim = embed_dim / num_heads[i] an
 *                             integer <= 32; embed_dim <= 512, divisible by compress_ratio, embed_dim / squeeze_factor >= 1;
 *                             1..FDSR_HAT_MAX_LAYERS layers of depth >= 1; upscale 2, 3, 4 or 8; img_range > 0.
 *   fdsr_hat_load             a host fp32 tensor under the reference's state_dict name and shape.  The two
 *                             relative_position_index_* buffers are functions of the geometry and are not taken.  The
 *                             upsampler's one Conv2d is upsample.upsampling.0.*; the names .2.* and .4.* that the reference's
 *                             state_dict repeats it under load the same tensor.  Any other name or shape: FDSR_E_KEY.
 *                             Host-synchronous; drops every captured graph.
 *   fdsr_hat_workspace_bytes  for a batch of height x width inputs.  FDSR_E_INVALID where the input cannot be reflect-padded to a
 *                             multiple of 16 (F.pad's rule: the padding is smaller than the side).
 *   fdsr_hat_forward          x_nchw [B][3][H][W] fp32 in [0, 1] -> out_nchw [B][3][Hp upscale][Wp upscale], Hp / Wp = H / W
 *                             rounded up to a multiple of 16: the reference does not crop its output.  flags: FDSR_HAT_GRAPH
 *                             replays the forward as one captured, linear hipGraph (hip_stream must be a created stream); one
 *                             graph is kept per (B, H, W), captured anew when x, out or the workspace move.
 *   fdsr_hat_debug_tensor     runs the forward up to a named tap and copies it out as NHWC [B][dims3[0]][dims3[1]][dims3[2]] at
 *                             the padded size: SwinIR's taps plus layers.I.blocks.J.cab (the gated CAB output before
 *                             conv_scale), layers.I.ocab.attn (after proj + shortcut) and layers.I.ocab.mlp.
 * fdsr_swinir_to_u8 is save_img1 for this family too.  Errors as for fdsr_swinir. */
#define FDSR_HAT_MAX_LAYERS 8
#define FDSR_HAT_GRAPH 1
typedef struct fdsr_hat_config {
  int32_t embed_dim;
  int32_t n_layers;                          /* len(depths) == len(num_heads), 1..FDSR_HAT_MAX_LAYERS */
  int32_t depths[FDSR_HAT_MAX_LAYERS];
  int32_t num_heads[FDSR_HAT_MAX_LAYERS];
  int32_t window_size;
  int32_t mlp_hidden;                        /* int(embed_dim * mlp_ratio), in the HABs and the OCAB */
  int32_t upscale;
  int32_t patch_norm;                        /* 0: no LayerNorm in patch_embed */
  float img_range;
  float mean[3];
  int32_t compress_ratio;                    /* the CAB's hidden map has embed_dim / compress_ratio channels */
  int32_t squeeze_factor;                    /* the gate's hidden layer has embed_dim / squeeze_factor channels */
  float conv_scale;
  int32_t overlap_win_size;                  /* int(window_size * overlap_ratio) + window_size */
} fdsr_hat_config;
typedef struct fdsr_hat_obj* fdsr_hat;
int fdsr_hat_create(const fdsr_hat_config* cfg, fdsr_hat* out);
int fdsr_hat_load(fdsr_hat s, const char* name, const float* host_f32, const int64_t* shape, int ndim);
int fdsr_hat_workspace_bytes(fdsr_hat s, int batch, int height, int width, size_t* bytes);
int fdsr_hat_forward(fdsr_hat s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                     size_t workspace_bytes, void* hip_stream, int flags);
int fdsr_hat_debug_tensor(fdsr_hat s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                          size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream);
void fdsr_hat_destroy(fdsr_hat s);

/* -- TransENet (MSI_SR_model/model/transenet.py: TransENet; model/transformer.py) inference ------------------------------------
 * An object of its own, in the shape of fdsr_hat.  What the reference hard-codes is fixed here too: 8 x 8 patches, dim 512, 6
 * heads of 32, mlp_dim 512, reduction 4 (channels = n_feats / 4), the tanh form of GELU, the logit scale 512^-0.5, no dropout.
 * Exact fp32, NHWC inside, on the GEMM / LayerNorm kernels of the SwinIR family plus: dense attention over every token of the
 * image (self-attention at (H / 8)(W / 8) and at scale^2 times as many tokens, cross-attention of the high tokens against the
 * low ones), one workgroup per (image, head, 32 queries), k and v streamed in chunks of 128 keys whatever their number; the
 * patch rearrange as a gather of the token GEMM and its inverse as embedding_to_patch's store; sub_mean and add_mean as general
 * 3x3 matrices with bias.  Reruns are bitwise identical and an image's result depends neither on B nor on its position in the
 * batch.
 *   fdsr_transenet_create           validates the configuration without touching the device.  FDSR_E_INVALID outside the
 *                                   envelope: n_colors 3; n_feats a multiple of 16, 16..256; scale 2, 3, 4 or 8; en_depth and
 *                                   de_depth 1..FDSR_TRANSENET_MAX_DEPTH.
 *   fdsr_transenet_load             a host fp32 tensor under the reference's state_dict name and shape (sub_mean.weight [3][3][1][1],
 *                                   encoder_up.layers.3.0.fn.fn.to_qkv.weight [576][512], ...).  Any other name or shape:
 *                                   FDSR_E_KEY.  Host-synchronous; drops every captured graph.
 *   fdsr_transenet_workspace_bytes  for a batch of height x width inputs.  FDSR_E_INVALID unless both sides are multiples of 8.
 *   fdsr_transenet_forward          x_nchw [B][3][H][W] fp32 -> out_nchw [B][3][H scale][W scale].  The geometry is the input's:
 *                                   the reference's hr_patch_size binds the Python module, not the engine.  flags:
 *                                   FDSR_TRANSENET_GRAPH replays the forward as one captured, linear hipGraph (hip_stream must be a
 *                                   created stream); one graph is kept per (B, H, W), captured anew when x, out or the workspace move.
 *   fdsr_transenet_debug_tensor     runs the forward up to a named tap and copies it out as NHWC [B][dims3[0]][dims3[1]][dims3[2]];
 *                                   token tensors are [B][H / 8][W / 8][512] (times the scale for the high tokens).  Taps: head,
 *                                   stageI, stageI.1x1, up, up.1x1, embed.lowI, embed.high, ENC.J.attn, ENC.J.ff, ENC (ENC =
 *                                   encoder_stage1..3, encoder_up), decoderI.J.self / .cross / .ff, embedding_to_patch, span.
 * fdsr_swinir_to_u8 is save_img1 for this family too.  Errors as for fdsr_swinir. */
#define FDSR_TRANSENET_MAX_DEPTH 32
#define FDSR_TRANSENET_GRAPH 1
typedef struct fdsr_transenet_config {
  int32_t n_feats;
  int32_t scale;
  int32_t n_colors;
  int32_t en_depth;
  int32_t de_depth;
} fdsr_transenet_config;
typedef struct fdsr_transenet_obj* fdsr_transenet;
int fdsr_transenet_create(const fdsr_transenet_config* cfg, fdsr_transenet* out);
int fdsr_transenet_load(fdsr_transenet s, const char* name, const float* host_f32, const int64_t* shape, int ndim);
int fdsr_transenet_workspace_bytes(fdsr_transenet s, int batch, int height, int width, size_t* bytes);
int fdsr_transenet_forward(fdsr_transenet s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                           size_t workspace_bytes, void* hip_stream, int flags);
int fdsr_transenet_debug_tensor(fdsr_transenet s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                                size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream);
void fdsr_transenet_destroy(fdsr_transenet s);

/* -- HSENet (MSI_SR_model/model/hsenet.py: HSENET) inference ---------------------------------------------------------------------
 * An object of its own, in the shape of fdsr_transenet.  Exact fp32, NHWC inside, on the GEMM kernels of the SwinIR family (every
 * 3x3 of the body with its ReLU, the gate m * sigmoid(.) as an epilogue) plus: the non-local block as one attention kernel over
 * every pixel of the image (one head of n_feats / 2 channels, unscaled logits, exact row maxima; self form and the cross form of
 * AdjustedNonLocalBlock), one workgroup per (image, 32 queries), k and v streamed in chunks of 128 keys whatever their number, no
 * N x N tensor in memory; the two bilinear resamplings of the HSEM (align_corners=False); sub_mean and add_mean as general 3x3
 * matrices with bias.  Reruns are bitwise identical and an image's result depends neither on B nor on its position in the batch.
 *   fdsr_hsenet_create           validates the configuration without touching the device.  FDSR_E_INVALID outside the envelope:
 *                                n_colors 3; n_feats 16, 32 or 64; scale 2, 3, 4 or 8; n_basic_modules >= 1.
 *   fdsr_hsenet_load             a host fp32 tensor under the reference's state_dict name and shape (sub_mean.weight [3][3][1][1],
 *                                body_modulist.0.body.0.NonLocal_base.theta.weight [n_feats / 2][n_feats][1][1], ...).  Any other
 *                                name or shape: FDSR_E_KEY.  Host-synchronous; drops every captured graph.
 *   fdsr_hsenet_workspace_bytes  for a batch of height x width inputs.  FDSR_E_INVALID unless both sides are at least 2 (the
 *                                half-scale branch needs a pixel).
 *   fdsr_hsenet_forward          x_nchw [B][3][H][W] fp32 -> out_nchw [B][3][H scale][W scale].  flags: FDSR_HSENET_GRAPH replays
 *                                the forward as one captured, linear hipGraph (hip_stream must be a created stream); one graph is
 *                                kept per (B, H, W), captured anew when x, out or the workspace move.
 *   fdsr_hsenet_debug_tensor     runs the forward up to a named tap and copies it out as NHWC [B][dims3[0]][dims3[1]][dims3[2]].
 *                                Taps: head, mI.head, mI.base.nl / .gate, mI.base, mI.down.in, mI.down.nl / .gate, mI.down (half
 *                                scale), mI.up, mI.cross, mI.hsem, mI (I = 0 .. n_basic_modules - 1), body, up.
 * fdsr_swinir_to_u8 is save_img1 for this family too.  Errors as for fdsr_swinir. */
#define FDSR_HSENET_GRAPH 1
typedef struct fdsr_hsenet_config {
  int32_t n_feats;
  int32_t scale;
  int32_t n_colors;
  int32_t n_basic_modules;
} fdsr_hsenet_config;
typedef struct fdsr_hsenet_obj* fdsr_hsenet;
int fdsr_hsenet_create(const fdsr_hsenet_config* cfg, fdsr_hsenet* out);
int fdsr_hsenet_load(fdsr_hsenet s, const char* name, const float* host_f32, const int64_t* shape, int ndim);
int fdsr_hsenet_workspace_bytes(fdsr_hsenet s, int batch, int height, int width, size_t* bytes);
int fdsr_hsenet_forward(fdsr_hsenet s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                        size_t workspace_bytes, void* hip_stream, int flags);
int fdsr_hsenet_debug_tensor(fdsr_hsenet s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                             size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream);
void fdsr_hsenet_destroy(fdsr_hsenet s);

/* -- EDiffSR: ConditionalNAFNet noise predictor + IR-SDE reverse process (EDiffSR/codes: DenoisingNAFNet_arch.py,
 * module_util.py, utils/sde_utils.py) --------------------------------------------------------------------------------
 * An object of its own, independent of fdsr_handle.  fp32 activations (NHWC inside), every 1x1 / 2x2 / 3x3 convolution a GEMM
 * on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered chain per output, no split-K), LayerNorm over channels with eps 1e-5,
 * fixed-order pools: reruns are bitwise identical and an image's result depends neither on B nor on its position in the batch.
 * Weights: host fp32 tensors under the reference's state_dict keys and shapes (fdsr_nafnet_weight_info lists them in
 * state_dict order; fastdiffsr_amd/ediffsr/arch.py is the Python twin).  Unknown key or wrong shape: FDSR_E_KEY.
 * Inputs are [B,3,H,W] fp32 NCHW device tensors of any H, W >= 1: the network pads right / bottom with zeros to a multiple of
 * 2^n_levels and crops its output (check_image_size).
 *   fdsr_nafnet_forward   out = model(x, cond, time): the noise prediction; time_dev [B] fp32 device, one value per image
 *                         (the reference's scalar time is that value repeated).
 *   fdsr_nafnet_set_sde   IRSDE's tables as the reference holds them: thetas / sigmas / sigma_bars [T+1] host fp32 (index 0 unused
 *                         by the loop), dt; sqrt(dt) is formed as (float)sqrt((double)dt), math.sqrt's value.
 *   fdsr_nafnet_sample    IRSDE.reverse_sde (reverse_ode under FDSR_NAFNET_ODE) with mu = cond, t = T .. 1:
 *                           score = -model(x, cond, t) / sigma_bar[t]
 *                           x <- x - (theta[t] (cond - x) - sigma[t]^2 score) dt - sigma[t] (eps sqrt(dt))         (SDE)
 *                           x <- x - (theta[t] (cond - x) - 0.5 sigma[t]^2 score) dt                                (ODE)
 *                         every operation rounded to fp32 in the order written (no contraction).
 *                           state [B,3,H,W]  x_T (IRSDE.noise_state of the upscaled LQ image);  out [B,3,H,W]  x_0
 *                           noise [T,B,3,H,W], plane k = the eps of step t = T - k; or NULL: drawn per step with the library's
 *                             Philox4x32-10 normals (see fdsr_set_seed for the generator): counter (i lo, i hi, k, 0),
 *                             key (seed lo, seed hi), i = (first_image + n)*H*W + pixel -- positions of a GLOBAL image index, so a
 *                             run split into batches draws what the unsplit run draws when each call states its first image.
 *                             fdsr_nafnet_randn writes plane k of that stream.  Ignored under FDSR_NAFNET_ODE.
 *                           traj [T,B,3,H,W] or NULL: x after every step (plane k = after step t = T - k)
 *                         flags: FDSR_SAMPLE_GRAPH captures ONE step (a linear graph on hip_stream, which must be a created
 *                           stream) whose per-step values -- the time-embedding rows, theta / sigma / sigma_bar, the noise plane --
 *                           are read from device tables through a device-side step counter, and replays it T times.  Eager runs
 *                           launch the same kernels with the same arguments: the results are bitwise equal.  One graph is cached per
 *                           object (key: pointers, shape, flags); loading a weight or a schedule drops it.
 *   fdsr_nafnet_debug_tensor  runs the forward up to the named tap and copies it out as NHWC [B][h][w][c] (dims3 = {h, w, c}; the
 *                         padded size at the tap's level): "intro", "enhance" (x + enhance(x)), "encoders.<i>.<j>", "downs.<i>",
 *                         "middle_blks.<j>", "ups.<i>" (after + enc_skip), "decoders.<i>.<j>", "ending" (before the crop).
 *                         Unknown name: FDSR_E_KEY; capacity_floats too small: FDSR_E_INVALID.
 *   fdsr_upscale_bicubic_f32  util.upscale: F.interpolate(scale_factor=scale, mode='bicubic', align_corners=False) on fp32 NCHW
 *                         (A = -0.75, source index (d + 0.5) / scale - 0.5, taps clamped to the image), evaluated in fp64 and
 *                         rounded once.  dst [B,C,h*scale,w*scale].
 * FDSR_E_STATE: a weight is missing, or fdsr_nafnet_sample before fdsr_nafnet_set_sde.  FDSR_E_WORKSPACE: workspace (256-byte
 * aligned) too small.  Stream-ordered, no implicit synchronisation (loading weights / tables is host-synchronous).  Calls on one
 * object must be ordered on one stream.  Messages: fdsr_last_error(NULL). */
#define FDSR_NAFNET_MAX_LEVELS 8
#define FDSR_NAFNET_ODE 2
typedef struct fdsr_nafnet_config {
  int32_t img_channel;                            /* 3 */
  int32_t width;                                  /* a multiple of 16 */
  int32_t n_levels;                               /* len(enc_blk_nums) == len(dec_blk_nums), 1..FDSR_NAFNET_MAX_LEVELS */
  int32_t enc_blk_nums[FDSR_NAFNET_MAX_LEVELS];
  int32_t middle_blk_num;
  int32_t dec_blk_nums[FDSR_NAFNET_MAX_LEVELS];
} fdsr_nafnet_config;
typedef struct fdsr_nafnet_obj* fdsr_nafnet;
int fdsr_nafnet_create(const fdsr_nafnet_config* cfg, fdsr_nafnet* out);
int fdsr_nafnet_num_weights(fdsr_nafnet n);
int fdsr_nafnet_weight_info(fdsr_nafnet n, int index, char* key, int key_capacity, int64_t* shape4, int* ndim);
int fdsr_nafnet_load_weight(fdsr_nafnet n, const char* key, const float* host_f32, const int64_t* shape, int ndim);
int fdsr_nafnet_weights_complete(fdsr_nafnet n);   /* 1: every tensor is loaded, 0: not yet */
int fdsr_nafnet_set_sde(fdsr_nafnet n, int T, const float* thetas, const float* sigmas, const float* sigma_bars, float dt);
int fdsr_nafnet_workspace_bytes(fdsr_nafnet n, int batch, int height, int width, size_t* bytes);
int fdsr_nafnet_forward(fdsr_nafnet n, const float* x_nchw, const float* cond_nchw, const float* time_dev, float* out_nchw, int batch,
                        int height, int width, void* workspace, size_t workspace_bytes, void* hip_stream);
int fdsr_nafnet_sample(fdsr_nafnet n, const float* state_nchw, const float* cond_nchw, const float* noise, uint64_t seed,
                       int64_t first_image, int flags, float* out_nchw, float* traj, int batch, int height, int width,
                       void* workspace, size_t workspace_bytes, void* hip_stream);
int fdsr_nafnet_debug_tensor(fdsr_nafnet n, const char* name, const float* x_nchw, const float* cond_nchw, const float* time_dev,
                             int batch, int height, int width, float* out_nhwc, size_t capacity_floats, int* dims3, void* workspace,
                             size_t workspace_bytes, void* hip_stream);
int fdsr_nafnet_randn(float* dst_nchw, int batch, int height, int width, int plane, uint64_t seed, int64_t first_image,
                      void* hip_stream);
int fdsr_upscale_bicubic_f32(const float* src_nchw, float* dst_nchw, int batch, int channels, int height, int width, int scale,
                             void* hip_stream);
/* Tile-addressed noise for the NAFNet sampler, with fdsr_set_noise_tiles' table and semantics: while one is set, the normals
 * fdsr_nafnet_sample draws itself (noise == NULL, SDE) have i = (y0[n] + y) * scene_w + (x0[n] + x) in their counter, so the tile at
 * (y0, x0) draws the crop of what fdsr_nafnet_randn(dst, 1, SH, SW, k, seed, 0) writes for the whole scene.  first_image must be 0 in
 * every fdsr_nafnet_sample while a table is set, and the batch at most n_tiles: else FDSR_E_INVALID.  The cached graph keys on the
 * table's pointer and scene_w too; the table is read when the kernels run.  origins_dev == NULL: off.
 * fdsr_nafnet_randn_tiles is fdsr_nafnet_randn for such tiles (it takes the table itself, as fdsr_nafnet_randn takes no object):
 * origins_dev [batch][2].  The origins address a counter, not memory: one outside the scene only draws other numbers. */
int fdsr_nafnet_set_noise_tiles(fdsr_nafnet n, const int32_t* origins_dev, int n_tiles, int scene_w);
int fdsr_nafnet_randn_tiles(float* dst_nchw, int batch, int height, int width, int plane, uint64_t seed, const int32_t* origins_dev,
                            int scene_w, void* hip_stream);
void fdsr_nafnet_destroy(fdsr_nafnet n);
/* Precision of the NAFNet's GEMMs (every 1x1 / 2x2 / 3x3 convolution that is not depthwise).
 *   fdsr_nafnet_set_precision   FDSR_PREC_F32 (default: the exact kernel above) or FDSR_PREC_F16X3: fp32-grade, the staged fp32
 *                             activation (after LN + FiLM / the SCA multiply) and the weights are each split into an f16 hi and
 *                             lo part and every product is lo.hi + hi.lo + hi.hi on v_mfma_f32_32x32x16_f16 with an fp32
 *                             accumulator, one summation order per output (no split-K): the bitwise properties above hold in
 *                             either mode.  Activations stay fp32 in memory; LayerNorm statistics, the depthwise convolution,
 *                             SCA / CA, the time path, bias / epilogues and the SDE tail are fp32 in both modes; workspace sizes
 *                             do not change.  Any other mode: FDSR_E_INVALID.  A switch drops the cached graph and rebuilds the
 *                             device weight forms from the fp32 master (after optimizer steps: the trained weights) on the next
 *                             call.  fdsr_nafnet_forward / _debug_tensor / _sample follow the mode; fdsr_nafnet_train_grads and
 *                             fdsr_nafnet_optim_step run in FDSR_PREC_F32 only (FDSR_E_INVALID under f16x3, and under f16 storage).
 *   fdsr_nafnet_check_saturation   f16x3 clamps a GEMM input beyond +-65504 to the f16 range and raises a sticky device flag (so does a NaN).
 *                             This call synchronises hip_stream, reads and clears the flag: FDSR_OK or FDSR_E_SATURATED (the
 *                             outputs since the last check are then not fp32-grade: re-run them in FDSR_PREC_F32, which has no
 *                             such limit).  FDSR_NAF_STORE_F16 raises the same flag from its stores too, and so does a training call under
 *                             fdsr_nafnet_set_train_storage(FDSR_NAF_STORE_F16).  Otherwise always FDSR_OK in FDSR_PREC_F32 with
 *                             FDSR_NAF_STORE_F32. */
int fdsr_nafnet_set_precision(fdsr_nafnet n, int mode);
int fdsr_nafnet_check_saturation(fdsr_nafnet n, void* hip_stream);
/* Storage of the NAFNet's activations: the 16-bit, PSNR-grade sampling mode (11 mantissa bits; not fp32-grade).
 *   fdsr_nafnet_set_storage   FDSR_NAF_STORE_F32 (default) or FDSR_NAF_STORE_F16; any other value: FDSR_E_INVALID.  Storage and
 *                             precision are two settings of one switch: FDSR_NAF_STORE_F16 while the precision is FDSR_PREC_F16X3,
 *                             and fdsr_nafnet_set_precision(FDSR_PREC_F16X3) while the storage is F16, are FDSR_E_INVALID:
 *                             leave one setting (back to F32) before taking the other.  A change
 *                             drops the cached graph and rebuilds the device weight forms on the next call, as a precision switch
 *                             does.  fdsr_nafnet_forward / _debug_tensor / _sample follow the mode (SDE and ODE, eager and graph,
 *                             given and engine-drawn noise); fdsr_nafnet_train_grads and fdsr_nafnet_optim_step return
 *                             FDSR_E_INVALID under F16 storage.  fdsr_nafnet_workspace_bytes does not change: an f16 tensor lies in
 *                             the first half of its fp32 slot.  fdsr_nafnet_debug_tensor returns the stored values widened to fp32.
 *     Arithmetic under FDSR_NAF_STORE_F16.  Stored as f16 (NHWC) between kernels: intro, the RCAB's two convolution outputs,
 *       x + enhance(x), every block's conv1 output, depthwise + gate output, y, conv4's gate output and out, the skips, downs,
 *       middle, ups and decoder results.  Kept in fp32: the 6-channel network input, ending's 3-channel output, LayerNorm statistics,
 *       strip sums, SCA / CA vectors, time rows and their table, the SDE state, cond, noise, trajectory, and all of the prep, tail
 *       and upscale kernels.  A kernel widens what it reads (exact), computes as the fp32 kernel does and rounds once, to nearest
 *       even, where it stores; the strip sums a kernel forms beside its output come from the fp32 values before that rounding.
 *       GEMMs: the staged operand -- fp32 after LN + FiLM or the SCA multiply, or the f16 input as it is -- is rounded to f16 once;
 *       the weight is f16(w 2^e), the hi plane of the f16x3 split forms; every product is one v_mfma_f32_32x32x16_f16 into an fp32
 *       accumulator, chunk after chunk in k order (no split-K, no atomics: the bitwise properties above hold); the epilogue -- bias,
 *       ReLU, gate product, res + v evec with res read as f16, PixelShuffle + skip -- is the fp32 kernel's on acc 2^-e, rounded
 *       once at the store.
 *     Range: a value to be stored or staged beyond +-65504, or a NaN, is clamped and raises the sticky flag that
 *       fdsr_nafnet_check_saturation reads (FDSR_E_SATURATED), in every kernel that stores f16: the mode does not saturate silently. */
#define FDSR_NAF_STORE_F32 0
#define FDSR_NAF_STORE_F16 1
int fdsr_nafnet_set_storage(fdsr_nafnet n, int mode);

/* EDiffSR training: one step of DenoisingModel.optimize_parameters (models/denoising_model.py) on the device, fp32.
 *   fdsr_nafnet_set_thetas_cumsum   IRSDE.thetas_cumsum [T+1] host fp32, after fdsr_nafnet_set_sde (which forgets it).
 *   fdsr_nafnet_train_grads   eps = model(state, cond, t);  score = -eps / sigma_bar[t]
 *                               xt_1_expection = state - (theta[t] (cond - state) - sigma[t]^2 score) dt        (reverse_sde_step_mean)
 *                               xt_1_optimum   = reverse_optimum_step(state, gt, t)
 *                               loss = weight * mean_b mean_chw |.| (l1) or (.)^2 (l2)                           (MatchingLoss)
 *                             and the gradient of loss with respect to every weight, into the object's flat gradient buffer.
 *                             timesteps_dev: int32 [B] in 1..T.  loss_out_dev [1 + B]: the loss, then every image's own mean.
 *                             loss_type: FDSR_NAFNET_LOSS_L1 / _L2; with FDSR_NAFNET_LOSS_WEIGHTED or'ed in: FDSR_E_INVALID
 *                             (is_weighted; the reference's driver passes no weights).  The workspace is the training one
 *                             (fdsr_nafnet_train_workspace_bytes); a forward / sample workspace is not touched.
 *                             Every sum has one order: two calls on the same inputs give the same bits.
 *   fdsr_nafnet_grad_buffer   the flat gradient: device pointer and length in floats; tensors in fdsr_nafnet_weight_info order,
 *                             each in the reference's own layout (what an all-reduce would be applied to).
 *   fdsr_nafnet_read_grad     one tensor of it to the host (synchronises).
 *   fdsr_nafnet_optim_step    kind FDSR_NAFNET_ADAM (torch.optim.Adam, weight_decay as an L2 term), _ADAMW (decoupled), _LION
 *                             (models/optimizer.py; eps unused) over the flat master copy -- hyperparameters as doubles, every
 *                             derived scalar (1 - beta, 1 - lr wd, lr / bias_correction1) formed in double and rounded once -- then a device-side re-pack of every
 *                             form the kernels read.  Drops the sampler's time-row table and graph.  No host round trip.
 *   fdsr_nafnet_read_weight   the current value of one tensor, to host memory or (dst_on_device) stream-ordered to device memory.
 *   fdsr_nafnet_optim_get_state / _set_state   exp_avg, exp_avg_sq (either may be NULL) and the step count, per key; the step
 *                             count is one number for the whole object.
 * FDSR_E_STATE: weights, fdsr_nafnet_set_sde or fdsr_nafnet_set_thetas_cumsum missing; fdsr_nafnet_optim_step without gradients.
 *
 * The same walk opened to an upstream gradient of the caller's choosing (what a torch.autograd.Function needs; fp32 only, the
 * training workspace, FDSR_E_INVALID under FDSR_PREC_F16X3 / FDSR_NAF_STORE_F16 with fdsr_nafnet_train_grads' messages):
 *   fdsr_nafnet_forward_train out = model(x, cond, time), bit for bit fdsr_nafnet_forward's, with every tensor the backward reads
 *                             kept in the workspace.  time_dev: fp32 [B].  *ticket names those activations.  No schedule needed.
 *   fdsr_nafnet_backward      from d_out_nchw (the gradient of anything with respect to out): the gradient of every weight into the
 *                             flat gradient buffer (zeroed first), and, where the pointer is not NULL, d x and d cond (NCHW) --
 *                             the input gradient continues through intro's transposed, tap-flipped 3x3 pack (64 -> 6) and undoes
 *                             cat[x - cond, cond]: d x = g[0:3], d cond = g[3:6] - g[0:3].  B, H, W and the workspace are those
 *                             of the ticket's forward.  One order for every sum, as fdsr_nafnet_train_grads.
 *     Tickets.  One is outstanding at most.  It goes stale with a second fdsr_nafnet_forward_train, fdsr_nafnet_train_grads,
 *     fdsr_nafnet_optim_step, fdsr_nafnet_set_weights_flat, any fdsr_nafnet_load_weight and any precision or storage switch, and
 *     fdsr_nafnet_backward consumes it (no second backward, no retain_graph).  A stale ticket is FDSR_E_STATE and the message
 *     names the call that came in between; it never yields gradients of other activations.  Neither call synchronises the
 *     device after the object's first training call.
 *   fdsr_nafnet_copy_grads    the flat gradient (count == the sum of all tensors' elements; fdsr_nafnet_weight_info order, the
 *                             reference's layouts), stream-ordered into device memory.
 *   fdsr_nafnet_set_weights_flat   all tensors at once from device memory in that same order and layout: the inverse of
 *                             fdsr_nafnet_read_weight.  Stream-ordered copy into the master, then the device-side re-pack of
 *                             fdsr_nafnet_optim_step; drops the time-row table and the graph as that call does.  The weights must
 *                             have been loaded once through fdsr_nafnet_load_weight.  No host round trip. */
#define FDSR_NAFNET_LOSS_L1 0
#define FDSR_NAFNET_LOSS_L2 1
#define FDSR_NAFNET_LOSS_WEIGHTED 256
#define FDSR_NAFNET_ADAM 0
#define FDSR_NAFNET_ADAMW 1
#define FDSR_NAFNET_LION 2
int fdsr_nafnet_set_thetas_cumsum(fdsr_nafnet n, int T, const float* thetas_cumsum);
int fdsr_nafnet_train_workspace_bytes(fdsr_nafnet n, int batch, int height, int width, size_t* bytes);
int fdsr_nafnet_train_grads(fdsr_nafnet n, const float* state_nchw, const float* cond_nchw, const float* gt_nchw,
                            const int32_t* timesteps_dev, int loss_type, float weight, float* loss_out_dev, int batch, int height,
                            int width, void* workspace, size_t workspace_bytes, void* hip_stream);
int fdsr_nafnet_forward_train(fdsr_nafnet n, const float* x_nchw, const float* cond_nchw, const float* time_dev, float* out_nchw,
                              int batch, int height, int width, void* workspace, size_t workspace_bytes, int64_t* ticket,
                              void* hip_stream);
int fdsr_nafnet_backward(fdsr_nafnet n, int64_t ticket, const float* d_out_nchw, float* d_x_nchw, float* d_cond_nchw, int batch,
                         int height, int width, void* workspace, size_t workspace_bytes, void* hip_stream);
int fdsr_nafnet_copy_grads(fdsr_nafnet n, float* dst_dev, size_t count, void* hip_stream);
int fdsr_nafnet_set_weights_flat(fdsr_nafnet n, const float* src_dev, size_t count, void* hip_stream);
int fdsr_nafnet_grad_buffer(fdsr_nafnet n, float** device_ptr, size_t* count);
int fdsr_nafnet_read_grad(fdsr_nafnet n, const char* key, float* host_f32);
int fdsr_nafnet_optim_step(fdsr_nafnet n, int kind, double lr, double beta1, double beta2, double eps, double weight_decay,
                           void* hip_stream);
int fdsr_nafnet_read_weight(fdsr_nafnet n, const char* key, float* dst, int dst_on_device, void* hip_stream);
int fdsr_nafnet_optim_get_state(fdsr_nafnet n, const char* key, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step);
int fdsr_nafnet_optim_set_state(fdsr_nafnet n, const char* key, const float* exp_avg_host, const float* exp_avg_sq_host,
                                int64_t step);

/* Training with f16 activation storage: mixed precision for the training calls, opt-in, fp32 gradients, no loss scaling.
 *   fdsr_nafnet_set_train_storage   FDSR_NAF_STORE_F32 (default) or FDSR_NAF_STORE_F16; any other value: FDSR_E_INVALID.  A setting
 *                             of the training calls alone -- fdsr_nafnet_train_grads, _forward_train, _backward, _optim_step,
 *                             _set_weights_flat and fdsr_nafnet_train_workspace_bytes, which answers for the current setting.  It
 *                             takes effect while the sampling side is FDSR_PREC_F32 with FDSR_NAF_STORE_F32; with the object in
 *                             f16x3 or in sampling f16 storage the training calls refuse as they always did, whatever this setting.
 *                             fdsr_nafnet_forward / _sample / _debug_tensor never look at it.  A change rebuilds the weight forms
 *                             on the next call and makes an outstanding ticket stale, as the other switches do.
 *     Forward.  The f16-storage forward of fdsr_nafnet_set_storage above: its kernels, roundings and range guard, written into the
 *       training slots.  Stored as f16: intro, the RCAB's two convolution outputs, x + enhance(x), per block out, conv1's output, the
 *       depthwise + gate output, y, conv4's pair before the gate (each half rounded once from the fp32 value the gate multiplies) and
 *       the gate output, the downs and the ups.  fp32 as before: LayerNorm statistics, SCA / CA vectors, strip sums, time rows, the
 *       6-channel input, eps, the loss head.  fdsr_nafnet_forward_train's out equals fdsr_nafnet_forward's under FDSR_NAF_STORE_F16
 *       bit for bit.
 *     Workspace.  An f16 tensor has a slot of half the bytes (not the first half of an fp32 slot).
 *     Backward.  Every gradient tensor in memory and the flat parameter gradient are fp32.  A kernel widens what it reads of the
 *       saved forward (exact) and computes in fp32 as the fp32 step does; the gradient is that of the forward as computed, a
 *       rounding passed straight through (d round(v) / d v = 1).  The three choices:
 *       - weight gradients: exact fp32 MFMAs, dW = A^T dY with dY fp32.  Where a prologue forms A again (LN + FiLM for conv1 /
 *         conv4, the SCA multiply for conv3), A is clamped and rounded to f16 as the forward staged it; a saved f16 input without a
 *         prologue is A as it is.  intro's A is the fp32 6-channel input, not rounded (the forward's staging rounded it).
 *       - input gradients: the exact fp32 kernel over the fp32 transposed packs, dX = dY W^T with the master's w, not the hi plane
 *         f16(w 2^e) 2^-e the forward multiplied by (they differ by 2^-12 |w| at most).
 *       - d beta / d gamma: conv3's and conv5's outputs are formed again by the forward's own f16 kernel on the saved input, with
 *         an fp32 store: the very value the forward scaled by beta / gamma, before any rounding.
 *       What the forward formed from fp32 values before a rounding and the backward can only form from the stored ones: SCA's pooled
 *       mean in d W_sca (from the stored gate output), the gate's partners in conv4's gate backward (the stored pair), ReLU's mask
 *       (the stored output).  Every sum keeps one order fixed by the shapes, there are no atomics, two calls give the same bits.
 *     Weights after a step.  fdsr_nafnet_optim_step and fdsr_nafnet_set_weights_flat rebuild the f16 weight forms on the device from
 *       the re-packed arena (per GEMM: max |w| -> e, then f16(w 2^e) and the lo plane in fragment order), bit for bit what the host
 *       builds from the same master; 2^-e goes to a small device table that the training launches of the f16 GEMM kernel read
 *       (sampling passes it as a kernel argument, as before).  No host round trip.
 *     Range.  The f16 stores raise the sticky flag as in sampling: fdsr_nafnet_check_saturation after fdsr_nafnet_train_grads /
 *       _forward_train returns FDSR_E_SATURATED (and clears it); the gradients of that call are not to be used. */
int fdsr_nafnet_set_train_storage(fdsr_nafnet n, int mode);

/* -- input-pipeline helper------------------------------------ */
/* The dataset's tensor transform on the device (data/util.py:66-75 transform_augment: ToTensor() = uint8 / 255 as fp32,
 * HWC -> CHW, then img * (hi - lo) + lo; LRHR_dataset.py:113-119 passes min_max = (-1, 1)): the loader threads hand over
 * the decoded uint8 batch, one byte per sample crosses PCIe.  src [B,H,W,C] uint8 device, dst [B,C,H,W] fp32 device,
 * bit-identical to the torch ops of the reference.  h may be NULL. */
int fdsr_u8_to_tensor(fdsr_handle h, const uint8_t* src_nhwc, float* dst_nchw, int batch, int channels, int height,
                      int width, float lo, float hi, void* hip_stream);

/* The conditioning image: LR uint8 RGB -> PIL-exact bicubic resize (Image.BICUBIC as used by
 * data/prepare_data_mfe_dm.py:17-40; Pillow's 8-bit fixed-point two-pass resample, bit for bit) ->
 * optionally the val-time tensor transform ToTensor()*2-1 (data/util.py:66-75).
 *   src [B,h,w,3] uint8 device; tmp: B*h*W*3 bytes of device scratch;
 *   dst_u8 [B,H,W,3] uint8 and/or dst_f32 [B,3,H,W] fp32 in [-1,1] (either may be NULL).  h may be NULL.
 * The first call for a new (in,out) size builds its coefficient tables (synchronous upload). */
int fdsr_resize_bicubic_u8(fdsr_handle h, const uint8_t* src_nhwc, int batch, int in_h, int in_w, int out_h,
                           int out_w, uint8_t* tmp, uint8_t* dst_u8_nhwc, float* dst_f32_nchw, void* hip_stream);

/* -- whole-scene tiling (fastdiffsr_amd/scene.py; DESIGN "Whole-scene sampling") ------------- */
/* A scene larger than the network takes in one call is sampled as square tiles of `tile` x `tile` pixels that overlap, and the
 * sampled tiles are blended back with separable linear ramps.  The three calls below are the device side; which tiles there are is
 * the caller's plan, handed over as two device tables of int32:
 *   origins [n][2]  (y0, x0) of tile i in the scene; 0 <= y0 <= SH - tile, 0 <= x0 <= SW - tile
 *   ramps   [n][4]  (top, left, bottom, right): over how many pixels the tile's weight ramps up from that side (0: full weight
 *                   up to the border), each in [0, tile]
 * A tile whose origin lies outside these bounds is skipped by every kernel (nothing is read or written for it); ramp lengths are
 * clamped to [0, tile].  Tables are read when the kernels run: keep them alive and unchanged until then.  h may be NULL.
 *
 * fdsr_scene_gather cuts the tiles' inputs out of scene-sized arrays:
 *   scene_u8 [SH,SW,3] uint8 (the upscaled scene)          -> cond  [n,3,tile,tile] fp32, fdsr_u8_to_tensor's arithmetic with
 *                                                             (lo, hi) = (-1, 1): ToTensor() * 2 - 1, bit for bit
 *   field    [planes,3,SH,SW] fp32 or NULL (a noise field) -> noise [planes,n,3,tile,tile], the layout fdsr_sample takes (copies)
 * noise is required with a field and ignored without one. */
int fdsr_scene_gather(fdsr_handle h, const uint8_t* scene_u8, const float* field, int planes, int scene_h, int scene_w,
                      const int32_t* origins, int n_tiles, int tile, float* cond, float* noise, void* hip_stream);
/* fdsr_scene_gather_f32: the same cut for an fp32 image, scene [3,SH,SW] -> tiles [n,3,tile,tile], plain copies (the noise
 * gather with one plane).  For conditioning that is not a uint8 image: EDiffSR's upscaled LQ scene in [0,1]. */
int fdsr_scene_gather_f32(fdsr_handle h, const float* scene, int scene_h, int scene_w, const int32_t* origins, int n_tiles, int tile,
                          float* tiles, void* hip_stream);
/* fdsr_scene_blend adds n sampled tiles [n,3,tile,tile] fp32 into acc [3,SH,SW] and wsum [SH,SW] (fp32; the caller zeroes both
 * once per scene):   acc[c][y][x] = acc + fl(w * v),   wsum[y][x] = wsum + w,   w = fl32(wy(y) * wx(x)), where along an axis
 *   w1(i) = (i < lead ? (i + 1) / (lead + 1) : 1) * (i >= tile - trail ? (tile - i) / (trail + 1) : 1)       i = 0 .. tile - 1
 * with (lead, trail) = (top, bottom) for wy and (left, right) for wx, evaluated in fp64 and rounded to fp32 once as the product.
 * Contract: tile i is one launch on hip_stream, in ascending i; inside a launch every scene pixel belongs to one thread; the
 * product and each sum are single correctly rounded fp32 operations (no fma), and there are no floating-point atomics.  A scene
 * pixel therefore receives its contributions in ascending tile index, whatever the grouping of tiles into calls (as long as the
 * calls pass ascending tiles on one stream): the accumulators are bitwise reproducible and independent of the batching. */
int fdsr_scene_blend(fdsr_handle h, const float* tiles, const int32_t* origins, const int32_t* ramps, int n_tiles, int tile,
                     float* acc, float* wsum, int scene_h, int scene_w, void* hip_stream);
/* fdsr_scene_finish: q = acc / wsum (one fp32 division) -> dst_f32 [3,SH,SW] and / or, through fdsr_tensor2img_u8's arithmetic
 * with (lo, hi) = (-1, 1) (clamp, map to [0,1], * 255, round half to even), dst_u8 [SH,SW,3].  Either destination may be NULL,
 * not both.  Every pixel must have been covered by a tile (wsum > 0). */
int fdsr_scene_finish(fdsr_handle h, const float* acc, const float* wsum, int scene_h, int scene_w, uint8_t* dst_u8,
                      float* dst_f32, void* hip_stream);

/* f16x3 range guard.  The split-f16 arithmetic clamps every operand to +-65504.  GroupNorm'ed conv inputs are re-scaled
 * before the split, but a RAW input (ResnetBlock res_conv, Down/Upsample convs: unet.py:66-83,112) beyond that range would be
 * clamped silently; the kernels raise a sticky device flag instead.  This call synchronises `hip_stream`, reads and clears the
 * flag: FDSR_OK, or FDSR_E_SATURATED if any fdsr_sample / fdsr_unet_forward since the last check clamped a raw input (their
 * outputs are then not fp32-grade: re-run them after fdsr_set_precision(FDSR_PREC_F32), which has no such limit). */
int fdsr_check_saturation(fdsr_handle h, void* hip_stream);

/* Bits of the "k32" and "strip" options of fdsr_debug_option (which kernel form a stride-1 3x3 launch lands on; every setting
 * computes the same function within the tested bounds).  fastdiffsr_amd/_lib.py mirrors the names for the tests and bench.py. */
enum fdsr_k32_bits {
  FDSR_K32_F16X3 = 1,              /* the 16x16x32-MFMA form in f16x3 */
  FDSR_K32_BF16 = 2,               /* ... and in bf16 */
  FDSR_K32_RIDER_16ROW = 4,        /* the 16-row tile with a res_conv rider */
  FDSR_K32_SMALL_GRID_2ROW = 8,    /* the 2-row-per-wave tiles of small grids */
  FDSR_K32_UP2 = 16,               /* the sub-pixel upsample convs */
  FDSR_K32_SMALL_WG_F16X3 = 32,    /* rider-less 64-cout launches of large grids on 4-wave workgroups, two per CU (f16x3) */
  FDSR_K32_SMALL_WG_RIDER_F16X3 = 64,   /* ... those with a rider too, rider chunks first (f16x3) */
  FDSR_K32_SMALL_WG_BF16 = 128,    /* the small-workgroup form in bf16 (8-row tiles) */
  FDSR_K32_SMALL_WG_RIDER_BF16 = 512,   /* ... with a rider in bf16 (off by default: slower) */
  FDSR_K32_RIDER_FIRST_8WAVE = 1024,    /* rider chunks first on the 8-wave rider kernels (launches without a K split) */
  FDSR_K32_DEFAULT = 1 | 2 | 8 | 16 | 32 | 64 | 128 | 1024     /* 1275 */
};
enum fdsr_strip_bits {
  FDSR_STRIP_BF16_64 = 1,          /* bf16 64 -> 64 launches on the column-strip kernel (two workgroups per CU) */
  FDSR_STRIP_F16X3_64 = 2,         /* the f16x3 64 -> 64 launches (one workgroup per CU: hi / lo weight planes) */
  FDSR_STRIP_BF16_ONE_WG = 4,      /* A/B: bf16 64 -> 64 on one workgroup per CU */
  FDSR_STRIP_BF16_CAT64 = 8,       /* bf16 (64 | 64) -> 64 */
  FDSR_STRIP_BF16_RIDER = 16,      /* bf16 64 -> 64 with a res_conv rider */
  FDSR_STRIP_BF16_CAT128 = 32,     /* bf16 (128 | 64) -> 64 (off by default: 216 weight registers spill) */
  FDSR_STRIP_BF16_COUT128 = 64,    /* bf16 128 -> 128 and 64 -> 128 as two workgroups of 64 couts per strip */
  FDSR_STRIP_DEFAULT = 1 | 2 | 8 | 16 | 64                     /* 91 */
};

/* -- introspection for parity tests and bench.py -------------------------- */
/* Debug / A-B options of the launchers (process-wide; nothing in the library reads the environment).  Names:
 * "rider" (0|1|2|3), "up2" (0|1), "th_min_wgs", "splitk" (0|1), "sk_target", "wgrad_form" (0 default | 1 four-wave | 2 eight-wave
 * plain), "wgrad_colsum" (0|1), "wgrad_f32" (0|1), "drop_stage" (0|1: f16x3 training forwards apply Dropout in the staging of the 16x16x32 kernels instead of materialising the dropped
 * activation; default 1), "gnb_fuse" (0|1: f16x3 training steps run the reduce half of the GroupNorm backward in the epilogue of the
 * input-gradient launch; default 1), "wgrad_big_bytes", "strip" (bits: 1 bf16 64 -> 64 launches on the column-strip kernel, 2 the f16x3 ones, 4 A/B: bf16 on one workgroup per CU, 8 bf16 (64|64) -> 64, 16 bf16 64 -> 64 with a res_conv rider, 32 bf16 (128|64) -> 64, 64 bf16 128 -> 128 and 64 -> 128; default 91), "strip_min_wgs" (from this many strip segments on; default 512),
 * "k32" (bits: 1 f16x3, 2 bf16, 4 16-row tiles with a rider, 8 2-row tiles of small grids, 16 the sub-pixel upsample convs, 32 the rider-less f16x3 64-cout
 * launches of large grids on 4-wave workgroups, two per CU, 64 those with a rider too, 128 in bf16 too, 512 the bf16 launches with a rider, 1024 rider chunks first on the 8-wave rider kernels too (launches without a K split); default 1275 -- the 16x16x32-MFMA form of the
 * stride-1 3x3 launches), "k32_sb_min_wgs" (bit 32 from this many workgroups on; default 1024), "k32_stagger" (start delay of a CU's odd
 * workgroup slot in that form, 64-cycle units per K chunk; default 0), "gn_consumer" (0|1: small grids form GroupNorm scale / shift in the consumer conv's prologue from the producers' fixed-point
 * channel-pair sums instead of a gn_finalize launch; default 1), "sat_guard" (0|1), "bf16_f16x3_steps" (probe: bf16 sampling runs the first n, or for n < 0 the last -n, reverse steps on the f16x3 kernels; default 0),
 * "tail" (0|1: the input / output convs of the 16-bit modes on their own bandwidth-shaped kernels),
 * "drop_image_offset" (the batch is images [k, k+N) of a larger one: its dropout masks are those images' masks, and a training step that
 * draws its own target noise draws those images' pixels).
 * Every setting computes the same function within the tested bounds; they exist so that tests can force each kernel
 * form and same-box A/B runs can price them.  Returns FDSR_E_INVALID for an unknown name.  Not for production use. */
int fdsr_debug_option(const char* name, long long value);
/* When on, the next plan keeps every layer output in its own buffer. */
int fdsr_set_debug(fdsr_handle h, int on);
/* Device pointer (NHWC fp32, inside the workspace of the last forward) and shape
 * of the output of reference module `name` ("downs.4", "mid.0", "ups.7", ...). */
int fdsr_debug_tensor(fdsr_handle h, const char* name, const float** dev_ptr,
                      int* n, int* hgt, int* wid, int* ch);
/* Element size of that tensor in the workspace: 4 (fp32), or 2 in bf16 mode, which keeps every
 * activation but the packed input and eps as bf16 in HBM. */
int fdsr_debug_tensor_elem_bytes(fdsr_handle h, const char* name, int* bytes);
/* The GroupNorm table the convolution op `conv` ("<p>.res_block.block1", "<p>.res_block.block2", "final_conv") applied in the last
 * forward: fp32 scale [n][ch] followed by shift [n][ch] (y = x * scale + shift in front of the Swish), as an offset into the
 * workspace like fdsr_debug_tensor.  A launch that formed its scale / shift itself (option "gn_consumer") leaves the table unwritten. */
int fdsr_debug_gn_table(fdsr_handle h, const char* conv, const float** dev_ptr, int* n, int* ch);
/* Timing hooks: record hipEvents on `stream` around every launch of the
 * dominant kernel family (the 3x3 MFMA convolutions) during the next calls,
 * then read back count / total milliseconds / algorithmic FLOPs. */
int fdsr_profile_begin(fdsr_handle h);
int fdsr_profile_end(fdsr_handle h, int* launches, double* conv_ms, double* conv_flops,
                     double* conv_bytes);

/* nn.Module.train() / .eval() of the denoiser: in training mode the Dropout(p) in front of every block2 conv
 * (unet.py:89-101, p = fdsr_config.dropout) is live, in fdsr_unet_forward and in fdsr_train_grads alike (the two
 * fp32-grade precisions only).  The keep-mask of a forward is a pure function of (fdsr_set_seed, the count of training-mode
 * forwards so far, block, element) -- Philox4x32-10 -- and can be read back for parity checks:
 * fdsr_debug_dropout_mask gives its offset inside the workspace of the last forward, [N][H][W][C] bytes (1 = keep),
 * and the factor 1/(1-p) kept elements are multiplied by.  `block` is the reference module, e.g. "downs.1". */
int fdsr_set_training(fdsr_handle h, int on);
/* Key of the dropout masks alone (fdsr_set_seed sets it too) and restart of the forward count: the facade draws it from
 * torch's generator before every training-mode call, so runs repeat under torch.manual_seed like the reference's. */
int fdsr_set_dropout_seed(fdsr_handle h, uint64_t seed);
int fdsr_debug_dropout_mask(fdsr_handle h, const char* block, const unsigned char** dev_off, int* n, int* hgt, int* wid,
                            int* ch, float* scale);

/* ---- training step (every variant) ------------------------------------------------
 * DDPM.optimize_parameters (model/model.py:47-57): zero_grad, l_pix = netG(data) = p_losses
 * (fastdiffsr_modules/diffusion.py:242-270), l_pix.sum() / (b*c*h*w), backward, Adam.step.  The engine keeps
 * an fp32 master copy of every executed checkpoint tensor, its gradient and the two Adam moments on the
 * device; the step runs in FDSR_PREC_F32 (everything exact fp32) or FDSR_PREC_F16X3 (forward, input-gradient and
 * weight-gradient convolutions fp32-grade on split-f16 MFMA kernels; everything else fp32), every reduction in a fixed
 * order: a step is bitwise reproducible.  The 44 never-executed tensors of the schema
 * (unet.py:212) get no gradient and are not touched, as in torch. */

/* Workspace for fdsr_train_grads at this shape (the forward keeps every activation). */
int fdsr_train_workspace_bytes(fdsr_handle h, int batch, int height, int width, size_t* bytes);

/* Forward + loss + backward: gradients of  loss_scale * loss(target, UNet(x, noise_level))  w.r.t. every
 * executed parameter, left on the device (fdsr_get_grad).
 *   x_nchw       [B,6,H,W]  cat([SR, x_noisy]) (diffusion.py:265-266), x_noisy = q_sample(img2res(HR,SR), gamma, noise)
 *   noise_level  [B]        gamma, the continuous sqrt(alpha_bar) drawn per sample (:246-255)
 *   target_nchw  [B,3,H,W]  the noise that q_sample mixed in (:259)
 *   loss_l2      0: nn.L1Loss(reduction='sum') (loss_type 'l1', :101-103); 1: nn.MSELoss(reduction='sum'); 2: the SUM of the Charbonnier
 *                terms sqrt(d^2 + 1e-6) (TESR's 'l1' is their mean, tesr_modules/unet.py:956-967: put the 1 / (b*c*h*w) of the mean into
 *                loss_scale beside the one of model.py:50-52)
 *   (SR3 / TESR variants: x_nchw = cat[SR, q_sample(HR, ...)] as their p_losses forms it, noise_level = the integer time t as a float
 *    (SR3, ddpm_modules/diffusion.py:279-291) or gamma (TESR); the backward then includes the SelfAttention blocks.
 *    GDP variant, gdp_modules/diffusion.py:277-299: x_nchw = cat[q_sample(HR, t), SR], noise_level = t as a float, target_nchw = HR
 *    itself -- the network predicts x_0 -- and loss_l2 = 1 for both of its loss types; the backward then runs through the scale-shift
 *    GroupNorms (whose (scale, shift) gradient feeds each ResBlock's Linear and the time MLP), the average-pooled / nearest-upsampled
 *    ResBlocks and the heads of QKVAttentionLegacy, gdp_modules/unet.py:276-439, :461-488.)
 *   loss_scale   the reference divides the summed loss by b*c*h*w before backward (model.py:50-52)
 *   loss_host    optional: receives the UNSCALED summed loss (what netG(data) returns); synchronises the stream
 * All pointers but loss_host are device pointers. */
int fdsr_train_grads(fdsr_handle h, const float* x_nchw, const float* noise_level, const float* target_nchw,
                     int loss_l2, float loss_scale, float* loss_host, int batch, int height, int width,
                     void* workspace, size_t workspace_bytes, void* hip_stream);
/* The same step from the training pair itself: img2res (diffusion.py:283-289), q_sample (:233-241) and cat([SR, x_noisy]) (:257-263)
 * run in the kernel that writes the packed network input (the arithmetic of the tensor torch forms op by op: separately rounded products and sums).  hr / sr / noise:
 * [B,3,H,W] NCHW fp32 device pointers, gamma: [B] (the continuous sqrt(alpha_bar) per sample, :246-256).  noise == NULL: the
 * engine draws N(0,1) itself and uses it as the target: plane 0 under the call counter after its increment (fdsr_set_seed), what
 * fdsr_randn(.., plane 0) reports after the step; a shard at "drop_image_offset" k draws images [k, k+N) of that plane. */
int fdsr_train_grads_pairs(fdsr_handle h, const float* hr_nchw, const float* sr_nchw, const float* gamma, const float* noise_nchw,
                           int loss_l2, float loss_scale, float* loss_host, int batch, int height, int width, void* workspace,
                           size_t workspace_bytes, void* hip_stream);

/* torch.optim.Adam.step on every executed tensor (model.py:37-38, :56: lr from the config, betas (0.9, 0.999),
 * eps 1e-8), then the device-side re-packing of the fp32 kernel forms. */
int fdsr_adam_step(fdsr_handle h, float lr, float beta1, float beta2, float eps, void* hip_stream);

/* Copy one tensor of the master copy / of the last gradients to the host, in checkpoint layout
 * (state_dict() after training; tests).  Never-executed tensors: FDSR_E_KEY. */
int fdsr_get_weight(fdsr_handle h, const char* key, float* host);
int fdsr_get_grad(fdsr_handle h, const char* key, float* host);

/* torch.optim.Adam's state of one executed tensor (exp_avg, exp_avg_sq; either may be NULL on get) and the
 * common step count: what `I{iter}_E{epoch}_opt.pth` stores and load_network restores (model.py:139-146, :161-166). */
int fdsr_get_optimizer_state(fdsr_handle h, const char* key, float* exp_avg, float* exp_avg_sq, int* step);
int fdsr_set_optimizer_state(fdsr_handle h, const char* key, const float* exp_avg, const float* exp_avg_sq, int step);

/* Device pointer and length of the gradient arena (every executed tensor in schema order).  Data-parallel
 * training (the reference wraps netG in nn.DataParallel, networks.py:116-118) sums it over the ranks in place,
 * one RCCL all-reduce, between fdsr_train_grads and fdsr_adam_step. */
int fdsr_grad_arena(fdsr_handle h, float** dev_ptr, size_t* count);

/* After optimiser steps: rebuild the 16-bit weight forms (f16x3 / bf16 sampling) from the master copy.
 * fdsr_sample and the eval-mode fdsr_unet_forward do this by themselves when needed (one host re-pack after the last optimiser
 * step, not one per step). */
int fdsr_sync_weight_forms(fdsr_handle h);

#ifdef __cplusplus
}
#endif
#endif /* FDSR_H_ */
