/* vd_amd.h -- C ABI of the MI355X-native video-diffusion denoise engine (libvdamd.so).
 *
 * The reference (cliangyu/video-diffusion) is pure Python and has no FFI; its seam for this hot path
 * is a set of Python call signatures.  Each entry point below names the reference
 * interface it replaces (paths relative to /root/reference).  All `const float*`/`float*` tensor
 * arguments are DEVICE pointers owned by the caller unless the name says `host`; `stream` is a
 * hipStream_t passed as void*.  Every function returns 0 on success or a negative code
 * (-1 bad argument / unsupported configuration, -2 HIP runtime error); text via vd_last_error().
 * No entry point synchronises the stream except vd_load_weight (a blocking H2D copy), vd_device_errors, and the two that read a
 * B*T mask back to shape their launches (vd_window_begin with the prefix cache / suffix skip on, vd_score_windows with suffix_skip = 1).
 * Contract: ONE device per process (the reference launches one process per GPU, command_launchers.py:32-62) and one
 * stream at a time per engine: kernel attributes are cached process-wide and an engine owns a single workspace.
 * vd_set_weight_storage binds the process to the current device and refuses a second one.
 */
#ifndef VD_AMD_H
#define VD_AMD_H
#ifdef __cplusplus
extern "C" {
#endif

/* Keys of video_model_and_diffusion_defaults() that shape the network
 * (improved_diffusion/script_util.py:15-57, create_video_model :229-300). */
typedef struct vd_config {
    int image_size;              /* 32 / 64 / 128 / 256 -> channel_mult table, script_util.py:255-264 */
    int num_channels;
    int num_res_blocks;
    int num_heads;
    int T;                       /* model's max_frames: only used by the frame-embedding period (unet.py:921) */
    int n_attention_ds;          /* attention_resolutions converted to downsample rates, script_util.py:266-268 */
    int attention_ds[8];
    int use_scale_shift_norm;
    int use_spatial_encoding;
    int use_frame_encoding;
    int enforce_position_invariance;
    int use_rpe_net;
    int allow_interactions_between_padding;
    float rp_alpha, rp_beta, rp_gamma;   /* bucket parameters of the table RPE (unet.py:330-340) */
    int time_embed_mult;         /* 4: time_embed_dim = 4*num_channels (unet.py:605) */
    int cond_emb_type;           /* CondMargVideoModel (unet.py:929-1020): 0 'channel' (5 input channels: frames + obs / kinda-marg
                                    indicators), 1 'duplicate' | 'all' (6: noisy frames | x0 * obs_mask), 2 't=0' (3: x itself,
                                    observed frames get timestep -1); the '-initzero' spellings differ at initialisation only */
    int learn_sigma;             /* 1: the network has 6 output channels, eps | variance values (script_util.py:129-131).  Boundary A
                                    only: the reference's own sampler cannot use them on video tensors -- p_mean_variance
                                    asserts model_output.shape == (B, 2*T, ...) (gaussian_diffusion.py:283, C = x.shape[1] = T) --
                                    so vd_p_sample & co. refuse such an engine as the reference does */
} vd_config;

typedef struct vd_engine vd_engine;

const char* vd_last_error(void);
const char* vd_version(void);
/* 16 hex digits: SHA-1 over the compiler flags and every source the library was built from (_lib.source_sha() recomputes it from
 * the sources on disk: a loaded library that does not match them is stale, whatever the file times say). */
const char* vd_source_sha(void);

/* CondMargVideoModel(...) constructor via create_video_model (script_util.py:229-300; unet.py:929-947).
 * Host-only: builds the topology and the parameter table; touches no GPU. */
int vd_create(const vd_config* cfg, vd_engine** out);
void vd_destroy(vd_engine* e);

/* model.state_dict() keys/shapes, in the reference's order (checkpoint format, train_util.py:570-574). */
int vd_param_count(vd_engine* e);
int vd_param_info(vd_engine* e, int index, char* name, int name_cap, int* ndim, long long shape[4]);

/* model.load_state_dict(sd) (scripts/video_sample.py:565).  Weights live in ONE packed device buffer in kernel-ready
 * layouts chosen at load time (split arithmetic: 3x3 stride-1 convs as the Winograd image U = G g G^T in three 16-bit
 * planes [I/16][16][O/32][3][64][8]; linear / 1x1 / stem / stride-2 convs as split MFMA fragments
 * [K/16][N/32][3][64][8], each image followed by its per-output scales; spatial_encoding -> [HW][C]) so that a
 * single RCCL broadcast replaces dist_util.sync_params' per-tensor broadcasts (dist_util.py:139-143).  The layout depends on
 * VD_MATH: vd_weights_layout_id() identifies it, and ranks compare it before accepting a broadcast buffer.
 * The buffer is caller-owned (e.g. a torch tensor) and must outlive the engine.
 * vd_set_weight_storage / vd_set_weight_storage_host with another buffer than the bound one drop every captured window graph first
 * (the graphs hold addresses inside the image; a window in flight is lost: vd_window_run reports "window graphs invalidated").
 * vd_load_weight / vd_load_weight_bwd into device storage of an engine that has run wait for the whole device before they
 * overwrite the image in place: captured graphs keep reading it, and the next window sees the new weights. */
long long vd_weights_bytes(vd_engine* e);
int vd_set_weight_storage(vd_engine* e, void* dev_buffer, long long bytes);
/* The same packed image assembled in HOST memory (no GPU needed): pack once, then ship it -- a broadcast, a file, one
 * H2D copy into a buffer later given to vd_set_weight_storage followed by vd_mark_weights_loaded.  The compute entry
 * points refuse an engine whose storage is still on the host. */
int vd_set_weight_storage_host(vd_engine* e, void* host_buffer, long long bytes);
int vd_load_weight(vd_engine* e, const char* name, const float* host_data, long long numel);
int vd_weights_missing(vd_engine* e);          /* number of parameters not loaded yet */
int vd_mark_weights_loaded(vd_engine* e);      /* after receiving the packed buffer by broadcast */
unsigned long long vd_weights_layout_id(vd_engine* e);   /* hash of (parameter table, kinds, offsets, arithmetic mode) */

/* Channels / resolution of the tensor the positional encodings are added to (unet.py:669-675,914-926). */
int vd_pos_channels(vd_engine* e);
int vd_pos_resolution(vd_engine* e);

/* Frequency tables of timestep_embedding / frame_embedding (nn.py:89-122), built by the host with
 * the reference's own float32 expression so the angles agree bit for bit.  A call that replaces tables already uploaded drops
 * every captured window graph first, like vd_set_schedule: each captured forward holds the tables' addresses. */
int vd_set_freqs(vd_engine* e, const float* host_time_freqs, int n_time, const float* host_frame_freqs, int n_frame);

/* SpacedDiffusion tables (respace.py:68-82, gaussian_diffusion.py:123-172,299-317).
 * host_tab: VD_NTAB rows of num_timesteps float32 (float64 tables cast like _extract_into_tensor,
 * gaussian_diffusion.py:1019-1031), row order VD_TAB_*.  timestep_map + rescale = _WrappedModel
 * (respace.py:111-119): t_model = map[t] * rescale (rescale = 1000/original_steps, or 1 with rescale off). */
enum { VD_TAB_SQRT_RECIP = 0, VD_TAB_SQRT_RECIPM1, VD_TAB_COEF1, VD_TAB_COEF2, VD_TAB_LOGVAR /* model log variance */,
       VD_TAB_ACP, VD_TAB_ACP_PREV, VD_TAB_SQRT_ACP, VD_TAB_SQRT_1M_ACP,
       VD_TAB_POST_LOGVAR /* posterior_log_variance_clipped */, VD_TAB_LOG_1M_ACP /* log_one_minus_alphas_cumprod */,
       VD_TAB_ALPHA /* alphas = 1 - betas (the guidance weight, gaussian_diffusion.py:363) */, VD_NTAB };
int vd_set_schedule(vd_engine* e, int num_timesteps, const float* host_tab, const int* host_timestep_map,
                    float rescale);
/* What the network's output is (ModelMeanType, gaussian_diffusion.py:29-36,326-341): 0 EPSILON (default); 1 START_X
 * (predict_xstart=True, script_util.py:429-431): pred_xstart = clamp(model_output), DDIM derives eps from it. */
int vd_set_model_mean_type(vd_engine* e, int type);


/* Timestep indices outside [0, num_timesteps) make the reference raise IndexError (_extract_into_tensor,
 * gaussian_diffusion.py:1019-1031).  The step entry points stay asynchronous: such a batch element is written as NaN
 * and a sticky device flag is set; this call waits for the whole DEVICE (steps issued on any stream, non-blocking side streams included, have finished),
 * copies the flags to the host, clears them, and the host
 * mirror raises IndexError.  bit 0: timestep index out of range.  Raised by every entry that runs the network (the timestep map
 * in front of the forward: vd_p_sample, vd_ddim_sample, vd_ddim_reverse_sample, vd_dpmpp_2m_sample, vd_p_mean_variance, vd_guided_step,
 * vd_dps_step, vd_eps_vjp, vd_ode_nll_eval, the window executor's captured step), by vd_score_windows / vd_op_eps_mse, vd_op_dps_seed, vd_op_ode_heun and by vd_vb_terms.  The network-free passes
 * vd_posterior_update, vd_posterior_from_xstart, vd_ddim_reverse_from_xstart, vd_dpmpp_2m_from_xstart and vd_q_sample (index -1 wraps
 * to the last row there; below -num_timesteps or above the last row is out of range) poison item b with NaN and do NOT raise
 * the bit: the range of t is their caller's to check (the host mirror reaches the *_from_xstart forms only behind
 * vd_p_mean_variance, which has raised it).  vd_prior_bpd reads no t.
 * bit 1: the network output a step consumed was not finite.  The reference would carry the NaN into its sample; here the clamp
 * of clip_denoised would turn it into a plausible -1, so the posterior kernels keep such an element NaN and set this bit
 * (vd_p_sample, vd_ddim_sample, vd_ddim_reverse_sample, vd_dpmpp_2m_sample, vd_p_mean_variance, vd_posterior_update, vd_posterior_from_xstart, vd_vb_terms, vd_guided_step, vd_dps_step,
 * the window executor's captured step).  In the default f16x3 arithmetic (two fp16 pieces per fp32 operand) this is how an
 * operand beyond the split's range (|x| >= 2^15 = 32768: the scaled remainder (x - a0) 2^12 then leaves fp16; for a 3x3 conv the operand
 * is the Winograd-domain value, a signed sum of four inputs, so |input| < 2^13 is safe) anywhere in the network shows: VD_MATH=bf16x6
 * carries the full fp32 range.
 * The host mirror raises FloatingPointError. */
int vd_device_errors(vd_engine* e, int* flags);

/* Test hook: what the engine's scratch memory holds when the next call begins.  A call's bits must not depend on it -- every range a
 * kernel reads is written by the same call first -- and tests/test_gpu_scratch_history.py checks that by comparing a call behind a fill
 * with the same call on a freshly created engine.  In order: requires the engine's device; ends a held loss-guidance pass (its tape lives
 * in the workspace: vd_guide_finish then fails on the stale ticket with this call's reason); waits for the whole device; hipMemset's
 * every byte of the workspace (all of its capacity, the tail and what a larger window grew included) and of every engine-owned buffer
 * that is scratch -- the list, with the rule and the buffers that are state, stands above the entry in csrc/engine.hip -- to `byte`
 * (0..255); reports the bytes written (0 on an engine that has not run).
 * Left alone: every address (nothing grows, nothing is freed, captured window graphs stay valid and are not dropped, the window generation
 * does not move) and every piece of state: weights and their backward image, the schedule and coefficient tables, the device flags, the
 * particle state, the armed window's counters, Philox triple and carried history, prefix stores, blur taps, operator matrices, FreeU's
 * trig tables, the zero mask of cfg_scale.  No existing path calls it. */
int vd_scratch_fill(vd_engine* e, int byte, long long* bytes_filled);

/* Longest window, in frames per batch item, that every forward / step / window entry point accepts: 128.  A window is any
 * T in 1..vd_max_window_frames() (the reference's UNet takes any T; --max_frames picks it at sampling time).  T <= 32 runs
 * on the original temporal attention / GroupNorm kernels, 33..128 on their long-window forms (key tiles with an online
 * softmax).  vd_guided_step (use_gradient_method), vd_dps_step, vd_eps_vjp and vd_ode_nll_eval are limited to T <= 32.  Larger T fails with a message naming the limit. */
int vd_max_window_frames(void);

/* The envelope of a model, checked by vd_create (host only) with the launchers' own constants and predicates, so that a model
 * that cannot be served fails there and not at its first forward.  The message names the parameter, the layer and the limit:
 *   num_channels           a GroupNorm32 over more than vd_gn_max_channels() = 1024 channels, the two halves of a decoder concat
 *                          counted together (num_channels 160 at 64 x 64: output_blocks.0 normalises 640 + 640)
 *   num_heads              a head dim the attention kernels do not serve: vd_attn_temporal_variant / vd_attn_spatial_variant refuse it
 *                          (multiples of 8; spatial: 8..64, 72, 80, 96, 112, 128), or heads that do not divide a layer's width
 * The spatial attention's forward has no token ceiling (attention_resolutions is free); the backward-data pass serves 1024 tokens
 * per frame and says so when it is asked.  The temporal attention's LDS ceiling moves with T and stays at the forward; no head dim
 * that the spatial attention serves reaches it at T <= 128. */
int vd_gn_max_channels(void);

/* Bytes of engine-owned workspace a (B, T) window needs; allocated lazily by the first call.  The relative-position tensors
 * grow with B*T^2 (about 60 KB per (b, t, s) pair for the default 64x64 model: ~1 GB at B = 1, T = 128).  The figure is the
 * activation arena of one forward plus the step's tail: t_model, the two network-output buffers (the second one is out_u of a
 * cfg_scale != 1 step and the finished x_0 of a dynamic-threshold step, below) and the scratch of the two guidance options. */
int vd_workspace_bytes(vd_engine* e, int B, int T, long long* bytes);

/* observed_frames: 0 'x_0', 1 'x_t', 2 'x_t_minus_1' (unet.py:958-974,991-1013). */

/* Boundary A: model(x, timesteps, **model_kwargs) -> eps   (unet.py:949-1026 after respace.py:111-119).
 * x, obs_src, eps: [B][T][3][H][W] fp32;  obs/lat/km masks: [B*T] fp32;  frame_indices: [B*T] int64;
 * t_model: [B] fp32 value handed to the network. */
int vd_unet_forward(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask,
                    const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                    const float* t_model, int observed_frames, float* eps, void* stream);

/* diffusion.p_sample(model, x, t, clip_denoised, model_kwargs) -> {'sample','pred_xstart'}
 * (gaussian_diffusion.py:403-448 through SpacedDiffusion.p_mean_variance, respace.py:84-86).
 * t: [B] int64 respaced indices (device).  noise: explicit N(0,1) draws or NULL -> in-kernel
 * Philox4x32-10(seed, offset).  x is not modified; sample/pred_xstart/eps are outputs (the last two may be NULL). */
int vd_p_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask,
                const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                const long long* t, int observed_frames, int clip_denoised, const float* noise,
                unsigned long long seed, unsigned long long offset, float* sample, float* pred_xstart, float* eps,
                void* stream);

/* diffusion.ddim_sample(..., eta) (gaussian_diffusion.py:597-634). */
int vd_ddim_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask,
                   const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                   const long long* t, int observed_frames, int clip_denoised, float eta, const float* noise,
                   unsigned long long seed, unsigned long long offset, float* sample, float* pred_xstart, float* eps,
                   void* stream);

/* diffusion.ddim_reverse_sample(model, x, t, clip_denoised, model_kwargs) -> {'sample','pred_xstart'} (gaussian_diffusion.py:636-668):
 * the deterministic DDIM step run towards the noise, x_t -> x_{t+1} (eta = 0 is the only path the reference has).  One UNet
 * forward, then one fused pass (launch_sampler_pass: deterministic_kernel, beside the posterior kernel) in the reference's operation order:
 *   pred_xstart = sqrt_recip[t] x - sqrt_recipm1[t] eps   (START_X: the network output), non-finite check, clamp when clip_denoised
 *   eps'        = (sqrt_recip[t] x - pred_xstart) / sqrt_recipm1[t]
 *   sample      = pred_xstart sqrt(abn) + sqrt(1 - abn) eps',   abn = alphas_cumprod[t + 1], 0 at the last index
 * (alphas_cumprod_next is the alphas_cumprod row shifted by one: no schedule row of its own).  No noise is read and no Philox
 * draw is consumed.  Opening checks, observed_frames and the treatment of a t[b] outside the schedule (NaN for item b, bit 0 of
 * the device flags; bit 1 for a non-finite network output) as in vd_ddim_sample.  pred_xstart and eps may be NULL.
 * vd_ddim_reverse_from_xstart: the same pass on a caller's x_0 prediction -- the `denoised_fn` form, as vd_posterior_from_xstart
 * is for the other samplers; per_sample = T*3*H*W must be a multiple of 4 and every tensor 16-byte aligned. */
int vd_ddim_reverse_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask,
                           const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                           const long long* t, int observed_frames, int clip_denoised, float* sample, float* pred_xstart,
                           float* eps, void* stream);
int vd_ddim_reverse_from_xstart(vd_engine* e, int B, long long per_sample, const float* x, const float* xstart_in,
                                const long long* t, int clip_denoised, float* sample, float* pred_xstart, void* stream);

/* diffusion.dpmpp_2m_sample(model, x, t, prev_xstart, clip_denoised, model_kwargs) -> {'sample','pred_xstart'}: this project's
 * extension (the reference has no such sampler) -- DPM-Solver++(2M), the second-order multistep solver in its data-prediction
 * form, x_t -> x_{t-1}.  One UNet forward, then one fused pass (the same kernel template as ddim_reverse_sample):
 *   D_t    = sqrt_recip[t] x - sqrt_recipm1[t] eps   (START_X: the network output), non-finite check, clamp when clip_denoised
 *            -- what vd_ddim_sample calls pred_xstart; it is written to `pred_xstart` and is the NEXT step's prev_xstart
 *   D      = D_t + w[t] (D_t - D_prev)   with history (prev_xstart = D_prev, the D_t of the step at index t + 1);  D = D_t without
 *   eps'   = (sqrt_recip[t] x - D) / sqrt_recipm1[t]
 *   sample = D sqrt(abp) + sqrt(1 - abp) eps',   abp = alphas_cumprod_prev[t]
 * i.e. the eta = 0 DDIM update with D in place of the x_0 prediction (algebraically x <- (sigma'/sigma) x - alpha' (e^-h - 1) D, written
 * so that nothing infinite appears at t = 0); without history it IS the eta = 0 DDIM step.  No noise is read, no Philox draw consumed.
 * w: the row uploaded by vd_set_multistep_weights, w[t] = (lambda[t-1] - lambda[t]) / (2 (lambda[t] - lambda[t+1])) for
 * 1 <= t <= num_timesteps - 2 with lambda = log(alphas_cumprod / (1 - alphas_cumprod)) / 2, and w[0] = w[num_timesteps - 1] = 0 (the
 * step to alphas_cumprod_prev = 1 is first-order: lambda is infinite there).  The row belongs to the schedule: it must have the bound
 * schedule's length, vd_set_schedule drops it, and the sampler fails by name without one.  It is a call of its own because the
 * VD_NTAB-row table of vd_set_schedule is public layout.  The sampler is meant for steps uniform in lambda (timestep_respacing
 * 'logsnrN' of the host mirror): with steps uniform in t and few of them w grows past 1 at the clean end and first-order DDIM can be
 * the better choice.
 * prev_xstart may be NULL (no history: a chain's first step) and may be the same tensor as pred_xstart (history kept in place: an
 * element is read and then written by one thread).  Opening checks, observed_frames, a t[b] outside the schedule and a non-finite
 * network output as in vd_ddim_sample.  pred_xstart and eps may be NULL.
 * vd_dpmpp_2m_from_xstart: the same pass on a caller's x_0 prediction -- the `denoised_fn` form, as vd_ddim_reverse_from_xstart;
 * per_sample = T*3*H*W must be a multiple of 4 and every tensor 16-byte aligned. */
int vd_set_multistep_weights(vd_engine* e, int num_timesteps, const float* host_w);
int vd_dpmpp_2m_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask,
                       const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                       const long long* t, const float* prev_xstart, int observed_frames, int clip_denoised, float* sample,
                       float* pred_xstart, float* eps, void* stream);
int vd_dpmpp_2m_from_xstart(vd_engine* e, int B, long long per_sample, const float* x, const float* xstart_in,
                            const float* prev_xstart, const long long* t, int clip_denoised, float* sample, float* pred_xstart,
                            void* stream);

/* diffusion.dpmpp_2m_sde_sample(model, x, t, prev_xstart, clip_denoised, model_kwargs) -> {'sample','pred_xstart'}: this project's
 * extension (the reference has no such sampler) -- SDE-DPM-Solver++(2M) of Lu et al. 2022, the STOCHASTIC second-order multistep
 * solver, x_t -> x_{t-1}.  One UNet forward, then one fused pass (dpmpp_2m_sde_kernel, a third kernel beside the two above):
 *   D_t    = as vd_dpmpp_2m_sample forms it; written to `pred_xstart`, the NEXT step's prev_xstart
 *   D      = D_t + w[t] (D_t - D_prev)   with history;  D = D_t without          (w: the row of vd_set_multistep_weights)
 *   sigma  = sqrt((1 - abp) / (1 - ab)) sqrt(1 - ab / abp),   ab = alphas_cumprod[t], abp = alphas_cumprod_prev[t]   (vd_ddim_sample's at eta = 1)
 *   eps'   = (sqrt_recip[t] x - D) / sqrt_recipm1[t]
 *   sample = D sqrt(abp) + sqrt(1 - abp - sigma^2) eps' + [t != 0] sigma z
 * i.e. the eta = 1 DDIM update with D in place of the x_0 prediction, as vd_dpmpp_2m_sample is the eta = 0 update on the same D.  With
 * lambda = log(ab / (1 - ab)) / 2, h = lambda[t-1] - lambda[t], r = h_prev / h and w[t] = 1 / (2 r) it is term by term
 *   x_{t-1} = (sigma'/sigma) e^-h x + alpha' (1 - e^-2h) D_t + alpha' (1 - e^-2h) (D_t - D_prev) / (2 r) + sigma' sqrt(1 - e^-2h) z.
 * At t = 0 abp = 1, w = 0 and sigma = 0: sample = D_0, nothing infinite, no noise.  Without history it IS vd_ddim_sample at eta = 1.
 * There is no eta: the stochasticity is the solver's own.  Meant for steps uniform in lambda ('logsnrN'), as vd_dpmpp_2m_sample.
 * z: `noise` [B][per], or with noise = NULL element i of the Philox stream at (seed, offset) -- vd_randn's element i, the draw
 * vd_ddim_sample makes for the same state; a step consumes the range of B*per blocks the other drawing samplers consume.
 * prev_xstart may be NULL and may be the same tensor as pred_xstart, sample may be x (an element is read and then written by one
 * thread).  A t[b] outside the schedule poisons every output of item b and reads no table; a network output that is not finite
 * leaves as NaN and sets bit 1 of the device flags, both as in vd_ddim_sample.  Without a weight row the call fails by name.
 * pred_xstart and eps may be NULL.
 * vd_dpmpp_2m_sde_from_xstart: the same pass on a caller's x_0 prediction, no network -- the `denoised_fn` form.  ANY per_sample and
 * alignment are served: 16-byte accesses where per_sample % 4 == 0 and every tensor is 16-byte aligned, element by element otherwise
 * (same values: the Philox draw of an element does not depend on the path). */
int vd_dpmpp_2m_sde_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask,
                           const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                           const long long* t, const float* prev_xstart, int observed_frames, int clip_denoised, const float* noise,
                           unsigned long long seed, unsigned long long offset, float* sample, float* pred_xstart, float* eps,
                           void* stream);
int vd_dpmpp_2m_sde_from_xstart(vd_engine* e, int B, long long per_sample, const float* x, const float* xstart_in,
                                const float* prev_xstart, const long long* t, int clip_denoised, const float* noise,
                                unsigned long long seed, unsigned long long offset, float* sample, float* pred_xstart, void* stream);

/* diffusion.unipc_sample(model, x, t, state, clip_denoised, model_kwargs) -> {'sample','pred_xstart','state'}: this project's extension
 * (the reference has no such sampler) -- UniPC of Zhao et al. 2023 in its data-prediction form, multistep order 2, B(h) = e^-h - 1
 * ("bh2"), x~_t -> x~_{t-1}.  The forward a step runs anyway at the PREDICTED point x~_t also corrects that point before the next
 * prediction: one order more than vd_dpmpp_2m_sample with no further network call.  One UNet forward, then one fused pass (unipc_kernel):
 *   D_t    = as vd_dpmpp_2m_sample forms it (non-finite check, clamp or threshold, measurement projection); written to `pred_xstart`
 *   n      = min(count, num_timesteps - 1 - t): the steps behind this one, never more than the schedule has above t
 *   x^c_t  = c0 base + c1 D1 + c2 D2 + c3 D_t     the corrector for the move t+1 -> t, of order min(2, n);  n = 0: x^c_t = x~_t
 *   sample = p0 x^c_t + p1 D_t + p2 D1            the predictor t -> t-1, of order min(2, n + 1)
 *   state  <- (x^c_t, D_t, D1)
 * with the state read (base, D1, D2) = (x^c_{t+1}, D_{t+1}, D_{t+2}).  With lambda = log(ab / (1 - ab)) / 2, alpha = sqrt(ab),
 * sigma = sqrt(1 - ab), ab = alphas_cumprod, and for a move s -> u = s - 1: h = lambda_u - lambda_s, phi = e^-h - 1 = B,
 * r = (lambda_{s+1} - lambda_s) / h (negative):
 *   corrector, order 1:  x^c_u = (sigma_u/sigma_s) base - alpha_u phi D1 - alpha_u B (D_u - D1) / 2
 *   corrector, order 2:  x^c_u = (sigma_u/sigma_s) base - alpha_u phi D1 - alpha_u B [rho1 (D2 - D1) / r + rho2 (D_u - D1)],
 *                        rho1 + rho2 = g1 / B, r rho1 + rho2 = 2 g2 / B, g1 = phi / (-h) - 1, g2 = g1 / (-h) - 1/2
 *   predictor:           x~_u  = (sigma_u/sigma_s) x^c_s - alpha_u phi D_s - [order 2] alpha_u B (D_{s+1} - D_s) / (2 r)
 * (the published multistep_uni_pc_bh_update; the order-2 predictor is vd_dpmpp_2m_sample's update).  At t = 0 the predictor row is
 * (0, 1, 0): sample = D_0, nothing infinite.
 * vd_set_unipc_rows uploads the coefficients, host_rows [14][num_timesteps] float32 (computed in float64, cast elementwise): rows
 * 0-3 c0..c3 at order 1 (c2 = 0), 4-7 c0..c3 at order 2, 8-10 p0..p2 at order 1 (p2 = 0), 11-13 p0..p2 at order 2, each at the index t
 * the step runs at.  Rows that do not exist are zero and never selected: any corrector at t = num_timesteps - 1, the order-2 corrector at
 * t > num_timesteps - 3, the order-2 predictor at t = num_timesteps - 1.  The table belongs to the schedule as the multistep weight row
 * does: the bound schedule's length, dropped by vd_set_schedule, and the sampler fails by name without it.
 * State: base / d1 / d2 are read (all three, or all NULL = no state: count must be 0), base_out / d1_out / d2_out written (all three, or
 * all NULL = not kept); the tensors written may be the tensors read (in place) and sample may be x: an element is read and then
 * written by one thread.  count = the steps the chain has finished (0: a chain's first step, first-order, no corrector).  No noise is
 * read, no Philox draw consumed.  A t[b] outside the schedule poisons every output of item b, the state written included, and reads no
 * table; a network output that is not finite leaves as NaN and sets bit 1 of the device flags.  Refused together with a known region
 * (vd_set_known_region), by name: the corrector rebuilds the state from `base`, a merge behind the pass would be discarded.
 * pred_xstart and eps may be NULL.  Meant for steps uniform in lambda ('logsnrN') and not too few: at h near 1 (logsnr10) the
 * corrector makes the result worse than vd_dpmpp_2m_sample's.
 * vd_unipc_from_xstart: the same pass on a caller's x_0 prediction, no network -- the `denoised_fn` form.  ANY per_sample and alignment
 * are served: 16-byte accesses where per_sample % 4 == 0 and every tensor is 16-byte aligned, element by element otherwise (same values). */
int vd_set_unipc_rows(vd_engine* e, int num_timesteps, const float* host_rows);
int vd_unipc_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask,
                    const float* kinda_marg_mask, const long long* frame_indices, const long long* t, const float* base,
                    const float* d1, const float* d2, int count, int observed_frames, int clip_denoised, float* sample,
                    float* pred_xstart, float* base_out, float* d1_out, float* d2_out, float* eps, void* stream);
int vd_unipc_from_xstart(vd_engine* e, int B, long long per_sample, const float* x, const float* xstart_in, const float* base,
                         const float* d1, const float* d2, int count, const long long* t, int clip_denoised, float* sample,
                         float* pred_xstart, float* base_out, float* d1_out, float* d2_out, void* stream);

/* diffusion.p_mean_variance(model, x, t, clip_denoised, model_kwargs) (gaussian_diffusion.py:229-372): one UNet forward,
 * then 'pred_xstart' (clipped) and 'mean' = posterior mean of it; 'variance' / 'log_variance' are the schedule rows
 * VD_TAB_LOGVAR at t (the host mirror broadcasts them).  Any of mean / pred_xstart / eps may be NULL. */
int vd_p_mean_variance(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask,
                       const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                       const long long* t, int observed_frames, int clip_denoised, float* mean, float* pred_xstart,
                       float* eps, void* stream);

/* The NLL path of scripts/video_nll.py.  vd_vb_terms = GaussianDiffusion._vb_terms_bpd (gaussian_diffusion.py:750-790;
 * losses.py normal_kl / discretized_gaussian_log_likelihood) plus the two per-step MSEs of calc_bpd_loop_subsampled
 * (:975-990), given the eps of a forward pass at x_t: vb[B] = KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) in bits per dim,
 * or the discretised decoder NLL where t == 0; xstart_mse[B] = mean((pred_xstart - x_start)^2); mse[B] =
 * mean((eps_from_xstart - noise)^2) (needs `noise`).  latent_mask: [B*T] or NULL; as in the reference's
 * mean_flat(tensor, mask) the mask multiplies and the mean still runs over all elements.  vd_prior_bpd = _prior_bpd (:909-926).
 * With vd_set_model_mean_type(1) (predict_xstart=True) `eps` is the network output as vd_p_mean_variance returns it, i.e. the x_0
 * prediction itself: pred_xstart = clamp(eps) and the eps of the second MSE is derived from it (_predict_eps_from_xstart, :392-396). */
int vd_vb_terms(vd_engine* e, int B, int T, const float* x_start, const float* x_t, const float* eps, const float* noise,
                const long long* t, int clip_denoised, const float* latent_mask, float* vb, float* xstart_mse, float* mse,
                float* pred_xstart, void* stream);
int vd_prior_bpd(vd_engine* e, int B, int T, const float* x_start, const float* latent_mask, float* out, void* stream);

/* The observed-frame search of scripts/video_optimal_schedule.py (:142-206,222-354).  One candidate evaluation there is
 * run_bpd_evaluation at ONE timestep per batch item, of which the search reads `mse` only.  vd_score_windows is that evaluation:
 *   noise    element j of item b = element j of vd_randn(out, per, seed, item_offset[b]) (per = T*3*H*W; item_offset: B Philox
 *            block offsets in DEVICE memory), or `noise` [B][per] when it is non-NULL (the form tests use);
 *   x_t      q_sample(x_start, t[b], noise), into engine-owned step memory;
 *   forward  one UNet forward at x_t in observed_frames = 'x_0' mode with obs_src = x_start, as vd_p_mean_variance launches it;
 *   mse_out  [B] float64 (device): sum over the frames with latent_mask != 0 of (eps' - noise)^2 * latent_mask, divided by ALL
 *            T*3*H*W elements (mean_flat(tensor, mask)); pred_xstart as in vd_vb_terms (EPSILON / START_X, the non-finite check
 *            before the clamp, bit 1 of the device flags), eps' = (sqrt_recip x_t - pred_xstart) / sqrt_recipm1
 *            (_predict_eps_from_xstart, gaussian_diffusion.py:392-396).  fp64 partial sums per block folded in a fixed order: the
 *            same call gives the same bits.  A t[b] outside the schedule gives NaN for item b and sets bit 0 of the device flags;
 *            frames in neither mask contribute nothing; an item without a latent frame scores 0.
 * suffix_skip = 1: under the conditions of the window suffix skip (cond_emb_type 'channel', an attention layer) everything behind
 * the last attention layer runs on the frames with latent_mask = 1 only -- the only frames the score reads; their eps, and so
 * mse_out, are those of suffix_skip = 0 bit for bit.  The number of such frames shapes the launches, so this form reads
 * latent_mask back first (B*T floats, one wait for `stream` before anything is enqueued); suffix_skip = 0 never waits.
 * vd_op_eps_mse: the reduction alone on a given network output `eps` [B][per] (test entry, like the vd_op_* below). */
int vd_score_windows(vd_engine* e, int B, int T, const float* x_start, const float* obs_mask, const float* latent_mask,
                     const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int clip_denoised,
                     unsigned long long seed, const unsigned long long* item_offset, const float* noise, int suffix_skip,
                     double* mse_out, void* stream);
int vd_op_eps_mse(vd_engine* e, int B, int T, const float* x_start, const float* eps, const long long* t, int clip_denoised,
                  const float* latent_mask, unsigned long long seed, const unsigned long long* item_offset, const float* noise,
                  double* mse_out, void* stream);

/* Window executor -- the loop of scripts/video_sample.py:149-168 (`for timestep in reversed(range(num_timesteps)):
 * local = diffusion.p_sample(model, local, t, ...)['sample']`) with the loop state on the device: the respaced index
 * t[B] and the Philox {seed, offset} live in engine-owned device memory, ONE hipGraph holds a whole step (t -> t_model,
 * UNet forward, posterior update of x IN PLACE, t -= 1, offset += B*T*3*H*W) and is captured once per window signature
 * (B, T, the six tensor addresses, observed_frames, sampler, clip, eta), so a window costs num_timesteps graph launches
 * instead of ~330 kernel launches per step from the host (BASELINE configs[4]: two signatures, Tw = 20 and Tw = 14).
 * vd_window_begin arms the counters (and captures if the signature is new: one eager forward, then the capture; `stream`
 * must not be the default stream); vd_window_run replays n_steps steps t_start, t_start-1, ...; x holds the result.
 * observed_frames: 0 x_0, 1 x_t, 2 x_t_minus_1 as p_sample_loop runs it (obs_src = the CLEAN frames, re-noised to t - 1 inside
 * every step from the second half of the step's Philox range, gaussian_diffusion.py:565-568), 3 x_t_minus_1 with obs_src read as it
 * is at every step (a direct p_sample caller: scripts/video_sample.py:149-166 hands x0).  Noise is always the in-kernel Philox stream (seed, offset + step*B*per + i):
 * identical to vd_p_sample(noise = NULL, seed, offset + step*B*per).
 * sampler: 0 p_sample, 1 ddim_sample, 2 ddim_reverse_sample (gaussian_diffusion.py:636-668).  Sampler 2 walks UPWARDS: t_start is
 * the first index, the captured step ends in its sampler pass in place and t += 1, the Philox counter does not move (seed, offset
 * and eta are not read), and vd_window_run refuses a run that would pass num_timesteps - 1.  It serves observed_frames 0, 1 and 3;
 * 2 needs noise inside the graph and is refused.  The prefix cache and the suffix skip apply to it unchanged.
 * Sampler 3 is dpmpp_2m_sample (above): it walks downwards like 0 and 1, the captured step ends in its sampler pass in place, the
 * history D_prev lives in an engine-owned buffer of B*T*3*H*W floats that the pass updates in place, and a device word counting the
 * window's finished steps tells the pass whether there is history -- so ONE graph serves a window's first step (first-order whatever
 * t_start is) and its later ones, and a second window on the same graph starts without history again.  No Philox draws (seed, offset
 * and eta are not read); observed_frames 2 is refused as for sampler 2; without a weight row (vd_set_multistep_weights) it fails
 * with a message that says so.  The prefix cache and the suffix skip apply unchanged.
 * Sampler 4 is dpmpp_2m_sde_sample (above): history AND noise state live in the graph -- the history buffer and step count of sampler 3,
 * the Philox pair of samplers 0 and 1 (offset += B*T*3*H*W per step; element i of step k is vd_randn's at (seed, offset + k*B*per)).
 * It serves observed_frames 0 to 3 as sampler 1 does; eta is not read (and is no part of its signature); vd_window_jump drops its
 * history; the prefix cache and the suffix skip apply as for sampler 3; without a weight row it fails by name.
 * Sampler 5 is unipc_sample (above): its three state tensors live in engine-owned buffers of B*T*3*H*W floats each (sampler 3's history
 * buffer and two more) that the pass updates in place, and the device word counting the window's finished steps picks the order of both
 * moves -- so ONE graph serves a window's first step (no corrector, first-order predictor, whatever t_start is), its second and its later
 * ones, and a second window on the same graph starts without state again.  The window tensor at index t holds the predicted x~_t.  No
 * Philox draws (seed, offset and eta are not read); observed_frames 2 is refused as for sampler 3; a known region and vd_window_jump are
 * refused by name; without its rows (vd_set_unipc_rows) it fails by name.  The prefix cache and the suffix skip apply unchanged. */
int vd_window_begin(vd_engine* e, int B, int T, float* x, const float* obs_src, const float* obs_mask,
                    const float* latent_mask, const float* kinda_marg_mask, const long long* frame_indices,
                    int observed_frames, int sampler, int clip_denoised, float eta, unsigned long long seed,
                    unsigned long long offset, long long t_start, void* stream);
int vd_window_run(vd_engine* e, int n_steps, void* stream);
/* Bumped by every vd_window_begin.  The step counters are one set per engine: a host object that armed a window keeps the
 * value it saw and refuses to run when another begin has happened since (executor.py).  vd_window_run itself fails with
 * "window graphs invalidated" when the armed window's graph was dropped (workspace growth, vd_set_schedule). */
unsigned long long vd_window_generation(vd_engine* e);
int vd_window_graphs(vd_engine* e);            /* captured graphs held by the engine */
/* What the armed window carries from step to step, copied out on `stream` (device to device, B*T*3*H*W floats each; every pointer
 * optional): `hist` -- the previous step's x_0 prediction of samplers 3 and 4, UniPC's D_{t+1} -- and UniPC's corrected state
 * x^c_{t+1} (`ubase`) and D_{t+2} (`ud2`).  Meaningful behind the window's first step; B and T are the armed window's; a sampler
 * without history, and `ubase` / `ud2` for any sampler but 5, are refused by name.  Reads only: nothing of the window changes. */
int vd_window_history(vd_engine* e, int B, int T, float* hist, float* ubase, float* ud2, void* stream);

/* Window prefix cache (opt-in, off by default; a host-side choice like the executor itself).  The reference recomputes the
 * whole UNet for every frame at every step (unet.py:838-846).  Before the first attention layer the network treats frames as
 * independent batch entries (input_blocks 0 .. first attention block - 1: ResBlocks / Downsample, per-frame GroupNorm), and in
 * 'x_0' mode with the default cond_emb_type='channel' an OBSERVED frame's input there never changes during a window: its x0
 * pixels, the indicator channels and the timestep-0 embedding (unet.py:991-1013).  With the cache on, vd_window_begin runs
 * those blocks for the observed frames (obs_mask = 1, latent_mask = 0) once, into persistent full-size tensors, and the
 * captured step runs them on the remaining frames only (a compact batch), scatters each block output and its GroupNorm
 * partial sums beside the cached rows and continues with the full batch (attention, decoder skips).  Same arithmetic per
 * frame; the GroupNorm partial sums of a tensor are folded in a different (fp64) grouping.  The set of cached frames is part
 * of the graph signature.  vd_window_prefix_frames: how many frames of the armed window are served from the cache. */
int vd_set_window_prefix_cache(vd_engine* e, int on);
int vd_window_prefix_frames(vd_engine* e);

/* Window suffix skip (opt-in, off by default; the sibling of the prefix cache at the other end of the network).  Behind its
 * LAST attention layer the UNet treats frames as independent batch entries again -- the remaining decoder ResBlocks, the
 * Upsample convs and the output head (unet.py:820-839) -- and the caller of a window keeps only its latent frames
 * (scripts/video_sample.py:170-186), while a purely observed frame (obs_mask = 1, latent_mask = 0) re-enters the network as
 * the observation whatever the step wrote to it (unet.py:958-983: observed_frames 'x_0' and 'x_t_minus_1' with
 * cond_emb_type='channel'; NOT 'x_t', where its input is its own running sample).  With the skip on, the captured step
 * gathers every other frame out of the last attention layer's output and out of the skip tensors the remaining blocks read
 * (rows and GroupNorm partial sums), runs those blocks and the head on that compact batch with the kernel variants the full
 * batch would get, and writes eps = 0 for the skipped frames: every frame that is not a pure observation receives the eps
 * -- and so the sample -- of the full step, bit for bit; the skipped frames' entries of the window tensor are meaningless.
 * vd_window_suffix_frames: frames the suffix of the armed window runs on (0: all of them -- skip off or nothing to skip). */
int vd_set_window_suffix_skip(vd_engine* e, int on);
int vd_window_suffix_frames(vd_engine* e);

/* cfg_scale: classifier-free guidance on the observed frames -- this project's extension (the reference samples at w = 1 only).  The
 * model is trained on every split of a window into observed and latent frames, the empty observed set included, so one set of weights
 * gives both branches.  For a step on (x, t, obs_mask, latent_mask, kinda_marg_mask, frame_indices, observed_frames) and w = cfg_scale:
 *   out_c = the network output of the step as it runs at w = 1
 *   out_u = the network output of the same call with obs_mask := 0 and nothing else changed: the formerly observed frames become
 *           padding frames (unet.py:953-983: fed x (1 - anything_mask), masked out of temporal attention)
 *   d     = out_c - out_u            one fp32 subtraction
 *   out_g = fmaf(w, d, out_u)        one fused multiply-add;  NaN where d is not finite;  out_u itself at w = 0
 * and out_g takes the place of the network output in front of the unchanged sampler pass (eps, or x_0 for predict_xstart=True: the
 * combination is linear).  Engine state like the two window switches; default 1; a w that is not finite is refused.
 * w == 1 is the step as it was: one forward, no combine pass.  Every other w (0 and negative values included) costs a second forward:
 * both run at batch B, one after the other, in the same workspace arena; out_u goes to a second engine-owned output buffer, the zero mask is
 * an engine-owned B*T buffer, one noise draw per step as before (the Philox offsets of a window do not depend on w), and in a window with
 * observed_frames = 2 the observation is re-noised once per step.
 * Honoured by vd_p_sample, vd_ddim_sample, vd_ddim_reverse_sample, vd_dpmpp_2m_sample, vd_p_mean_variance (whose `eps` output is then
 * out_g) and vd_window_begin / vd_window_run: the weight is part of a captured graph's signature, so a later vd_window_begin under
 * another w captures (or finds) another graph.  NOT honoured by vd_unet_forward, vd_guided_step, vd_score_windows, vd_vb_terms /
 * vd_prior_bpd (the NLL path scores the conditional model) and the vd_*_from_xstart / vd_posterior_update passes, which run no network;
 * vd_dps_step fails by name while w != 1.
 * With w != 1, vd_window_begin fails while the prefix cache or the suffix skip is switched on (in the unconditional forward the
 * observed frames are padding whose content is whatever the window tensor holds: neither invariant nor meaningless), and a step fails
 * while an attention capture (vd_set_attn_capture) is armed.
 * vd_op_cfg_combine: the pass alone, any n > 0, no engine; out may be out_c or out_u; tensors that are not all 16-byte aligned run element
 * by element. */
int vd_set_cfg_scale(vd_engine* e, float w);
float vd_cfg_scale(vd_engine* e);
int vd_op_cfg_combine(const float* out_c, const float* out_u, float w, long long n, float* out, void* stream);

/* FreeU -- this project's extension (Si, Huang, Jiang, Liu: "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024): the one option that acts
 * INSIDE the UNet forward.  Decoder levels count from the bottom: stage 1 is the first num_res_blocks + 1 output blocks (lowest
 * resolution) with the constants (b1, s1), stage 2 the next num_res_blocks + 1 with (b2, s2).  Every model vd_create builds has both:
 * the level count follows the image size, four to six levels (vd_freeu_stages() == 2; a topology of one level, which cannot be created
 * today, would have stage 1 alone).  Every output block of a stage reads cat([h', skip']) in the place of
 * cat([h, skip]), h and skip being N frames of S x S pixels, channels-last:
 *   skip' (the skip filter): per frame and channel, with theta = 2 pi / S and x the S x S plane,
 *     x'[i,j] = x[i,j] + (s - 1)/S^2 (m0 + ci cos(theta i) + si sin(theta i) + cj cos(theta j) + sj sin(theta j)
 *                                        + cd cos(theta (i+j)) + sd sin(theta (i+j))),
 *     m0 = sum x, (ci, si) = sum x[i',j'] (cos, sin)(theta i'), (cj, sj) the same in j', (cd, sd) the same in i' + j'
 *     = Re ifft2(M . fft2(x)) with M = s on the four bins (u, v) in {0, S-1}^2 and 1 elsewhere: the published code's fftshift box
 *     [S/2 - 1 : S/2 + 1]^2 at threshold 1 with .real taken.  The threshold is fixed at 1.
 *   h' (the backbone scale): with H = C_h / 2, channels c >= H are copied; for c < H
 *     plain:    h' = (float)b * h, one fp32 multiply;
 *     adaptive: h' = h ((b - 1) g + 1), g = (m - lo)/(hi - lo), m[n,p] the mean of h[n,p,:] over ALL C_h channels, lo and hi its
 *               minimum and maximum over the pixels of frame n (the paper's structure-aware form).  hi == lo gives g = 0, where the
 *               published code divides 0 by 0.
 * The seven sums, the mean, min / max, g, the factor and the update are fp64 in a fixed order without atomics, the result is rounded once
 * to fp32: two runs on equal inputs give equal bits.  The cos / sin tables of the two sides are computed on the host in double and
 * uploaded by the first vd_set_freeu that switches the option on.  h' and skip' go to engine-owned buffers (one pair, reused block after
 * block; never in place: a skip tensor may outlive the step), and so do their GroupNorm partial sums, one statistics pass over each
 * modified half: FreeU takes nothing from the step's workspace, whose size does not depend on it.
 * vd_set_freeu: all four constants must be finite and > 0; all four equal to 1 = off (the default): no launch is added and every entry
 * is the one it was, to the bit.  Otherwise a stage with b == 1 adds no backbone launch and one with s == 1 no filter launch; per block
 * the plain form adds up to 2 launches, the adaptive form up to 3 (the structure map is a launch of its own).
 * Honoured by every untaped forward: vd_unet_forward, vd_p_mean_variance, the step entries (vd_p_sample, vd_ddim_sample,
 * vd_ddim_reverse_sample, vd_dpmpp_2m_sample, vd_dpmpp_2m_sde_sample, vd_unipc_sample) -- both forwards of a cfg_scale step -- and
 * vd_window_begin / vd_window_run, where the constants are part of a captured graph's signature.  Refused by name while it is on:
 * vd_guided_step, vd_dps_step, vd_deblur_step, vd_linear_dps_step, vd_guide_begin, vd_eps_vjp and vd_ode_nll_eval (the taped forward
 * does not run the passes), vd_score_windows and vd_vb_terms (the search and the NLL score the model as trained), and vd_window_begin
 * while the prefix cache or the suffix skip is switched on.
 * vd_freeu: returns 1 while on, 0 while off; consts (4 doubles: b1, b2, s1, s2) and adaptive may be NULL.
 * vd_op_freeu_filter / vd_op_freeu_backbone: the passes alone on [N][S*S][C] tensors, C % 4 == 0, 16-byte aligned, y != input, no
 * engine; they allocate their table / scratch, wait for `stream` and free it.  s == 1 copies the input bits; the filter needs S >= 2
 * (at one pixel the four bins coincide, and the published box is empty). */
int vd_set_freeu(vd_engine* e, double b1, double b2, double s1, double s2, int adaptive);
int vd_freeu(vd_engine* e, double* consts, int* adaptive);
int vd_freeu_stages(vd_engine* e);
int vd_op_freeu_filter(const float* x, int N, int S, int C, double s, float* y, void* stream);
int vd_op_freeu_backbone(const float* h, int N, int S, int C, double b, int adaptive, float* y, void* stream);

/* Guidance rescale and dynamic thresholding -- this project's extensions; the two standard remedies for the over-saturation of
 * cfg_scale > 1 under the static clamp of x_0 to [-1, 1].  "Item" is one batch element, and each statistic below runs over the elements of
 * the item's LATENT frames only (latent_mask == 1); observed and padding frames keep the bits of the step without the option.
 *
 * guidance_rescale phi in [0, 1] (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", 3.4); 0 = off (default);
 * acts only with cfg_scale != 1.  With out_g the bits of the combine pass above:
 *   sigma_c, sigma_g = standard deviations about the mean of out_c and out_g over the item's latent elements (fp64 sums, block partials
 *                      folded in a fixed order, no floating-point atomics: run-to-run deterministic)
 *   f = 1 + phi (sigma_c / sigma_g - 1)   in fp64, rounded once to fp32;  f = 1 where sigma_g = 0 or the item has no latent frame
 *   latent frames: out_g * f (one fp32 product);  other frames: out_g
 * It acts on the network output, whichever of eps and x_0 the model predicts.  Two passes in place of the combine pass.
 *
 * dynamic_threshold p in (0, 1] (Saharia et al. 2022, Imagen, 2.3); 0 = off (default); acts only with clip_denoised, whose clamp it
 * replaces; independent of cfg_scale.  x_0 is the prediction as the step forms it (the network output of a START_X model):
 *   n = the item's latent elements, a = sorted |x_0|, h = (n - 1) (double)p, k = floor(h)
 *   s = a[k] + (h - k) (a[min(k + 1, n - 1)] - a[k])   in fp64, rounded once to fp32 (torch.quantile's linear interpolation);  s <- max(s, 1)
 *   latent frames: clamp(x_0, -s, s) / s;  other frames: clamp(x_0, -1, 1) as before
 * a[k] and a[k + 1] are exact: a radix select over the bit patterns of |x_0| (four histogram passes, integer atomics, counters zeroed in the
 * stream by a kernel).  A latent x_0 that is not finite turns the item's latent x_0 into NaN and sets VD_ERR_NONFINITE.  Where max |x_0| <= 1 on
 * an item's latent frames, s = 1 and the step is the clamped step to the bit.  The finished x_0 goes to an engine-owned buffer and the
 * sampler pass runs in the form the vd_*_from_xstart entries expose, with its clamp off.
 *
 * Both are engine state like cfg_scale, part of a window graph's signature, and use the step's tail of the workspace
 * (vd_workspace_bytes counts it): no allocation, no host round trip.  Honoured by the entries that honour cfg_scale (vd_p_sample,
 * vd_ddim_sample, vd_ddim_reverse_sample, vd_dpmpp_2m_sample, vd_p_mean_variance, vd_window_begin / vd_window_run) and NOT honoured by
 * vd_unet_forward, vd_guided_step (use_gradient_method), vd_score_windows, vd_vb_terms / vd_prior_bpd (the NLL path) and the
 * vd_*_from_xstart / vd_posterior_update passes; vd_dps_step fails by name while either is set.  vd_window_begin fails while an option that would act is set together with the prefix
 * cache or the suffix skip.  A caller's denoised_fn together with dynamic_threshold is refused on the Python side.
 * vd_op_cfg_rescale / vd_op_dynamic_threshold: the passes alone on [B][T][frame_elems] tensors with the [B*T] latent mask `lat`, no engine;
 * they allocate their scratch, wait for `stream` and free it.  out may alias an input; frame_elems % 4 != 0 or tensors that are not 16-byte
 * aligned run element by element.  factor_out[B] = f;  s_out[B] = max(s, 1), NaN for a poisoned item, 1 for an item without latent frame. */
int vd_set_guidance_rescale(vd_engine* e, float phi);
float vd_guidance_rescale(vd_engine* e);
int vd_set_dynamic_threshold(vd_engine* e, float p);
float vd_dynamic_threshold(vd_engine* e);
int vd_op_cfg_rescale(const float* out_c, const float* out_u, float w, const float* lat, int B, int T, long long frame_elems, float phi,
                      float* out, float* factor_out, void* stream);
int vd_op_dynamic_threshold(const float* x0, const float* lat, int B, int T, long long frame_elems, float p, float* out, float* s_out,
                            void* stream);

/* Known region: pixel-mask inpainting -- this project's extension (RePaint, Lugmayr et al. 2022; the reference conditions on whole frames
 * only).  It needs no weights of its own: after every reverse step the known pixels of the LATENT frames are overwritten with the known
 * content noised to the level the step just reached, and a caller may walk the chain a few steps back up and down again ("resampling")
 * so that the generated part harmonises with the known part.  No claim about sample quality is made here: that depends on the checkpoint.
 *   known_src  [B][T][3][H][W] float32, the known content (clean, in the model's [-1, 1] space)
 *   known_mask [B][T][H][W] float32, broadcast over the three channels; a pixel is known where the mask is != 0
 * The merge pass (csrc/known.hip: known_merge_kernel), for a step at respaced index t[b] that produced `sample`, in place:
 *   an element is merged iff its frame has latent_mask == 1 and its pixel is known; every other element keeps the bits of the step
 *   (observed and padding frames are never touched);
 *   t >= 1: sample = fmaf(sqrt_one_minus_alphas_cumprod[t-1], z, sqrt_alphas_cumprod[t-1] * known_src) = q_sample(known_src, t - 1, z)
 *           in vd_q_sample's rounding order;   t == 0: sample = known_src, bit for bit;
 *   z = known_noise[i] (explicit, [B][T][3][H][W]), or element i of the Philox stream (seed, offset + B*per/4), per = T*3*H*W, integer
 *       division.  Philox layout of a step's range of B*per blocks: the sampler noise uses blocks [0, B*per/4), the merge
 *       [B*per/4, B*per/2), the 'x_t_minus_1' re-noise of a window [B*per/2, 3*B*per/4);
 *   a t[b] outside the schedule turns every element of item b into NaN, as the sampler pass did; the merge sets no error bit of its own.
 * vd_set_known_region: engine state like cfg_scale; the caller's device tensors, which must stay alive and of the shape of the steps that
 * follow; NULL known_src and known_mask clear it (both or neither); known_noise may be NULL.  vd_known_region: 1 while set, else 0.
 * Honoured by vd_p_sample, vd_ddim_sample, vd_dpmpp_2m_sample and vd_window_begin / vd_window_run: the merge runs on `sample` right behind
 * the sampler pass; pred_xstart and eps stay the model's own.  vd_ddim_reverse_sample (and sampler 2 in a window) fails by name while it is
 * set: the merge noises to t - 1.  NOT honoured by vd_unet_forward, vd_p_mean_variance (it has no sample), vd_guided_step, vd_score_windows,
 * vd_vb_terms / vd_prior_bpd and the vd_*_from_xstart / vd_posterior_update passes; vd_dps_step fails by name while it is set.  It composes with cfg_scale, guidance rescale and
 * dynamic thresholding: they act before or inside the sampler pass, the merge behind it.
 * In a window the two addresses are part of the graph's signature; known_noise must be NULL: the draws come from the window's own Philox
 * pair at offset + B*per/4, and EVERY sampler's captured step then advances the counter by B*per -- sampler 3 (dpmpp_2m_sample) included,
 * which otherwise draws nothing.  vd_window_begin fails by name while the prefix cache or the suffix skip is on together with a known
 * region (the merge touches latent frames only, so they are compatible in principle; not built).
 * vd_known_merge: the pass alone on frames of frame_pixels = H*W pixels (any value; the engine's image size is not read), no network, like
 * vd_posterior_update.  Four elements per thread while frame_pixels % 4 == 0 and the tensors are 16-byte aligned, else element by element.
 *
 * vd_q_jump: one forward diffusion step x_{t-1} -> x_t at index t[b] (csrc/known.hip: q_jump_kernel), out = x allowed: on the frames with
 * latent_mask == 1 (all pixels) out = fmaf(sqrt_beta[t], z, sqrt_alpha[t] * x); other frames keep their bits; z = noise[i] or element i of
 * the Philox stream (seed, offset) -- blocks [0, B*per/4) of a range of its own; a t[b] outside the schedule gives NaN for item b.
 * vd_set_jump_rows uploads sqrt_alpha = sqrt(1 - betas) and sqrt_beta = sqrt(betas) of the bound (respaced) schedule, float32 casts of the
 * float64 values (1 - alpha in fp32 would lose three digits at beta = 1e-4; the VD_NTAB-row table is public layout).  The rows belong to the
 * schedule: vd_set_schedule drops them, and a jump without them fails with a message that says so.
 * vd_window_jump: n times on the armed window, as plain launches on `stream` (not captured): t += 1; a jump of the window tensor at the new
 * t from the device's {seed, offset}; offset += B*per; the count of finished steps returns to 0, so a dpmpp_2m window's next step is
 * first-order again.  It extends the window's remaining-step count by n and refuses a jump past num_timesteps - 1, sampler 2, and a window
 * without a known region. */
int vd_set_known_region(vd_engine* e, const float* known_src, const float* known_mask, const float* known_noise,
                        unsigned long long seed, unsigned long long offset);
int vd_known_region(vd_engine* e);
int vd_known_merge(vd_engine* e, int B, int T, long long frame_pixels, float* sample, const float* known_src, const float* known_mask,
                   const float* latent_mask, const long long* t, const float* known_noise, unsigned long long seed,
                   unsigned long long offset, void* stream);
int vd_set_jump_rows(vd_engine* e, int num_timesteps, const float* sqrt_alpha, const float* sqrt_beta);
int vd_q_jump(vd_engine* e, int B, int T, long long frame_pixels, const float* x, const float* latent_mask, const long long* t,
              const float* noise, unsigned long long seed, unsigned long long offset, float* out, void* stream);
int vd_window_jump(vd_engine* e, int n, void* stream);

/* Measurement: zero-shot restoration -- this project's extension (DDNM, Wang, Yu, Zhang 2022: the range/null-space projection
 * x_0 <- x_0 + A^+(y - A x_0) applied to the x_0 prediction of every step; the reference has nothing like it).  It needs no weights of its
 * own and conditions on a DEGRADED copy of the video, where the known region conditions on known pixels.  No claim about restoration
 * quality is made here: what is pinned is the arithmetic.
 * One operator family, "cell mean".  A cell is scale x scale pixels of one channel plane (gray = 0) or of the three planes of its frame
 * (gray = 1, channel weights 1/3 each).  A = the mean over every cell: y [B][T][Cy][H/scale][W/scale] float32, Cy = 3, or 1 with gray.
 * A^+ replicates a cell's value over its cell, so A A^+ = I.  Served: scale 2, 4, 8 with either gray value and scale 1 with gray = 1
 * (super-resolution, colourisation, both); H and W must be divisible by scale.
 * The pass (csrc/measure.hip: measurement_project_kernel), one launch, on the frames with latent_mask == 1 only: every element of a cell
 * becomes x_0 + (y_cell - mean_cell(x_0)), mean_cell = sum / n with the sum in a fixed order (no atomics: item b of a batch has the bits of
 * the call on item b alone) -- |out - exact| <= gamma_n mean_cell|x_0| + u |y - m| + u |out|, n the cell's size, u = 2^-24; other frames
 * keep the unprojected x_0.  A cell that holds a value that is not finite comes out not finite in every element.
 * vd_set_measurement: engine state like cfg_scale; y is the caller's device tensor, which must stay alive and of the shape of the steps
 * that follow; NULL clears it.  vd_measurement: 1 while set, else 0; the scale and gray flag through the two pointers (either may be NULL).
 * Honoured by vd_p_sample, vd_ddim_sample, vd_dpmpp_2m_sample, vd_p_mean_variance and vd_window_begin / vd_window_run.  Order inside a
 * step: network (both forwards and the combine or rescale pass of cfg_scale), x_0 with the clamp of clip_denoised or the dynamic
 * threshold in its place, the projection, then the sampler pass on the projected x_0 with its clamp off -- pred_xstart, the mean and
 * dpmpp_2m's history are the projected x_0, and at t == 0, where every sampler returns x_0, A(sample) = y up to rounding on the latent
 * frames.  With no measurement set a step launches exactly what it launched before.
 * Fails by name: vd_ddim_reverse_sample (sampler 2 in a window), vd_guided_step (use_gradient_method), vd_dps_step, a window with the prefix cache or
 * the suffix skip on, and a measurement together with a known region (vd_set_known_region; not built).  NOT honoured by vd_unet_forward,
 * vd_score_windows, vd_vb_terms / vd_prior_bpd and the vd_*_from_xstart / vd_posterior_update passes.
 * In a window y's address, scale and gray are part of the graph's signature: one graph per (signature, scale, gray).
 * vd_measurement_project: the projection alone, in place on an x_0 handed in, on frames of H x W (any size; the engine's image size is
 * not read), no network and no clamp.  16-byte accesses while W % 4 == 0 and x0_inout is 16-byte aligned, else element by element: same bits. */
int vd_set_measurement(vd_engine* e, const float* y, int scale, int gray);
int vd_measurement(vd_engine* e, int* scale, int* gray);
int vd_measurement_project(vd_engine* e, int B, int T, int H, int W, float* x0_inout, const float* y, const float* latent_mask, int scale,
                           int gray, void* stream);

/* The posterior arithmetic alone, given eps (same formulas; mode 0 p_sample, 1 ddim). */
int vd_posterior_update(vd_engine* e, int mode, int B, long long per_sample, const float* x, const float* eps,
                        const long long* t, int clip_denoised, float eta, const float* noise,
                        unsigned long long seed, unsigned long long offset, float* sample, float* pred_xstart,
                        void* stream);

/* process_xstart with a caller-supplied `denoised_fn` (gaussian_diffusion.py:319-324): the host takes the unclipped
 * pred_xstart (vd_p_mean_variance, clip_denoised = 0), applies its function, and hands the result back here; the clamp,
 * q_posterior_mean_variance (:208-227) and the noise add (:438-443; ddim: eps re-derived from x_0, :597-634) run as in
 * vd_posterior_update.  Any of sample / pred_xstart / mean may be NULL. */
int vd_posterior_from_xstart(vd_engine* e, int mode, int B, long long per_sample, const float* x, const float* xstart_in,
                             const long long* t, int clip_denoised, float eta, const float* noise,
                             unsigned long long seed, unsigned long long offset, float* sample, float* pred_xstart,
                             float* mean, void* stream);

/* return_attn_weights (unet.py:457-466,799-836; gaussian_diffusion.py:277,496): per attention block the softmax weights
 * averaged over the heads, absolute value -- temporal (B*HW, T, T) and spatial (B*T, HW, HW) -- in execution order (input
 * blocks, middle, output blocks).  vd_attn_blocks / vd_attn_block_info size the buffers; vd_set_attn_capture arms the
 * capture for the following forwards (n = 0 clears it).  Two extra passes over q, k per block: the logging path.
 * vd_window_begin refuses by name while a capture is armed: a captured step would bake the buffers' addresses in. */
int vd_attn_blocks(vd_engine* e);
int vd_attn_block_info(vd_engine* e, int i, int* resolution, int* channels);
int vd_set_attn_capture(vd_engine* e, float* const* temporal, float* const* spatial, int n);

/* use_gradient_method (gaussian_diffusion.py:264-271,350-364; scripts/video_sample.py:429 `--use_gradient_method`).
 * Windows of at most 32 frames (the backward kernels of temporal attention and GroupNorm); a longer T fails with a message
 * that names use_gradient_method and the limit.
 * The guidance needs d(loss)/d(x_t) through the whole UNet: backward-DATA only, no weight gradients.  Its matrix products
 * run on the forward kernels over a second packed image -- transposed linear weights, 180-degree-rotated transposed 3x3
 * kernels -- that exists only when asked for: vd_bwd_weights_bytes -> vd_set_bwd_weight_storage (device memory, or host
 * memory for a broadcast image) -> vd_load_weight_bwd per checkpoint tensor (a no-op for tensors the backward never reads).
 * vd_guided_step is p_mean_variance(..., use_gradient_method=True) (+ p_sample's noise add when `sample` is given):
 *   the network sees obs_mask := 0 and latent_mask := obs_mask + latent_mask; with the unguided mean / variance a sample
 *   x_{t-1} = mean + [t != 0] sigma_t * noise is drawn, loss = sum(((x_{t-1} - x_t_minus_1) * obs_mask)^2) is differentiated
 *   w.r.t. x, and mean' = mean - 10 * alpha_t * grad / 2.  Outputs (each may be NULL): mean', pred_xstart, grad,
 *   sample = mean' + [t != 0] sigma_t * noise2. */
long long vd_bwd_weights_bytes(vd_engine* e);
int vd_set_bwd_weight_storage(vd_engine* e, void* buf, long long bytes, int on_host);
int vd_load_weight_bwd(vd_engine* e, const char* name, const float* host_data, long long numel);
int vd_guided_step(vd_engine* e, int B, int T, const float* x, const float* obs_mask, const float* latent_mask,
                   const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int clip_denoised,
                   const float* x_t_minus_1, const float* noise, const float* noise2, float* mean, float* pred_xstart,
                   float* grad, float* sample, void* stream);

/* Diffusion posterior sampling for noisy measurements -- this project's extension (DPS: Chung, Kim, McCann, Klasky, Ye, ICLR 2023; the
 * reference has nothing like it).  Where a measurement (vd_set_measurement, DDNM) takes y = A x as exact and copies its noise into every
 * frame, DPS moves the sample of every reverse step down the gradient of rho_b = ||y - A x_0(x_t)||_2 with respect to x_t -- a derivative
 * through the whole UNet, on the backward-data pass of use_gradient_method (second packed image: vd_set_bwd_weight_storage).  No claim about
 * restoration quality is made here: what is pinned is the arithmetic.
 * The operators and y's layout are the measurement's ("cell mean": scale 2, 4, 8, or any of 1, 2, 4, 8 with gray); n_c = scale^2, with
 * gray 3 scale^2, is the number of elements of a cell.  Per item b, with L_b its frames with latent_mask == 1, for an epsilon model at t:
 *   1. eps: the taped forward of the window as the plain step runs it (the caller's masks and obs_mode; obs_src is a constant);
 *   2. x_0r = a x_t - b eps (a = sqrt_recip_alphas_cumprod[t], b = sqrt_recipm1_alphas_cumprod[t]; two rounded products, one
 *      subtraction), x_0 = clamp(x_0r, -1, 1) with clip_denoised -- the x_0 head of every sampler pass;
 *   3. r = y - A x_0 on the cells of the frames in L_b, 0 elsewhere; rho_b = sqrt(sum r^2): the sum in fp64 in a fixed order that does
 *      not depend on B (an item handed alone gives the same bits), rounded once to fp32; no floating-point atomics;
 *   4. q = -r_cell / (rho_b n_c) on every element of a cell (0 where rho_b == 0 or L_b is empty), q_r = q [-1 <= x_0r <= 1] with
 *      clip_denoised, d eps = -b q_r, d_x = a q_r: one fp32 rounding each (rho_b n_c is exact without gray);
 *   5. g = d_x + (d eps / d x_t)^T d eps: the backward-data pass on a power-of-two multiple of d eps, as vd_guided_step runs it;
 *   6. sample' and pred_xstart: the plain sampler pass (sampler 0 p_sample, 1 ddim_sample with eta) on (x_t, eps) with `noise` -- the
 *      bits of vd_p_sample / vd_ddim_sample with the same noise;
 *   7. sample = fmaf(-zeta, g, sample') on the frames of L_b; every other frame keeps the bits of sample'.
 * This is x_{t-1} = x'_{t-1} - zeta grad ||y - A x_0||_2 of the official implementation, per batch item.  zeta = 0 is the plain step.
 * Outputs: sample, pred_xstart; grad (g on every frame: 0 on observed frames, the network's own gradient on padding frames) and
 * residual_norm ([B], rho_b) may be NULL.  `noise` is explicit.  Plain launches on `stream`, no host wait; the workspace is the guided
 * step's (r and the partial sums lie in spare slots of its tail), and a plain step behind it has its usual bits.  A t[b] outside the
 * schedule poisons item b with NaN as the sampler pass does; a network output that is not finite sets VD_ERR_NONFINITE through it.
 * Fails by name: T above 32, a model that is not epsilon-prediction, a missing backward image, a sampler other than 0 or 1, zeta
 * negative or not finite, an operator that is not served or an image size not divisible by scale, and engine state that would act on
 * a plain step: cfg_scale != 1, guidance rescale, dynamic threshold, a known region, a measurement, an armed attention capture.
 * Not part of vd_window_begin / vd_window_run: eager steps only.
 * vd_op_dps_seed: steps 2-4 alone on a caller's (x_t, eps) on frames of H x W (any size; the engine's image size is not read), no network:
 * d_eps, d_x, rho ([B], may be NULL) and pred_xstart (x_0 of every frame, may be NULL).  It allocates its scratch, waits for `stream` and
 * frees it.  16-byte accesses while W % 4 == 0 and the tensors are 16-byte aligned, else element by element: same bits. */
int vd_dps_step(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask,
                const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int obs_mode, int clip_denoised,
                int sampler, float eta, const float* noise, const float* y, int scale, int gray, float zeta, float* sample,
                float* pred_xstart, float* grad, float* residual_norm, void* stream);
int vd_op_dps_seed(vd_engine* e, int B, int T, int H, int W, const float* x_t, const float* eps, const long long* t, int clip_denoised,
                   const float* y, const float* latent_mask, int scale, int gray, float* d_eps, float* d_x, float* rho,
                   float* pred_xstart, void* stream);

/* Particle steering -- this project's extension (Feynman-Kac steering: Singhal et al. 2025; the twisted diffusion sampler of Wu et al.
 * 2023 without its gradient proposal; the reference has nothing like it): guidance by a reward on the step's x_0 prediction WITHOUT a
 * derivative of the UNet -- sequential Monte Carlo over the reverse chain.  The batch is G groups of K consecutive items ("particles"):
 * item g K + k is particle k of group g, and a group's items share t, the masks, the frame indices and the observed content.  Every
 * particle runs the ordinary stochastic step; behind it the caller computes one fp64 reward r per item and hands them to
 * vd_particle_apply, which per group (particles.hip; every sum in index order in fp64, no floating-point atomics):
 *   1. logw_k += lambda (r_k - rprev_k), rprev_k = r_k (a reward or a log-weight of -inf keeps the particle at -inf);  m = max_k logw_k;
 *      p_k = exp(logw_k - m) / sum_j exp(logw_j - m);  ESS = 1 / sum_k p_k^2;
 *   2. if the K log-weights are bit-equal nothing else happens (a constant reward leaves the plain step's bits);
 *   3. else if ESS < ess_threshold K: systematic resampling at u = uniforms[2 g]: c_k = sum_{j <= k} p_j (1 from the last k with p_k > 0
 *      on), a_i = min{k : c_k > (u + i) / K}; item g K + i of each of the n <= 4 `tensors` ([B][per] floats, in place) takes the content of
 *      item g K + a_i, rprev_i = rprev_{a_i}, logw_i = 0, and the group's resample counter goes up;
 *   4. at t[g K] == 0 step 3 is skipped and chosen[g] = min{k : c_k > u2}, u2 = uniforms[2 g + 1]; nothing is gathered.
 * The increments telescope, so with the last reward taken on the final sample the chain targets p(x_0) exp(lambda r(x_0)) as K grows.
 * A group whose log-weights are all -inf is left as it is and its `degenerate` counter goes up.  A NaN or +inf reward is the caller's error.
 * vd_set_particles: engine state like the measurement.  K <= 1 or lambda == 0 clears it; K <= 256, lambda finite and not negative,
 *   ess_threshold in [0, 1].  y == NULL: the rewards are the caller's, through vd_particle_apply behind every step (eager steps only).
 *   y != NULL: the BUILT-IN reward of a noisy measurement, r_b = -rho_b^2 / (2 sigma_y^2), rho_b^2 the sum over the cells of item b's
 *   frames with latent_mask == 1 of (y - A x_0)^2 for the cell-mean operators of vd_set_measurement (scale, gray; y the caller's device
 *   tensor of that layout, kept alive), sigma_y > 0.  Every step whose sample is wanted (vd_p_sample, vd_ddim_sample,
 *   vd_dpmpp_2m_sde_sample with `pred_xstart` non-NULL, and the captured step of vd_window_begin) then appends three launches behind the
 *   sampler pass and behind nothing else: the residual pass of vd_dps_step's step 3 as it is, on the step's pred_xstart (at t == 0: on its
 *   sample, so that the increments telescope to lambda r(x_0)) -- same residual, partial layout and fold order, so an item's reward does
 *   not depend on B -- the weights from its partials, and the gather of `sample` and `pred_xstart` (dpmpp_2m_sde's history).  With the
 *   target exp(lambda r) and lambda = 1 the chain samples the Bayesian posterior of y = A x_0 + N(0, sigma_y^2) as K grows.
 *   While particles are set, a step whose sample is wanted fails by name for: a sampler that draws no noise (ddim_sample at eta = 0,
 *   dpmpp_2m_sample, unipc_sample, ddim_reverse_sample: duplicates would never separate), B no multiple of K, a known region, a
 *   measurement, an armed attention capture; so do the differentiated passes (vd_guided_step, vd_dps_step, vd_guide_begin, vd_eps_vjp,
 *   vd_ode_nll_eval), and vd_window_begin for the caller's rewards (a callback cannot be captured), the window prefix cache and the
 *   suffix skip.  cfg_scale, guidance rescale, dynamic thresholding, both mean types, every observed_frames mode and windows of 1..128
 *   frames are served.  With the state clear no launch is added and every path keeps its bits.  vd_particles: K, or 0 when clear.
 * The uniforms of the built-in reward: a window draws them from its own Philox stream -- group g's (u, u2) are the two 53-bit halves
 *   (words 0, 1 and 2, 3; 27 bits of the first above 26 of the second, times 2^-53) of block offset + 3/4 B per + g of the step's range
 *   of B per blocks: the sampler's noise uses the first quarter, the known-region merge the second, the re-noised observed frames the
 *   third, nothing else the fourth.  An eager step takes what vd_particle_draws set: a device tensor [G][2], or (uniforms NULL) the
 *   same Philox block at (seed, offset + 3/4 B per + g), offset being the head of the step's range -- how an eager loop repeats a
 *   window's draws.  vd_window_begin resets the state (vd_particle_reset) itself; eager chains call it before their first step.
 * vd_particle_reset: sizes the state for B items and zeroes it (logw, rprev, counters); waits for the device.  The state outlives
 *   vd_set_particles -- it can be read behind a window after the setting was cleared -- and a step or an apply under another K fails by name.
 * vd_particle_apply: two launches on `stream` (the weights, the gather), no host wait; rewards [B] fp64, t [B] the index of the step just
 *   made, uniforms [G][2] fp64 in [0, 1), all on the device; `tensors` is a host array of n device pointers (n = 0: weights only).
 * vd_particle_state: copies out logw [B], rprev [B], ancestors [B] (of the last apply: the item each item took, itself where nothing
 *   moved), chosen [G] (-1 unless the last apply was at t == 0), ess [G] and counters [G][2] (resamplings, degenerate steps); any may be
 *   NULL; host or device destinations; waits for the device.
 * vd_op_particle_weights / vd_op_particle_gather: the two passes alone on a caller's device state, no engine.  The weights pass takes the
 *   rewards, or (rewards NULL) nblk fp64 partial sums per item of a squared residual, folded in index order: r = -(sum / (2 sigma_y^2)).
 *   uniforms NULL: group g's pair from Philox block (seed, offset + g), as above.
 *   The gather serves ANY map `ancestors` over the B items, cycles included; it allocates its scratch, waits for `stream` and frees it.
 *   16-byte accesses while per % 4 == 0 and the tensors are 16-byte aligned, else element by element: same bits. */
int vd_set_particles(vd_engine* e, int K, double lambda, double ess_threshold, const float* y, int scale, int gray, double sigma_y);
int vd_particles(vd_engine* e);
int vd_particle_reset(vd_engine* e, int B);
int vd_particle_draws(vd_engine* e, const double* uniforms, unsigned long long seed, unsigned long long offset);
int vd_particle_apply(vd_engine* e, int B, long long per, const double* rewards, const long long* t, const double* uniforms,
                      float* const* tensors, int n, void* stream);
int vd_particle_state(vd_engine* e, int B, double* logw, double* rprev, int* ancestors, int* chosen, double* ess, long long* counters);
int vd_op_particle_weights(int G, int K, double lambda, double ess_threshold, const double* rewards, const double* partials, int nblk,
                           double sigma_y, const long long* t, const double* uniforms, unsigned long long seed, unsigned long long offset,
                           double* logw, double* rprev, int* ancestors, int* chosen, double* ess, long long* counters, void* stream);
int vd_op_particle_gather(int B, long long per, const int* ancestors, float* const* tensors, int n, void* stream);

/* Deblurring -- this project's extension: DPS (vd_dps_step) and the built-in reward of particle steering (vd_set_particles) for a
 * convolution measurement y = w * x_0 + noise (blur.hip).  w is ONE real k x k kernel, k odd, 1 <= k <= 15, applied to every channel plane
 * of every frame; the output has the plane's size, with zeros outside the plane; the orientation is torch's conv2d (correlation), c = k / 2:
 *   (A x)[i][j]   = sum_{a,b} w[a][b] x[i + a - c][j + b - c]
 *   (A^T r)[p][q] = sum_{a,b} w[a][b] r[p - a + c][q - b + c]      (the exact adjoint, which is why the padding is zeros)
 * y has the video's shape [B][T][3][H][W].  w need not be symmetric, normalised or non-negative.  Every sum over the taps runs in fp32 in one
 * fixed order -- a ascending, inside it b ascending, acc = acc + w[a][b] v with the product and the sum each rounded, never fused.
 * vd_set_blur_kernel: engine state.  k == 0 clears it (refused while vd_set_particle_blur is on); otherwise k*k finite taps on the HOST,
 *   row-major, not all zero, copied into an engine-owned device buffer whose address never changes; waits for the device.
 *   vd_blur_kernel: 1 and *k when a kernel is installed, else 0.
 * vd_deblur_step: vd_dps_step on the installed kernel -- its argument list without scale and gray, its seven steps with
 *   3. r = y - A x_0 on the frames in L_b, rho_b = sqrt(sum r^2) folded as there (fp64, fixed order, independent of B, no atomics);
 *   4. q = -(A^T r) / rho_b (0 where rho_b == 0 or L_b is empty), then q_r, d eps and d_x as there;
 *   its outputs, its workspace and its refusals under the name "deblur"; it also fails while no kernel is installed.  Eager steps only.
 * vd_op_deblur_seed: steps 2-4 alone on a caller's (x_t, eps) and taps ON THE DEVICE, on frames of H x W (any size), no network; outputs as
 *   vd_op_dps_seed.  vd_op_blur: out = A x (adjoint == 0) or A^T x of a [B][T][3][H][W] tensor, out != x; no engine.
 *   16-byte accesses while W % 4 == 0 and the tensors are 16-byte aligned, else element by element: same bits.
 * vd_set_particle_blur: on != 0 (a kernel must be installed) makes the installed kernel the operator of the built-in reward of
 *   vd_set_particles: y then has the video's shape and the scale and gray handed to vd_set_particles are not read (hand scale 1 with
 *   gray).  The residual pass runs inside the step's launches and is captured into a window graph; the graph's key carries k, and taps
 *   changed between two windows at equal k act without a new capture.  vd_particle_blur: the switch. */
int vd_set_blur_kernel(vd_engine* e, const float* taps_host, int k);
int vd_blur_kernel(vd_engine* e, int* k);
int vd_deblur_step(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask,
                   const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int obs_mode, int clip_denoised,
                   int sampler, float eta, const float* noise, const float* y, float zeta, float* sample, float* pred_xstart,
                   float* grad, float* residual_norm, void* stream);
int vd_op_deblur_seed(vd_engine* e, int B, int T, int H, int W, const float* x_t, const float* eps, const long long* t, int clip_denoised,
                      const float* y, const float* latent_mask, const float* taps_dev, int k, float* d_eps, float* d_x, float* rho,
                      float* pred_xstart, void* stream);
int vd_op_blur(int B, int T, int H, int W, const float* x, const float* taps_dev, int k, int adjoint, float* out, void* stream);
int vd_set_particle_blur(vd_engine* e, int on);
int vd_particle_blur(vd_engine* e);

/* Separable linear measurements -- this project's extension: the exact projection (vd_set_measurement's), DPS (vd_dps_step's) and the
 * built-in reward of particle steering for a measurement that acts on every channel plane of every frame alike as
 *   y[b][t][c] = A_h x_0[b][t][c] A_w^T,   A_h: Mh x H,  A_w: Mw x W,  1 <= Mh <= H <= 128,  1 <= Mw <= W <= 128   (linop.hip)
 * -- bicubic or bilinear down-sampling, a separable blur with any padding and stride, the cell mean.  y is [B][T][3][Mh][Mw].  The adjoint
 * is A_h^T r A_w, the back-projection P_h r P_w^T with P_h (H x Mh) and P_w (W x Mw), the caller's (truncated) pseudo-inverses.  All
 * matrices are dense, row-major fp32.  Every product is Z = L X R^T (L: P x Q, X: Q x U, R: S x U), the right factor first:
 *   tmp[q][s] = sum_u X[q][u] R[s][u], then Z[p][s] = sum_q L[p][q] tmp[q][s]
 * each sum from 0 in ascending index order, acc = acc + a * b with the product and the sum each rounded to fp32, never fused; tmp is fp32.
 * Forward: L = A_h, R = A_w.  Adjoint: L = A_h^T, R = A_w^T.  Back-projection: L = P_h, R = P_w.
 * vd_set_linear_operator: engine state, H = W = the model's image size.  Matrices on the HOST, finite, A_h and A_w not all zero, copied
 *   into engine-owned device buffers whose addresses never change; waits for the device.  P_h and P_w come together or are both NULL (the
 *   projection is then refused by name).  A_h or A_w NULL clears the operator (refused while vd_set_linear_measurement or
 *   vd_set_particle_linear reads it; while one does, new matrices keep the shape).  vd_linear_operator: 0 none, 1 installed, 2 with a
 *   back-projection; *Mh, *Mw.
 * vd_set_linear_measurement: y on the device (the caller's; NULL: off).  Every step then projects its x_0 prediction,
 *   x_0 <- x_0 + P_h (y - A_h x_0 A_w^T) P_w^T on the frames with latent_mask == 1, in the place and under the rules of vd_set_measurement:
 *   in front of the sampler pass, behind the dynamic threshold, the sampler pass in its x0_given form with the clamp off; composes with
 *   cfg_scale and guidance rescale; two launches per step.  Refused, by name, together with a known region, the window prefix cache or
 *   suffix skip, a sampler that walks up, vd_set_particles, the differentiated passes, and vd_set_measurement itself.  A window graph's
 *   key carries (y, Mh, Mw): new matrices of equal shape between two windows act without a new capture.  vd_linear_measurement: the switch.
 * vd_linear_dps_step: vd_deblur_step on the installed operator -- r = y - A x_0, rho_b, q = -(A_h^T r A_w) / rho_b; its outputs, its
 *   workspace and its refusals under the name "linear_dps"; it also fails while no operator is installed.  Eager steps only.
 * vd_set_particle_linear: on != 0 (an operator must be installed; refused together with vd_set_particle_blur) makes the installed operator
 *   the operator of the built-in reward of vd_set_particles: y is then [B][T][3][Mh][Mw] and the scale and gray handed there are not read
 *   (hand scale 1 with gray).  Captured into a window graph, whose key carries (Mh, Mw).  vd_particle_linear: the switch.
 * vd_op_linop: out = L x R^T of `planes` planes of Q x U, matrices ON THE DEVICE, out != x; no engine.
 * vd_op_linear_project: the projection alone on an x_0 handed in (through the clamp when clip_denoised), in place, on frames of H x W, no
 *   network; frames with latent_mask != 1 keep their bits unless clip_denoised.  vd_op_linear_dps_seed: the residual and seed passes alone
 *   on a caller's (x_t, eps); outputs as vd_op_dps_seed.  16-byte loads while the row length is a multiple of 4 and the tensors are 16-byte
 *   aligned, else element by element: same bits. */
int vd_set_linear_operator(vd_engine* e, const float* A_h_host, int Mh, const float* A_w_host, int Mw, const float* P_h_host,
                           const float* P_w_host);
int vd_linear_operator(vd_engine* e, int* Mh, int* Mw);
int vd_set_linear_measurement(vd_engine* e, const float* y);
int vd_linear_measurement(vd_engine* e);
int vd_linear_dps_step(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask,
                       const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int obs_mode, int clip_denoised,
                       int sampler, float eta, const float* noise, const float* y, float zeta, float* sample, float* pred_xstart,
                       float* grad, float* residual_norm, void* stream);
int vd_set_particle_linear(vd_engine* e, int on);
int vd_particle_linear(vd_engine* e);
int vd_op_linop(long long planes, int Q, int U, const float* x, const float* L_dev, int P, const float* R_dev, int S, float* out, void* stream);
int vd_op_linear_project(vd_engine* e, int B, int T, int H, int W, float* x0_inout, const float* y, const float* latent_mask,
                         const float* A_h_dev, int Mh, const float* A_w_dev, int Mw, const float* P_h_dev, const float* P_w_dev,
                         int clip_denoised, void* stream);
int vd_op_linear_dps_seed(vd_engine* e, int B, int T, int H, int W, const float* x_t, const float* eps, const long long* t, int clip_denoised,
                          const float* y, const float* latent_mask, const float* A_h_dev, int Mh, const float* A_w_dev, int Mw, float* d_eps,
                          float* d_x, float* rho, float* pred_xstart, void* stream);

/* Loss-guided sampling -- this project's extension: a reverse step moved down the gradient, with respect to x_t, of ANY differentiable
 * function of the step's x_0 prediction.  The function is the caller's own code: vd_dps_step is split in two around the point where the
 * cotangent of x_0 is formed, and the taped forward survives between the two calls.  Per item b, with L_b its frames with
 * latent_mask == 1, for an epsilon model at t (a, b as above):
 *   vd_guide_begin   steps 1, 2 and 6 of vd_dps_step: the taped forward, and the plain sampler pass (sampler 0 p_sample, 1 ddim_sample with
 *                    eta) -> sample' and pred_xstart, the bits of vd_p_sample / vd_ddim_sample with the same noise.  The tape is kept: the
 *                    engine holds the pass and *ticket (never 0) names it.
 *   (the caller)     cot = d loss / d pred_xstart, [B][T][3][H][W], by any means, on the device; what it holds off L_b is not read.
 *   vd_guide_finish  c_r = cot [-1 <= x_0r <= 1] with clip_denoised, else cot (x_0r = a x_t - b eps: the sampler pass's bits);
 *                    d eps = (-b) c_r, d_x = a c_r on L_b, 0 elsewhere: one fp32 rounding each;
 *                    g = d_x + (d eps / d x_t)^T d eps: the backward-data pass on a power-of-two multiple of d eps;
 *                    normalize: n_b = fp32(sqrt(sum over L_b of g^2)), the sum in fp64 in a fixed order that does not depend on B, no
 *                    floating-point atomics; m_b = n_b == 0 ? 0 : fp32(scale[b] / n_b); else m_b = scale[b];
 *                    sample = fmaf(-m_b, g, sample) on the frames of L_b, in place; every other frame keeps its bits.
 * `sample` of vd_guide_finish is the tensor vd_guide_begin wrote (or a copy of it); grad (g on every frame: 0 on observed frames) may be
 * NULL; grad_norm ([B], n_b) is written only with normalize and may be NULL; scale is [B] floats on the device, each finite and not
 * negative (the caller checks: the host does not read them).  A cot element that is not finite propagates into grad and sample and raises
 * no error bit: it is the caller's value.  A scale of 0 leaves sample' as it is.  A step costs one taped forward and one backward pass.
 * LIFETIME: x, obs_src, the masks, frame_indices and t of vd_guide_begin are read again by vd_guide_finish and must stay alive and
 * unchanged until it returns.  Both calls issue plain launches on `stream`, no host wait; the caller's code between them must be ordered
 * on that stream.
 * THE HELD PASS is never read stale.  One pass is held at most; it points into the workspace, so every entry that runs the network
 * (forward or backward), sizes the workspace or replays a window graph (vd_window_run) drops it before doing anything else, as do
 * vd_set_schedule and vd_set_bwd_weight_storage; a second vd_guide_begin drops the first pass and hands out a new ticket.
 * vd_guide_finish with a ticket that is not the live one fails with "loss_guidance: no taped pass is held for this ticket" and the cause
 * (never begun, already finished, or dropped by an engine call in between), launches nothing and leaves `sample` untouched.  Otherwise
 * the held pass is released when vd_guide_finish returns, whatever it returns.  vd_guide_abort drops a held pass (none: no effect);
 * vd_destroy calls it.  With no pass held no other entry changes what it launches.
 * vd_guide_begin fails by name ("loss_guidance") where vd_dps_step fails ("dps"): T above 32, a model that is not epsilon-prediction, a
 * missing backward image, a sampler other than 0 or 1, cfg_scale != 1, guidance rescale, dynamic threshold, a known region, a
 * measurement, an armed attention capture.  Not part of vd_window_begin / vd_window_run: a caller's code cannot be captured.
 * vd_op_guide_seed: the seed pass alone on a caller's (x_t, eps, cot) on frames of H x W (any size), no network, no workspace: d_eps, d_x.
 * A t[b] outside the schedule writes NaN on item b and raises bit 0 of the error word.  16-byte accesses while W % 4 == 0 and the tensors
 * are 16-byte aligned, else element by element: same bits. */
int vd_guide_begin(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask,
                   const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int obs_mode, int clip_denoised,
                   int sampler, float eta, const float* noise, float* sample, float* pred_xstart, unsigned long long* ticket,
                   void* stream);
int vd_guide_finish(vd_engine* e, unsigned long long ticket, const float* cot, const float* scale, int normalize, float* sample,
                    float* grad, float* grad_norm, void* stream);
int vd_guide_abort(vd_engine* e);
int vd_op_guide_seed(vd_engine* e, int B, int T, int H, int W, const float* x_t, const float* eps, const long long* t, int clip_denoised,
                     const float* cot, const float* latent_mask, float* d_eps, float* d_x, void* stream);

/* The vector-Jacobian product of the network, and on it the exact log-likelihood of the probability-flow ODE -- this project's extension
 * (Song, Sohl-Dickstein, Kingma, Kumar, Ermon, Poole, ICLR 2021; trace estimate: Skilling-Hutchinson; the reference has the variational
 * bound only, vd_vb_terms).  Both run the taped forward and the backward-data pass of use_gradient_method (second packed image:
 * vd_set_bwd_weight_storage) and are modelled on vd_dps_step: its workspace, plain launches on `stream`, no host wait.
 * vd_eps_vjp: eps = eps_theta(x, t) (eps_out, may be NULL) and vjp_out = (d eps / d x)^T cot for a caller's cotangent `cot` of x's shape,
 *   read on every frame.  The pass runs on s * cot with s the power of two that puts max |cot| into [1, 2) (the split arithmetic keeps its
 *   22 bits there) and 1 / s is applied on the way out.  The observed frames reach the network through obs_src and are constants: vjp_out
 *   is exactly 0 on them; on padding frames it is the network's own derivative.
 * vd_ode_nll_eval: eps (eps_out, may be NULL) and trace_out[b] = (1 / K) sum_k v_k^T (d eps / d x)^T v_k, K = n_probes in 1..64, the dot
 *   over the frames of item b with latent_mask == 1, accumulated in fp64 in a fixed order (no floating-point atomics: the same bits on
 *   every run and for every B).  One taped forward serves the K backward passes.  probe == NULL: v_k is the Rademacher probe number
 *   probe0 + k of vd_rademacher at (seed, item_offset): +-1 needs no rescaling.  Else probe is [K][B][T][3][H][W], read in place as it is
 *   (no rescaling: keep max |v| near 1; it should be 0 off the latent frames, where the dot does not look).  x_next (may be NULL): the
 *   Euler step of d(x / r) / d sigma = eps to index t + 1, r = sqrt_alphas_cumprod, sigma = sqrt_recipm1_alphas_cumprod -- the pass of
 *   vd_ddim_reverse_sample on (x, eps) with its clamp off, on the frames with latent_mask == 1; every other frame keeps the bits of x.
 * Both fail by name: T above 32, a model that is not epsilon-prediction, learn_sigma, an obs_mode other than 0 (x_0), cfg_scale != 1,
 *   guidance rescale, dynamic threshold, a known region, a measurement, an armed attention capture, a missing backward image; vd_ode_nll_eval
 *   also n_probes outside 1..64.  A t[b] outside the schedule raises bit 0 of the error word as every entry that runs the network does.
 * vd_rademacher: out [B][T][frame_elems] = probe number `probe`: +-1.0f on the frames with lat == 1, 0 elsewhere.  Element j of item b
 *   (j in 0..per-1, per = T * frame_elems < 2^31) is bit j & 31 of word (j >> 5) & 3 of the Philox4x32-10 block
 *   (seed, item_offset[b] + probe * ceil(per / 128) + (j >> 7)) of vd_randn's generator; a set bit is -1.  item_offset: [B] device words;
 *   item b of a batched call has the bits of the call on b alone.
 * vd_op_masked_dot: out[b] (double, device) = sum over the frames of item b with lat == 1 of (double)a * (double)b: every product exact, the
 *   sum in an order fixed by (T, frame_elems).  It allocates its scratch, waits for `stream` and frees it.
 * vd_op_ode_heun: the corrector of Heun's method on the frames with lat == 1, out = r' (x / r + 0.5 (sigma' - sigma) (eps + eps2)) with
 *   the float32 tables at t[b] and t[b] + 1, one fp32 rounding per operation, nothing fused; other frames keep the bits of x.  out may
 *   alias x.  A t[b] with no next level poisons item b with NaN and raises bit 0 of the error word.
 * vd_dequantize: uniform dequantisation of 8-bit data scaled to [-1, 1]: on the frames with lat == 1 out = x + (2 / 256) u, u in [0, 1) with 24
 *   bits: u = (w >> 8) 2^-24, w word j & 3 of the Philox block (seed, item_offset[b] + (j >> 2)) for element j of item b (the block element j
 *   of vd_randn(., seed, item_offset[b]) reads); other frames keep the bits of x; out may alias x.
 * vd_rademacher, vd_op_masked_dot and vd_op_ode_heun take 16-byte accesses while frame_elems % 4 == 0 and the tensors are 16-byte aligned, else element by element: same bits. */
int vd_eps_vjp(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask,
               const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int obs_mode, const float* cot,
               float* eps_out, float* vjp_out, void* stream);
int vd_ode_nll_eval(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask,
                    const float* kinda_marg_mask, const long long* frame_indices, const long long* t, int obs_mode, int n_probes,
                    unsigned long long seed, const unsigned long long* item_offset, unsigned long long probe0, const float* probe,
                    float* eps_out, double* trace_out, float* x_next, void* stream);
int vd_rademacher(float* out, const float* latent_mask, int B, int T, long long frame_elems, unsigned long long seed,
                  const unsigned long long* item_offset, unsigned long long probe, void* stream);
int vd_dequantize(const float* x, const float* latent_mask, int B, int T, long long frame_elems, unsigned long long seed,
                  const unsigned long long* item_offset, float* out, void* stream);
int vd_op_masked_dot(const float* a, const float* b, const float* latent_mask, int B, int T, long long frame_elems, double* out, void* stream);
int vd_op_ode_heun(vd_engine* e, int B, int T, long long frame_elems, const float* x, const float* eps, const float* eps2, const long long* t,
                   const float* latent_mask, float* out, void* stream);

/* diffusion.q_sample(x_start, t, noise) (gaussian_diffusion.py:190-206). */
int vd_q_sample(vd_engine* e, int B, long long per_sample, const float* x_start, const long long* t,
                const float* noise, float* out, void* stream);

/* th.randn(*shape) replacement on the engine's own counter-based generator. */
int vd_randn(float* out, long long n, unsigned long long seed, unsigned long long offset, void* stream);

/* Per-kernel-class timing with HIP events recorded on the launch stream (bench.py's roofline leg; no
 * reference counterpart).  Between begin and end every engine launch is bracketed by two events;
 * vd_profile_end synchronises and writes, per class i, out[4i..4i+3] = {launches, total ms,
 * algorithmic FLOPs, algorithmic bytes}. */
int vd_profile_begin(void);
int vd_profile_end(double* out, int cap);
int vd_profile_classes(void);
const char* vd_profile_class_name(int i);

/* ---- arithmetic of the matrix products (environment VD_MATH, read once per process) -------------
 *   0  f16x3  (default) an fp32 operand x is carried as two fp16 pieces, x ~ a0 + 2^-12 a1, a0 = f16(x), a1 = f16((x - a0) 2^12):
 *             22 significand bits (relative error <= 2^-22 for 2^-14 <= |x| < 2^15, absolute <= 2^-37 below; |x| >= 2^15 = 32768 -- not
 *             fp16's 65504: the scaled remainder (x - a0) 2^12 reaches 65536 there -- gives NaN, never a silently wrong number; inputs of
 *             a 3x3 conv: |x| < 2^13, its operand is a signed sum of four of them); a product is three piece products a0 b0 + a0 b1 + a1 (2^-12 b0) on
 *             v_mfma_f32_32x32x16_f16 with fp32 accumulation; weights carry a per-output power-of-two scale (image trailer).
 *   1  bf16x6 the exact split: three bf16 pieces per operand, six piece products (the default of earlier releases).
 *   2  fp32   every product on v_mfma_f32_32x32x2_f32.
 * The packed weight image depends on it (vd_weights_layout_id). */
int vd_math_mode(void);
/* uint16 count of a split weight image with n_out outputs and k_total inputs per output, trailer included
 * (= 3 n_out k_total + 4 n_out): [k/16][n_out/32][piece 3][lane 64][8 x 16 bit], then n_out float scales, n_out reciprocals. */
long long vd_split_image_u16(long long n_out, long long k_total);

/* ---- single-operator entry points (parity tests call the kernels through these) -------------- */
/* NHWC conv / linear on fp32 MFMA.  src1/C0: virtual channel concat; affA/affB: folded GroupNorm(+FiLM);
 * act: SiLU on the operand; res: residual in the epilogue; fbias: per-frame bias [nfr][fbias_ld]. */
/* w_packed: [tap][Cout][Cin] (generic kernel; may be NULL when w_frag / w_wino covers the shape);
 * w_frag: MFMA-fragment-major weights of a linear layer / 1x1 conv from vd_pack_linear_frag, or NULL;
 * w_wino: Winograd-transformed 3x3 weights from vd_pack_conv3_wino, or NULL (preferred when given and supported:
 *         one plain source tensor -- no concat, no affine/act prologue -- stride 1, square power-of-two >= 8x8,
 *         Cout % 64 == 0, Cin % 32 == 0). */
int vd_op_conv(const float* src0, const float* src1, int C0, int Cin, int nfr, int Hs, int Ws, int ups, int stride,
               int pad, int ksz, const float* w_packed, const float* w_frag, const float* w_wino, const float* bias,
               const float* affA, const float* affB, int act, const float* res, const float* fbias, int fbias_ld,
               float* out, int Cout, void* stream);
/* vd_op_conv whose epilogue also writes the GroupNorm partial sums of its OUTPUT (Winograd shapes only, -1 otherwise):
 * gn_part[nfr][split][Cout][2] doubles = per (frame, block of the frame, channel) [sum, sum of squares], with
 * split = vd_conv_stats_split(output height).  vd_op_gn_affine folds one or two such tables (the halves of a channel
 * concat; tables from vd_op_conv_stats or from a statistics pass have the same layout) into the (A, B) pair of
 * vd_op_gn_fold, so the consumer's GroupNorm (unet.py:185-198) never reads the tensor for its statistics. */
int vd_conv_stats_split(int Hout);
/* Output channels per block of the Winograd kernel a stride-1 3x3 conv of this shape runs on under the split arithmetic: 128
 * (conv_wino_z128.hip) or 64 (conv_wino_r64.hip).  Same weight image, same results up to summation order; tests use it to
 * know which kernel they exercised. */
int vd_conv_wino_block_couts(int nfr, int H, int Cin, int Cout);
int vd_op_conv_stats(const float* src0, int Cin, int nfr, int Hs, int Ws, int ups, const float* w_wino, const float* bias,
                     const float* res, const float* fbias, int fbias_ld, float* out, int Cout, double* gn_part,
                     void* stream);
int vd_op_gn_affine(const double* part0, int split0, int C0, const double* part1, int split1, int C, int nfr, int HW,
                    const float* gamma, const float* beta, const float* film, int film_ld, float* affA, float* affB,
                    void* stream);
/* The same fold, also writing mr_out[nfr][32][2] = the groups' (mean, rstd) as floats: what the backward pass reads. */
int vd_op_gn_affine_mr(const double* part0, int split0, int C0, const double* part1, int split1, int C, int nfr, int HW,
                       const float* gamma, const float* beta, const float* film, int film_ld, float* affA, float* affB,
                       float* mr_out, void* stream);
/* The statistics pass alone: part[nfr][split][C][2] doubles = per (frame, pixel range, channel) [sum, sum of squares] of the
 * virtual concat (src0: channels [0, C0), src1: [C0, C), null when C0 == C); range r covers pixels [r * per, min(HW, (r + 1) * per)),
 * per = ceil(HW / split), an empty range writes zeros.  split <= 0: vd_gn_stats_split(nfr, HW, C), the engine's choice. */
int vd_gn_stats_split(int nfr, int HW, int C);
int vd_op_gn_stats(const float* src0, const float* src1, int C0, int C, int nfr, int HW, int split, double* part, void* stream);
/* GroupNorm(+FiLM)(+SiLU) in one launch: every block folds its frame's statistics from the one or two tables itself, then
 * y[n][p][c] = SiLU?(concat(src0, src1)[n][p][c] * A[n][c] + B[n][c]) with the (A, B) of vd_op_gn_affine. */
int vd_op_gn_act_fold(const float* src0, const float* src1, int C0, int C, const double* part0, int split0, const double* part1,
                      int split1, int nfr, int HW, const float* gamma, const float* beta, const float* film, int film_ld, int act,
                      float* y, void* stream);
/* The form the engine's GroupNorm + activation takes for a layer call of layer_frames frames of HW pixels and C channels:
 * 0 = vd_op_gn_act_fold's kernel, 1 = vd_op_gn_affine then vd_op_affine_act (from 64 MB of fp32 tensor on). */
int vd_gn_act_form(int layer_frames, int HW, int C);
/* Winograd F(2x2,3x3) image of a 3x3 weight for the fp32-MFMA kernel: U = G g G^T per (cout, cin) with row 2 negated (the
 * kernel negates row 2 of B^T as well), 16*O*I floats in [I/16][16][O/32][2][64][4]; pass as w_wino. */
int vd_pack_conv3_wino(const float* host_oihw, float* host_out, int O, int I);
/* nn.Linear / 1x1-conv weight [N][K] (N, K multiples of 32) -> [K/32][N/32][4][64][4] for the fp32-MFMA kernel; pass the
 * result as w_frag with ksz = 1. */
int vd_pack_linear_frag(const float* host_w, float* host_out, int N, int K);
/* Linear layer on the 16-bit matrix cores at fp32 accuracy (csrc/gemm_split.hip) in the process' arithmetic (f16x3 | bf16x6;
 * with VD_MATH=fp32 these entry points run bf16x6).  The weight is split on the host: [N][K] (N, K multiples of 32) ->
 * vd_split_image_u16(N, K) uint16.  out[m][n] = bias[n] + res[m][n] + sum_k f(a[m][k]) w[n][k], f = SiLU if act.  The engine's
 * kernel for every nn.Linear / 1x1 conv / the stem. */
int vd_pack_linear_split(const float* host_w, unsigned short* host_out, int N, int K);
/* 3x3 convolutions that Winograd does not cover (the stride-2 Downsample convs, unet.py:98) on the same arithmetic: the
 * split GEMM kernel walks an implicit im2col operand (k = tap*I + c; taps outside the image read 0).
 * Weights: OIHW -> the split image of the [O][9*I] matrix = vd_split_image_u16(O, 9*I) uint16.  stride 1 or 2, padding 1. */
int vd_pack_conv3_split(const float* host_oihw, unsigned short* host_out, int O, int I);
int vd_op_conv_split(const float* src0, int Cin, int nfr, int Hs, int Ws, int stride, const void* w_split, const float* bias,
                     const float* res, float* out, int Cout, void* stream);
/* The same arithmetic for the 3x3 stride-1 convs: Winograd F(2x2,3x3) whose element products run as piece products of the
 * split fp32 operands, 64 couts per block, input transform and split in the MFMA fragment layout, in registers
 * (csrc/conv_wino_r64.hip); maps >= 8x8.  Weights: OIHW -> U = G g G^T (fp64, row 3 negated) split into
 * [I/16][16][O/32][3][64][8] + trailer = vd_split_image_u16(O, 16*I) uint16.  One plain source tensor, stride 1, square
 * power-of-two maps, O % 64 == 0, I % 32 == 0; gn_part as vd_op_conv_stats (or NULL).  Big windows are cut along frames. */
int vd_pack_conv3_wino_split(const float* host_oihw, unsigned short* host_out, int O, int I);
int vd_op_conv_wino_split(const float* src0, int Cin, int nfr, int Hs, int Ws, int ups, const void* w_split, const float* bias,
                          const float* res, const float* fbias, int fbias_ld, float* out, int Cout, double* gn_part,
                          void* stream);
/* The ResBlock's `GroupNorm -> SiLU -> conv3x3` (unet.py:138-141,185-198) with the normalisation's folded affine and the SiLU applied
 * INSIDE the convolution kernel: out = conv3x3(silu(x * affA[frame][c] + affB[frame][c])) + bias (+ res), zero padding applied to the
 * ACTIVATED tensor as in the reference.  csrc/conv_wino_z128.hip stages the patch through registers and activates it there, so the
 * activation image (one write + one read of the tensor) does not exist.  The input may be the virtual channel concat of two tensors
 * (src1 != NULL: C0 channels from src0, Cin - C0 from src1: th.cat([h, hs.pop()], 1), unet.py:826-828).  Shapes: vd_conv_wino_act_ok(nfr, H, Cin, Cout) -- the f16x3
 * arithmetic, maps >= 16 x 16, Cout in {128, 256}, Cin <= 320, a grid that fills the chip. */
int vd_op_conv_wino_act(const float* src0, const float* src1, int C0, int Cin, int nfr, int Hs, int Ws, const void* w_split, const float* bias,
                        const float* affA, const float* affB, const float* res, float* out, int Cout, double* gn_part, void* stream);
int vd_conv_wino_act_ok(int nfr, int H, int Cin, int Cout);
/* Upsample (nearest x2, unet.py:70-77) + conv3x3 in its sub-pixel form on csrc/conv_wino_r64.hip: output pixel (2y + a, 2x + b) sees
 * only a 2 x 2 neighbourhood of the SOURCE map, i.e. four 3x3 "phase" kernels with one zero row and one zero column each
 * ((w0, w1 + w2, 0) for a = 0, (0, w0 + w1, w2) for a = 1; sums in fp64), convolved with the low-resolution map; in the Winograd
 * domain one of the four columns of every such kernel is zero and is skipped (a quarter of the matrix work of F(2x2,3x3) on
 * the upsampled map).  Weights: OIHW -> 4*O phase kernels -> the vd_pack_conv3_wino_split layout = vd_split_image_u16(4*O, 16*I) uint16.  src0
 * [nfr][Hs][Hs][Cin], out [nfr][2Hs][2Hs][Cout]; gn_part [nfr][vd_conv_ups_stats_split(Hs)][Cout][2] doubles or NULL. */
int vd_pack_conv3_wino_ups(const float* host_oihw, unsigned short* host_out, int O, int I);
int vd_conv_ups_stats_split(int Hs);
int vd_op_conv_wino_ups(const float* src0, int Cin, int nfr, int Hs, const void* w_ups, const float* bias, float* out, int Cout,
                        double* gn_part, void* stream);
int vd_op_linear_split(const float* a, int M, int K, const void* w_split, const float* bias, const float* res, int act,
                       float* out, int N, void* stream);
/* The same layer with the GroupNorm partial sums of its output from the epilogue (the rows are the HW pixels of M / HW
 * consecutive frames; unet.py:537-538 followed by the next block's normalization, nn.py:15-17): gn_part is
 * [M / HW][vd_linear_stats_split(M, N, HW)][N][2] doubles, per channel [sum, sum of squares]. */
int vd_op_linear_split_stats(const float* a, int M, int K, const void* w_split, const float* bias, const float* res, int act,
                             float* out, int N, int HW, double* gn_part, void* stream);
int vd_linear_stats_split(int M, int N, int HW);
/* GroupNorm32 statistics folded to y = x*A + B per (frame, channel); film ([nfr][2C] scale|shift) optional. */
int vd_op_gn_fold(const float* src0, const float* src1, int C0, int C, int nfr, int HW, const float* gamma,
                  const float* beta, const float* film, int film_ld, float* affA, float* affB, void* stream);
int vd_op_affine_apply(const float* x, const float* affA, const float* affB, int nfr, int HW, int C, float* y,
                       void* stream);
/* y[n][p][0..C) = SiLU?(concat(src0, src1)[n][p][c] * A[n][c] + B[n][c]): GroupNorm(+FiLM)+SiLU and the skip concat
 * materialised once as the input of a 3x3 conv (in_layers / out_layers of ResBlock, unet.py:150-199). */
int vd_op_affine_act(const float* src0, const float* src1, int C0, int C, const float* affA, const float* affB, int nfr,
                     int HW, int act, float* y, void* stream);
int vd_op_gn_temporal(const float* x, const float* gamma, const float* beta, int B, int T, int HW, int C, float* y,
                      void* stream);
int vd_op_attn_spatial(const float* qkv, int nfr, int L, int C, int heads, float* out, void* stream);
int vd_op_attn_temporal(const float* qkv, const float* Rk, const float* Rq, const float* Rv, const float* mask, int B,
                        int T, int HW, int C, int heads, int allow_pad, float* out, void* stream);
/* The return_attn_weights maps (unet.py:457-466: attn.view(B*D, -1, T, T).mean(dim=1).abs()) alone, through the launchers the forward
 * calls under vd_set_attn_capture, with the operands, layouts and scale of the two entries above.
 * Temporal: out [B*HW][T][T] = | mean over heads of softmax_s(q'_t . (k_s + Rk[t,s]) + scale k_s . Rq[s,t]) |, masked by the rule of
 * unet.py:511-524 (a masked entry is exactly 0); Rk and Rq both or neither; mask may be NULL; T <= 128, one kernel for T <= 32 and one
 * that cuts the query rows into chunks of 32 above; refused ("head dim too large") where a block's rows exceed 150 KiB of LDS.
 * Spatial: out [nfr][L][L], no relative positions, no mask; head dim a multiple of 4 ("shape"), refused ("sequence too long") where 16
 * score rows and their mean exceed 150 KiB of LDS (L above about 1100). */
int vd_op_attn_temporal_weights(const float* qkv, const float* Rk, const float* Rq, const float* mask, int B, int T, int HW, int C,
                                int heads, int allow_pad, float* out, void* stream);
int vd_op_attn_spatial_weights(const float* qkv, int nfr, int L, int C, int heads, float* out, void* stream);
/* Which kernel instantiation vd_op_attn_temporal (and the engine) runs a per-item shape on, as its C++ name --
 * "attn_temporal_mfma_kernel<NT,JM,RPE,EXACT>", "attn_temporal_kernel<PB,TMAX,RPE>" (T <= 32),
 * "attn_temporal_long_mfma_kernel<NJ,RPE>", "attn_temporal_long_kernel<RPE>" (T = 33..128) -- or "refused: <reason>".
 * Returns 1 (a kernel), 0 (refused) or a negative code (no room in name[cap]).  Host only: no launch, no device call; the
 * launchers dispatch through the same function.  The batch size is no argument: it never changes the choice.  Tests use it
 * to know which kernel they exercised. */
int vd_attn_temporal_variant(int T, int HW, int C, int heads, int rpe, char* name, int cap);
/* The same for vd_op_attn_spatial (and the engine), in the process' own VD_MATH: "attn_spatial_split_kernel<F,F16,NW>" (f16x3: F16 =
 * true, bf16x6: false; NW = 2 for L <= 64, 4 for L <= 128, 8 above), "attn_spatial_kernel<F>" (fp32), or "refused: <reason>" -- C not
 * divisible by heads, a head dim F = C / heads outside {8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 112, 128}, a non-positive L, C or
 * heads.  Same return values; host only; the launcher dispatches through the same table and vd_op_attn_spatial returns -1 for a
 * refused shape before any launch.  The frame count is no argument: it never changes the choice. */
int vd_attn_spatial_variant(int L, int C, int heads, char* name, int cap);
/* The same for every convolution and linear layer (vd_op_conv, vd_op_conv_wino_*, vd_op_conv_split, vd_op_linear_split*, the entries below
 * and the engine), in the process' own VD_MATH: the full instantiation name out of the table its kernel file dispatches through --
 * "gemm_split_kernel<BM,BN,ACT,CONV,F16,SIDE>", "conv3x3_wino_r64_kernel<TF4,F16>" ("+ksplitS" appended when the channel loop is cut
 * into S slices), "conv3x3_wino_r64_ups_kernel<TF4,F16>", "conv3x3_wino_z128_kernel<ACT>", "gemm_frag_kernel<BM,BN,ACT>",
 * "conv3x3_wino_kernel<TF4>", "igemm_kernel<BM,BN>" -- or "refused: <reason>".  Arguments, as they decide the dispatch: kernel size (1 |
 * 3), stride, ups (source read through a nearest x2 upsample), channels (C0 < Cin: a virtual concat), frames of this launch and of the
 * whole layer call (nfr_sel, 0 = nfr), the square source map H (a linear layer of M rows: nfr = M, H = 1), the weight image given --
 * 0 [tap][Cout][Cin], 1 vd_pack_linear_frag, 2 vd_pack_conv3_wino, 3 vd_pack_linear_split | vd_pack_conv3_split, 4
 * vd_pack_conv3_wino_split, 5 vd_pack_conv3_wino_ups (the sub-pixel form) --, SiLU on the operand, presence of the operand's affine
 * pair, per-frame bias, residual and side output, the number of batched problems, and whether split-K scratch is offered (the engine
 * and vd_op_conv_wino_split_k do, the other entries do not).  Returns 1 / 0 (refused) / < 0 (no room for the name); host only. */
int vd_igemm_variant(int ksz, int stride, int ups, int Cin, int C0, int Cout, int nfr, int nfr_sel, int H, int weights, int act, int affine,
                     int fbias, int res, int side, int zcount, int ksplit_scratch, char* name, int cap);
/* Every instantiation name those tables hold for the process' VD_MATH, one per line; returns their number. */
int vd_igemm_variant_list(char* names, int cap);
/* Engine-only paths as single operators.  vd_conv_wino_ksplit: slices of the channel loop conv_wino_r64.hip cuts a small grid into (1: none).
 * vd_op_conv_wino_split_k: vd_op_conv_wino_split with the split-K scratch the engine provides, kernel and slices chosen for nfr_sel frames
 * (0: nfr) -- a frame's bits do not depend on which other frames share its launch.  vd_op_linear_split_side: the ResBlock's fused skip
 * conv, a 1x1 over the virtual concat (a0 [M][C0], a1 [M][K - C0] or NULL) on the 128x128 tile, which also writes side [M][K] =
 * SiLU(a * sideA[frame][k] + sideB[frame][k]) (frames of HW rows); -1 where the shape is not one the engine would fuse.
 * vd_op_linear_batched: zcount problems of one shape in one launch (the relative-position nets): problem z reads a + z M K, writes out +
 * z M N, weight image at zbase + ztab[2z] and bias at zbase + ztab[2z + 1] (float offsets, a device table); the image is the mode's
 * (vd_pack_linear_split, or vd_pack_linear_frag under VD_MATH=fp32). */
int vd_conv_wino_ksplit(int nfr, int H, int Cin, int Cout);
int vd_op_conv_wino_split_k(const float* src0, int Cin, int nfr, int Hs, int Ws, int ups, const void* w_split, const float* bias,
                            const float* res, const float* fbias, int fbias_ld, float* out, int Cout, double* gn_part, int nfr_sel,
                            void* stream);
int vd_op_linear_split_side(const float* a0, const float* a1, int C0, int K, int M, int HW, const void* w_split, const float* bias,
                            const float* sideA, const float* sideB, float* out, float* side, int N, void* stream);
int vd_op_linear_batched(const float* a, int zcount, int M, int K, int N, const float* zbase, const long long* ztab_dev, float* out,
                         void* stream);
/* The output head out = conv3x3(SiLU(h * A[frame] + B[frame])) + bias (unet.py:744-749,838) in its direct form (out_conv_kernel):
 * h [nfr][H][W][C], w_packed [tap][Cout][C], out NCHW; Cout <= 8, C % 32 == 0.  This kernel is the op-only form and is NOT on the
 * forward, which runs the head as vd_op_out_head does. */
int vd_op_out_conv(const float* x, const float* affA, const float* affB, const float* w_packed, const float* bias,
                   int nfr, int H, int W, int C, int Cout, float* out_nchw, void* stream);
/* The same head (unet.py:744-749,838) through the code the forward runs: T[pixel][co * 9 + tap] = SiLU(h * A + B) . w[co][:][tap] as a
 * 1x1 GEMM over 32 (Cout 3) or 64 (Cout 6) columns -- head_gemm_kernel where H * W % 1024 == 0, C % 8 == 0 and C <= 128 at 32
 * columns, in its 2- or 8-tiles-per-wave form by the pixel count; the generic fp32 kernel with the affine and SiLU in its operand
 * load otherwise (C % 32 == 0) -- then out[n][co][y][x] = bias[co] + sum over the 9 taps of T at the neighbour the tap points to,
 * zero outside the image (out_gather_kernel).  h [nfr][H][W][C], affA / affB [nfr][C], bias [Cout] and out_nchw [nfr][Cout][H][W] on
 * the device; w_oihw is the checkpoint's out.2.weight [Cout][C][3][3] in host or device memory, packed here by the function
 * vd_load_weight packs it with.  Cout is 3 or 6.  The scratch T is allocated for the call, which synchronises the stream before it
 * returns.  A refused shape returns -1 with the reason in vd_last_error() before any launch. */
int vd_op_out_head(const float* h, const float* affA, const float* affB, const float* w_oihw, const float* bias, int nfr, int H, int W,
                   int C, int Cout, float* out_nchw, void* stream);
/* Which GEMM vd_op_out_head (and the forward) runs a head shape on: "head_gemm/tpw2", "head_gemm/tpw8", "igemm/32", "igemm/64" (the
 * generic kernel at 32 | 64 columns), or "refused: <reason>".  Returns 1, 0 (refused) or a negative code (no room in name[cap]).
 * Host only: no launch, no device call; read off the function that launches. */
int vd_out_head_variant(int nfr, int H, int W, int C, int Cout, char* name, int cap);
/* Backward-data operators of use_gradient_method (csrc/backward.hip); each one synchronises its stream before it returns. */
/* GroupNorm32(+FiLM)(+SiLU) backward over a virtual concat; mr [nfr][32][2] (mean, rstd); dx0 / dx1 assigned or accumulated (acc0 / acc1), plus extra if given. */
int vd_op_gn_bwd(const float* x0, const float* x1, int C0, int C, const float* affA, const float* affB, const float* mr,
                 const float* dy, int act, int nfr, int HW, const float* extra, float* dx0, int acc0, float* dx1, int acc1,
                 void* stream);
/* Backward of vd_op_gn_temporal without its affine shift (the statistics are recomputed from x); T <= 32. */
int vd_op_gn_temporal_bwd(const float* x, const float* gamma, const float* dy, int B, int T, int HW, int C, int accumulate,
                          float* dx, void* stream);
/* Backward of vd_op_attn_temporal: dout [B*T*HW][C] -> dqkv [B*T*HW][3C]; T <= 32. */
int vd_op_attn_temporal_bwd(const float* qkv, const float* Rk, const float* Rq, const float* Rv, const float* mask, int B,
                            int T, int HW, int C, int heads, int allow_pad, const float* dout, float* dqkv, void* stream);
/* Backward of vd_op_attn_spatial: dout [nfr*L][C] -> dqkv [nfr*L][3C]; L <= 1024, head dim <= 128 and a multiple of 4. */
int vd_op_attn_spatial_bwd(const float* qkv, int nfr, int L, int C, int heads, const float* dout, float* dqkv, void* stream);
/* Output head conv backward, data part: deps [nfr][Cout][H][W] -> da [nfr][H][W][C]; w as vd_op_out_conv's w_packed [tap][Cout][C]. */
int vd_op_out_conv_bwd(const float* deps, const float* w, int nfr, int H, int W, int C, int Cout, float* da, void* stream);
/* Stem backward: dcols [nfr][H*W][64] (k = tap * stem channels + channel) -> dx [nfr][3][H][W]; cond_mode 0 channel, 1 duplicate / all, 2 t=0. */
int vd_op_stem_col2im(const float* dcols, const float* obs, const float* lat, const float* km, int nfr, int H, int W,
                      int cond_mode, float* dx, void* stream);
/* What lies between those kernels in the backward-data pass.
 * The backward image of a forward weight -- the operator d out / d in of the layer as a forward layer of its own -- by the one function
 * vd_load_weight_bwd packs with.  host_w: [O][I] (linear layer, 1x1 conv) or OIHW (3x3), O and I the FORWARD's outputs and inputs.  kind:
 *   0 linear        W^T [I][O] as vd_pack_linear_split(N = I, K = O)
 *   1 stem          the matrix [k = tap * I + i][o], rows 9 I .. 63 zero, as vd_pack_linear_split(N = 64, K = O)
 *   2 Winograd conv w'[i][o][t] = w[o][i][8 - t] (transposed, rotated by 180 degrees) as vd_pack_conv3_wino_split(O' = I, I' = O)
 *   3 generic conv  the same kernel as [tap][I][O] floats
 * vd_bwd_image_floats: floats of the image (-1: no such kind or shape).  Host only. */
long long vd_bwd_image_floats(int kind, int O, int I);
int vd_pack_weight_bwd(const float* host_w, int kind, int O, int I, float* host_out);
/* The two matrix-product calls of the pass, with the engine's own argument setup, in the process' arithmetic; VD_MATH=fp32 is refused
 * as vd_set_bwd_weight_storage refuses it.  out[nfr][H][H][cout_bwd] = conv3x3 (stride 1, padding 1) of dy [nfr][H][H][cin_bwd] with
 * the image w_bwd (kind 2 | 3, on the device; cin_bwd = the forward's O, cout_bwd = its I) + res (or NULL; res == out is allowed: the
 * Downsample branch accumulates in place).  Kind 2 is offered split-K scratch by the engine's rule (allocated for the call, which then
 * waits for the stream).  vd_op_linear_bwd_data: out[M][N] = dy[M][K] * image (kind 0: K = O, N = I; kind 1: N = 64) + res. */
int vd_op_conv3_bwd_data(const float* dy, int nfr, int H, int cin_bwd, const void* w_bwd, int kind, int cout_bwd, const float* res, float* out,
                         void* stream);
int vd_op_linear_bwd_data(const float* dy, int M, int K, const void* w_bwd, const float* res, float* out, int N, void* stream);
/* y[n][2oy][2ox][c] = x[n][oy][ox][c], zero elsewhere (x [nfr][Ho][Wo][C], y [nfr][2Ho][2Wo][C]): the Downsample conv's backward is a
 * stride-1 conv of this.  sumpool2: y[n][oy][ox][c] (+)= ((b00 + b01) + b10) + b11 of the 2x2 block of x [nfr][2Ho][2Wo][C]: the
 * nearest x2 upsample's backward.  add: y (+)= x, n % 4 == 0.  C % 4 == 0; enqueued only. */
int vd_op_zero_stuff2(const float* x, int nfr, int Ho, int Wo, int C, float* y, void* stream);
int vd_op_sumpool2(const float* x, int nfr, int Ho, int Wo, int C, int accumulate, float* y, void* stream);
int vd_op_add(const float* x, long long n, int accumulate, float* y, void* stream);
/* g *= s in place, s = 2^k with max |g| s in [1, 2) (k clamped to +-100; s = 1 when the maximum is 0 or not below 3e38; a NaN does not
 * enter the maximum and stays); gs (4 floats on the device) receives {s, 1 / s, the bits of max |g|, 0}.  Enqueued only. */
int vd_op_grad_rescale(float* g, long long n, float* gs, void* stream);
/* The two guidance passes of vd_guided_step on caller's tensors [B][per] (per = T frames of per / T elements), the engine's schedule
 * table; no network.  guided_grad: d loss / d eps, the direct part of d loss / d x, the unguided mean and pred_xstart (the last two
 * may be NULL).  guided_final: g = dxd + dx_net * gs[1], mean_out = mean - 10 alpha_t g / 2, sample = mean_out + [t != 0] sigma_t
 * noise2; grad, mean_out and sample may be NULL.  A t[b] outside the schedule writes NaN rows; a non-finite x_0 sets VD_ERR_NONFINITE. */
int vd_op_guided_grad(vd_engine* e, int B, int T, long long per, const float* x, const float* eps, const float* noise, const float* x_t_minus_1,
                      const float* obs, const long long* t, int clip_denoised, float* deps, float* dxd, float* mean, float* xstart, void* stream);
int vd_op_guided_final(vd_engine* e, int B, int T, long long per, const long long* t, const float* dxd, const float* mean, const float* dx_net,
                       const float* gs, const float* noise2, float* grad, float* mean_out, float* sample, void* stream);
/* The kernels that build what the network is conditioned on (csrc/misc.hip), each through the launcher the forward pass calls and
 * with the arguments in the forward pass' form.  Enqueued only.
 * out[i] = [cos(t[i] f_j) | sin(t[i] f_j)], j < dim / 2, and a zero last column when dim is odd (timestep_embedding / frame_embedding,
 * nn.py:89-122); freqs: dim / 2 floats on the device, as vd_set_freqs receives them. */
int vd_op_sinus_embed(const float* t, int n, int dim, const float* freqs, float* out, void* stream);
/* tv[b][t] = frame_indices[b][t] (- their float32 mean over t when center; unet.py:914-926). */
int vd_op_frame_t(const long long* frame_indices, int B, int T, int center, float* tv, void* stream);
/* RPENet hidden layer of nz nets at once (unet.py:283-296): E[z][b][t][s][c] = silu(te[b*T + t][tab[3z] + c] + Wd_z[c][:] . feat(d)
 * + bd_z[c]), d = fi[b][t] - fi[b][s], feat = (log(1 + max(d, 0)), log(1 + max(-d, 0)), d == 0); te rows of te_ld floats; Wd_z [C][3]
 * at wbase + tab[3z + 1], bd_z [C] at wbase + tab[3z + 2]; tab: 3 nz offsets (in floats) on the device; net z writes at E + z * zs_e. */
int vd_op_rpe_hidden(const float* te, int te_ld, const float* wbase, const long long* tab, const long long* frame_indices, int B, int T,
                     int C, float* E, int nz, long long zs_e, void* stream);
/* Bucket-table relative positions (RPE.get_bucket_ids, unet.py:330-347): R[b][t][s][:] = table[bucket(fi[b][t] - fi[b][s])], table
 * [2 beta + 1][C], negative buckets wrapping as torch indexing does. */
int vd_op_rpe_table(const float* table, const long long* frame_indices, int B, int T, int C, float alpha, float beta, float gamma,
                    float* R, void* stream);
/* y[n][p][c] = x[n][p][c] + P[p][c] + femb[n][c] (unet.py:914-926); P and femb may each be NULL; C % 4 == 0. */
int vd_op_posenc_add(const float* x, const float* P, const float* femb, int nfr, int HW, int C, float* y, void* stream);
/* The network input of CondMargVideoModel.forward (unet.py:951-983,991-1013) as the im2col matrix of the 3x3 stem, x_cols
 * [B*T*H*W][Kpad] with k = tap * Cs + channel (Cs = 5 | 6 | 3 stem channels for cond_mode 0 | 1 | 2; zeros for taps outside the image and
 * for k >= 9 Cs; Kpad 64, 128 or 256), plus the per-frame timesteps t_frames [B*T] (obs_t_mode: 0 'x_0', 1 'x_t', 2 'x_t_minus_1') and the
 * attention mask amask [B*T].  With frame_list (n_list device ints) the rows of frame frame_list[i] go to row block i and the per-frame
 * scalars are not written; with scalars_only x_cols is not written; both together are refused. */
int vd_op_assemble(const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask, const float* kinda_marg_mask,
                   const float* t_model, int obs_t_mode, int B, int T, int H, int W, int Kpad, int cond_mode, const int* frame_list,
                   int n_list, int scalars_only, float* x_cols, float* t_frames, float* amask, void* stream);
/* Frame-granular moves of the window prefix cache / suffix skip: gather dst[i] = src[list[i]], scatter dst[list[i]] = src[i], rows of
 * row_floats floats (a multiple of 4), i < n.  vd_op_scatter_stats: GroupNorm partial sums src [n][split][C][2] doubles folded over
 * split, in order, into dst[list[i]][C][2]. */
int vd_op_move_rows(int scatter, const float* src, const int* list, int n, long long row_floats, float* dst, void* stream);
int vd_op_scatter_stats(const double* src, int split, int C, const int* list, int n, double* dst, void* stream);

/* ---- LPIPS frame distance of the adaptive-* frame schedulers (csrc/lpips.hip).
 * Replaces LpipsEmbedder (improved_diffusion/inference_util.py:15-31: lpips.LPIPS(net='alex', spatial=False), AlexNet features
 * with per-layer unit normalisation, lin-weight scaling, flattened) as AdaptiveInferenceStrategyBase.embed uses it (:142-150), and
 * the farthest-point loop of select_obs_indices (:157-185).  fp32 operands and accumulation whatever VD_MATH says; deterministic.
 * A handle belongs to the device current at vd_lpips_create. */
typedef struct vd_lpips vd_lpips;
int vd_lpips_create(vd_lpips** out);
void vd_lpips_destroy(vd_lpips* h);
/* Host fp32 tensors, blocking H2D copy; packing happens here, once.  Names: "conv1.weight" .. "conv5.weight" (OIHW, torchvision
 * alexnet.features.{0,3,6,8,10}), "conv1.bias" .. "conv5.bias", "lin1" .. "lin5" ((C,) lin-layer weights, non-negative), and optional
 * "shift" / "scale" (3 values each; default: the lpips ScalingLayer constants). */
int vd_lpips_load_weight(vd_lpips* h, const char* name, const float* host, long long bytes);
/* Embedding length D of an H x W frame, or -1 when some layer of the feature stack would be empty. */
long long vd_lpips_dim(int H, int W);
/* frames [N][3][H][W] in the model's [-1, 1] space (no remapping, as LpipsEmbedder.forward) -> out [N][D].  Workspace owned by
 * the handle (grown on demand, bounded: frames are processed in chunks). */
int vd_lpips_embed(vd_lpips* h, int N, int H, int W, const float* frames, float* out, void* stream);
/* Frames of H x W that vd_lpips_embed puts through the feature stack per pass when N is larger (the workspace bound of 2^26 floats over
 * the per-frame activations, at most 65535), or -1 where vd_lpips_dim gives -1.  vd_lpips_embed runs min(N, this) frames at a time.
 * Host only. */
int vd_lpips_embed_chunk(int H, int W);
/* Test hook, as vd_scratch_fill: waits for the device and sets every byte of the handle's workspace to `byte`; the weights and the
 * workspace's address stay.  bytes_filled: 0 on a handle that has not embedded. */
int vd_lpips_scratch_fill(vd_lpips* h, int byte, long long* bytes_filled);
/* Farthest-point selection on embs [B][n_cand][D] (inference_util.py:157-185): out [B*n + 1] ints receives per item the n picked
 * CANDIDATE indices (pick 0 and every pick i < n_always is always_host[i]; the others the argmax of the squared distance to the
 * nearest earlier pick, lowest index on ties; repicks possible), and out[B*n] an error word (bit 0: a distance was not finite).
 * work: B*n_cand floats.  Enqueued only: the caller reads `out` back once. */
int vd_fps_select(int B, int n_cand, long long D, const float* embs, int n, const int* always_host, int n_always, float* work,
                  int* out, void* stream);

/* ---- Evaluation metrics of sampled videos (csrc/metrics.hip).
 * Replaces the per-frame, per-channel host loops of scripts/video_eval.py: compute_metrics_lazy (:205-225; scikit-image 0.19.3
 * structural_similarity and peak_signal_noise_ratio on float32 planes) and the distance half of compute_lpips_lazy (:228-252;
 * lpips.LPIPS(net='alex', spatial=False) of two frames = the squared L2 distance of their vd_lpips_embed embeddings).
 *
 * Frame metrics: gt [N][C][H][W] float32 in [0, 1]; pred the same shape, uint8 (read as u / 255) when pred_is_u8, else float32.  Per frame the
 * mean over its C planes of
 *   SSIM: 7 x 7 uniform window, sample covariance (49/48), K1 = 0.01, K2 = 0.03, data range ssim_data_range (2.0 is what the
 *         reference's scikit-image takes for float images when none is passed, 1.0 the true range), mean over the windows that lie
 *         inside the plane (the crop of 3 pixels per side);
 *   PSNR: 10 log10(1 / mse), mse the float64 mean of the squared float32 differences; +inf for identical planes.
 * Sums in float64, fixed order: a frame's values do not depend on the other frames of the call.  Limits: H, W >= 7, W <= 1024, C >= 1.
 * Device pointers; enqueued only.  The partial-sum table is owned by the library (per device, grown on demand). */
int vd_frame_metrics(int N, int C, int H, int W, const float* gt, const void* pred, int pred_is_u8, double ssim_data_range,
                     double* ssim_out, double* psnr_out, void* stream);
/* What vd_frame_metrics launches with for H x W planes, from the function it calls itself: the input rows of a full LDS strip
 * (32, fewer once two planes of 32 rows pass the tile: W >= 240, down to 7 at W = 1024), the strips per plane, and the row runs a
 * strip's output rows are cut into (1 once W - 6 > 256: every thread then walks several columns).  Returns 0, or vd_frame_metrics'
 * refusal of the size.  Host only. */
int vd_frame_metrics_plan(int H, int W, int* rows_tile, int* nstrips, int* groups);
/* Test hook, as vd_scratch_fill: waits for the device and sets every byte of the current device's partial-sum table to `byte`; its
 * address stays.  bytes_filled: 0 before the first vd_frame_metrics. */
int vd_frame_metrics_scratch_fill(int byte, long long* bytes_filled);
/* out[n] = sum over d of (a[n][d] - b[n][d])^2 for rows of D floats, differences and sum in float64, fixed order. */
int vd_pair_sqdist(int N, long long D, const float* a, const float* b, double* out, void* stream);

/* ---- Green-hallway pixel count of GQN-Mazes frames (csrc/hallway.hip).
 * Replaces the per-frame host loop of scripts/video_eval_room_seq_acc.py: _count_hallway_pixels (:126-137), i.e. per frame
 * cv2.cvtColor(image[14:45], COLOR_RGB2HSV), cv2.inRange(hsv, (50, 25, 25), (70, 255, 255)), cv2.erode(mask, ones((2, 2))) and the
 * number of non-zero pixels left, and the quantisation (x * 255).astype(np.uint8) in front of it (:247, :278).
 *
 * The 8-bit HSV is OpenCV's integer arithmetic restated: v = max, m = min, d = v - m, S = (d * sdiv[v] + 2048) >> 12 with
 * sdiv[i] = round(255 * 4096 / i), H = (h' * hdiv[d] + 2048) >> 12 (arithmetic shift, + 180 when negative) with
 * hdiv[i] = round(180 * 4096 / (6 i)) and h' = g - b if v == r, else b - r + 2d if v == g, else r - g + 4d; sdiv[0] = hdiv[0] = 0.
 * A pixel is green when 50 <= H <= 70, S >= 25 and V >= 25.  The erosion keeps pixel (y, x) of the STRIP when every in-strip pixel
 * among (y-1, x-1), (y-1, x), (y, x-1), (y, x) is green (anchor (1, 1); what lies outside the strip does not count).
 *
 * frames [N][3][H][W] planar: uint8 when is_u8, else float32 in [0, 1] quantised as (uint8)(x * 255.0f) -- one fp32 multiply, clamped
 * to 0..255, truncated.  counts[n] = eroded green pixels of rows row0 .. row1 - 1 of frame n; only those rows are read.  One block
 * per frame; a frame's count does not depend on the other frames of the call.  Limits: 1 <= H, W; 0 <= row0 < row1 <= H;
 * (row1 - row0) * W <= vd_hallway_max_strip() pixels (the strip's mask is held in LDS).  Device pointers; enqueued only. */
int vd_hallway_counts(int N, int H, int W, int row0, int row1, const void* frames, int is_u8, int* counts, void* stream);
/* Largest strip, in pixels, that vd_hallway_counts takes. */
int vd_hallway_max_strip(void);
/* The per-pixel half on its own: rgb [n][3] uint8 -> hsv [n][3] (or NULL) and mask [n], 255 where green else 0, before any erosion.
 * The same device function as vd_hallway_counts: an entry for tests. */
int vd_op_green_mask(long long n, const unsigned char* rgb, unsigned char* hsv, unsigned char* mask, void* stream);

/* ---- I3D video embedding of the Frechet video distance (csrc/i3d.hip).
 * Replaces create_id3_embedding(preprocess(videos, (224, 224))) (improved_diffusion/frechet_video_distance.py:38-133; the TF-Hub
 * module deepmind/i3d-kinetics-400/1, output RGB/inception_i3d/Mean:0): TF1 bilinear resize to 224 x 224 and 2 x / 255 - 1, the
 * 57 Unit3D convolutions of Inception-v1 inflated to 3-D with TF's SAME padding, the logits layer, the mean over time.  fp32 operands
 * and accumulation whatever VD_MATH says; deterministic; a video's feature does not depend on the other videos of the call.
 * A handle belongs to the device current at vd_i3d_create. */
typedef struct vd_i3d vd_i3d;
int vd_i3d_create(vd_i3d** out);
void vd_i3d_destroy(vd_i3d* h);
/* Host fp32 tensors, blocking H2D copy; packing happens here, once.  Names: "<unit>.weight" ([Cout][Cin][kt][kh][kw], the BatchNorm
 * already folded in) and "<unit>.bias" ([Cout]) for <unit> = Conv3d_1a_7x7, Conv3d_2b_1x1, Conv3d_2c_3x3 and
 * Mixed_{3b,3c,4b,4c,4d,4e,4f,5b,5c}.{b0,b1a,b1b,b2a,b2b,b3b}; "logits.weight" ([400][1024]) and "logits.bias". */
int vd_i3d_load_weight(vd_i3d* h, const char* name, const float* host, long long bytes);
/* Longest video vd_i3d_embed takes (1024 frames); the shortest has 9. */
int vd_i3d_max_frames(void);
/* videos [N][T][3][H][W] uint8 (device) -> out [N][400] (device).  Workspace owned by the handle, grown on demand for T; the videos
 * are processed one after another on `stream`.  A T outside 9 .. vd_i3d_max_frames() is refused before anything is allocated. */
int vd_i3d_embed(vd_i3d* h, int N, int T, int H, int W, const unsigned char* videos, float* out, void* stream);
/* Test hook, as vd_scratch_fill: waits for the device and sets every byte of the handle's workspace to `byte`; the weights and the
 * workspace's address stay.  bytes_filled: 0 on a handle that has not embedded. */
int vd_i3d_scratch_fill(vd_i3d* h, int byte, long long* bytes_filled);
/* One convolution of that network on its own: x [T][H][W][Cin] channels-last, w [Cout][Cin][kt][kh][kw] and bias [Cout] (or NULL) on
 * the device, SAME padding, optional ReLU; output row (ot, oy, ox) at out + ((ot*Ho + oy)*Wo + ox) * out_stride, Cout floats
 * (out may point into a wider tensor).  Packs w on every call and waits for the stream: an entry for tests. */
int vd_op_conv3d_same(const float* x, const float* w, const float* bias, int T, int H, int W, int Cin, int Cout, int kt, int kh,
                      int kw, int st, int sh, int sw, int relu, float* out, long long out_stride, void* stream);
/* Max pool with SAME padding (the padding never wins): x [T][H][W][C] -> out [To][Ho][Wo][C], sizes ceil(size / stride); C % 4 == 0. */
int vd_op_maxpool3d_same(const float* x, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw, float* out,
                         void* stream);
/* The preprocessing: frames [T][3][H][W] uint8 -> out [T][224][224][3] float32 in [-1, 1]. */
int vd_op_resize_bilinear_tf1(const unsigned char* frames, int T, int H, int W, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
