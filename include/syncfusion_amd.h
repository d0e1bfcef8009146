/*
 * syncfusion_amd -- C ABI of the MI355X (gfx950) implementation of SyncFusion's
 * generation hot path.
 *
 * The reference (mcomunita/syncfusion) has no FFI: its "plugin API" is Hydra
 * `_target_` instantiation plus Python duck typing.  The
 * entry points below are what a binding for that path would bind; each cites the
 * reference interface it replaces.  All pointers are DEVICE pointers unless
 * marked host; all tensors are fp32, contiguous, in the reference's own
 * (channels-first PyTorch) layout at the boundary.  No ownership is transferred,
 * no exceptions cross the ABI, every call returns SF_OK (0) or an SF_ERR_* code
 * and leaves a message in sf_last_error().  `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  Nothing here allocates inside the timed path:
 * activations live in a caller-provided workspace.
 */
#ifndef SYNCFUSION_AMD_H
#define SYNCFUSION_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_MAX_DEPTH 12

enum {
  SF_OK = 0,
  SF_ERR_INVALID = 1,        /* bad argument / inconsistent config                       */
  SF_ERR_MISSING_WEIGHT = 2, /* a named parameter was not supplied or has the wrong size  */
  SF_ERR_SHAPE = 3,          /* B/L0/T/H/W not supported by this model (stride, length)   */
  SF_ERR_HIP = 4,            /* a HIP runtime call failed                                 */
  SF_ERR_WORKSPACE = 5,      /* workspace missing or too small                            */
  SF_ERR_UNSUPPORTED = 6
};

enum { SF_UP_NEAREST_CONV3 = 0, SF_UP_TRANSPOSE = 1 };
/* arithmetic / storage type of the activations and packed weights (accumulation, statistics, softmax and the sampler state are fp32 in every
 * mode).  SF_F32X ("fp32x", the parity-grade fast path): activations stay fp32 in HBM, every matrix product is built from split fp16
 * operands -- a = hi + lo'/2048, three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation -- which measures 7.5e-8 rel-L2 against fp64
 * on a K = 3072 GEMM (plain fp32 MFMA: 3.5e-7) at several times the fp32 matrix rate; operands must stay inside the fp16 range (< 65504). */
enum { SF_F32 = 0, SF_BF16 = 1, SF_F16 = 2, SF_F32X = 3 };

/* One named parameter of a torch state_dict: fp32, contiguous, PyTorch layout, device memory. */
typedef struct {
  const char *name;
  const void *data;
  int64_t numel;
} sf_tensor;

const char *sf_version(void);
const char *sf_last_error(void);
/* 1 when a gfx950 device is visible to the HIP runtime, else 0 (never fails). */
int sf_device_ok(void);
/* Measurement aid (bench.py; no reference counterpart): the shader clock the chip holds WHILE a workload runs.  _start puts a one-wave
 * kernel on `stream` (a side stream) that compares the shader-cycle counter with the constant 100 MHz counter for `microseconds`;
 * _read waits for it and returns MHz (host pointer).  One probe at a time per process. */
int sf_clock_probe_start(double microseconds, void *stream);
int sf_clock_probe_read(double *mhz_out);

/* ------------------------------------------------------------------------------------------
 * U-Net denoiser + v-sampler
 *   replaces: audio_diffusion_pytorch.UNetV0 / DiffusionModel.sample as instantiated by
 *   exp/model/diffusion.yaml:11-33 and called from main/generation.py:77-83,
 *   main/module_diffusion.py:77,200-206.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_layers;
  int32_t in_channels;
  int32_t channels[SF_MAX_DEPTH];
  int32_t factors[SF_MAX_DEPTH];
  int32_t items[SF_MAX_DEPTH];
  int32_t attentions[SF_MAX_DEPTH];
  int32_t cross_attentions[SF_MAX_DEPTH];
  int32_t context_channels[SF_MAX_DEPTH];
  int32_t attention_heads;
  int32_t attention_features;
  int32_t embedding_features;
  int32_t embedding_max_length;
  int32_t modulation_features;
  int32_t resnet_groups;
  int32_t dtype; /* SF_F32 (parity path), SF_BF16 or SF_F16 */
  /* Up path of a block (a-unet apex.py): SF_UP_NEAREST_CONV3 = nn.Upsample(nearest) + Conv1d(k=3) [UpsampleInterpolate];
   * SF_UP_TRANSPOSE = ConvTranspose1d(kernel = stride = factor) [Upsample]; `blocks.{d}.up.weight` is (in, C, 3) resp. (C, in, factor). */
  int32_t upsample_mode;
  /* [RECALLED] facts about a-unet's TimeConditioningPlugin / AttentionBase that only the upstream package can settle;
   * zero = SURVEY appendix A.3 as written.  tools/pin_upstream.py decides them, keymap.py reads the first and the last off a checkpoint.
   *   time_fourier_features: learned frequencies of the time embedder (0 = modulation_features / 2; a-unet NumberEmbedder(dim=256) = 128):
   *     `time.fourier_w` has this many entries, `time.lin0.weight` is (modulation_features, 1 + 2 * time_fourier_features);
   *   time_no_first_act: 1 = no GELU between the embedder's Linear and the two (Linear, GELU) layers;
   *   attention_out_bias: 1 = every `to_out` Linear of the attention items carries a bias (`<item>.{attn,cross}.to_out.bias`). */
  int32_t time_fourier_features, time_no_first_act, attention_out_bias;
} sf_unet_config;

typedef struct sf_unet sf_unet;

/* Build the engine: packs/folds the named fp32 parameters into its own device buffers
 * (weights are copied; the caller may free `weights` afterwards).  Parameter names are
 * listed by sf_unet_param_name(). */
int sf_unet_create(const sf_unet_config *cfg, const sf_tensor *weights, int n_weights, void *stream, sf_unet **out);
void sf_unet_destroy(sf_unet *h);

/* Enumerate the parameter names/sizes the engine expects for `cfg` (host strings). */
int sf_unet_param_count(const sf_unet_config *cfg);
int sf_unet_param_name(const sf_unet_config *cfg, int index, char *name_out, int name_cap, int64_t *numel_out);

/* Bytes of caller-allocated workspace needed for batch B and length L0 (two_pass != 0 when
 * embedding_scale != 1: cond and uncond evaluations run as one 2B batch). */
int64_t sf_unet_workspace_bytes(const sf_unet *h, int B, int L0, int two_pass);
/* Same for sf_vsample with `num_steps` steps (adds the sigma schedule and the per-step modulation table). */
int64_t sf_vsample_workspace_bytes(const sf_unet *h, int B, int L0, int two_pass, int num_steps);

/* One denoiser evaluation  v = net(x, sigma; channels, embedding, embedding_scale)
 *   (replaces UNetV0.forward, reached from main/module_diffusion.py:77 through VDiffusion).
 *   x, out: (B, in_channels, L0).  sigma: (B).  ctx[d]: (B, context_channels[d], L0/prod(factors[:d+1])).
 *   emb: (B, embedding_max_length, embedding_features). */
int sf_unet_forward(sf_unet *h, const float *x, const float *sigma, const float *const *ctx, const float *emb,
                    int B, int L0, float embedding_scale, float *out, void *ws, int64_t ws_bytes, void *stream);

/* The whole sampling loop  x <- VSampler(net)(x_noisy, num_steps, ...)  in place
 *   (replaces DiffusionModel.sample, main/generation.py:77-83, main/module_diffusion.py:200-206).
 *   use_graph != 0 captures one step into a hipGraph and replays it. */
int sf_vsample(sf_unet *h, float *x_inout, const float *const *ctx, const float *emb, int B, int L0,
               int num_steps, float embedding_scale, int use_graph, void *ws, int64_t ws_bytes, void *stream);

/* The inpainting loop  x <- VInpainter(net)(source, mask, num_steps, num_resamples, x_noisy = x, ...)  in place  (SURVEY.md A.6):
 *   sf_vsample's loop over num_steps * num_resamples iterations; after each v-step, where mask != 0, x is replaced by the source re-noised
 *   to the iteration's target level,  alpha * source + beta * z,  z = the standard normals of sf_op_philox_normal(seed, iteration, element).
 *   A resample (all but the last iteration of a step) re-noises to the step's OWN level.  The last iteration has beta == 0: where the mask
 *   is set the result is the source, bit for bit.
 *   x_inout, source: (B, in_channels, L0) fp32.  mask: (B, in_channels, L0), one byte per element, non-zero = keep the source.
 *   Neither source nor mask is written.  Conditioning, graph use and the single host synchronisation are sf_vsample's; the step graph is
 *   cached separately from sf_vsample's and replayed for any later source / mask / seed of the same shape, workspace and guidance scale.
 *   The workspace is larger than sf_vsample's (source, mask and seed live in it): sf_vinpaint_workspace_bytes. */
int64_t sf_vinpaint_workspace_bytes(const sf_unet *h, int B, int L0, int two_pass, int num_steps, int num_resamples);
int sf_vinpaint(sf_unet *h, float *x_inout, const float *source, const uint8_t *mask, const float *const *ctx, const float *emb, int B,
                int L0, int num_steps, int num_resamples, uint64_t seed, float embedding_scale, int use_graph, void *ws, int64_t ws_bytes,
                void *stream);

/* The sampling loop with a linear multistep rule on x0_hat = alpha x - beta v and a caller-given schedule, in place ("Multistep
 * sampler"; an addition, not part of the reference):  step i evaluates v at sigmas[i] and applies
 *   X_i = al x - be v,   x <- cx x + c0 X_i + c1 X_{i-1},      (al, be, cx, c0, c1) = table[8 i .. 8 i + 4]   (X_{-1} = 0)
 *   sigmas: HOST, num_steps + 1 floats, finite, strictly decreasing, inside [0, 1].  table: HOST, num_steps rows of 8 floats (three unused),
 *   finite; syncfusion_amd.solvers.solver_table builds it.  Both are copied into the workspace before the call returns.
 *   Conditioning, graph use and the single host synchronisation are sf_vsample's; the step graph is cached separately from sf_vsample's and
 *   sf_vinpaint's and replayed for any later table / sigmas of the same shape, workspace and guidance scale.
 *   The workspace is larger than sf_vsample's (the history X_{i-1} and the table live in it): sf_vsample_ms_workspace_bytes. */
int64_t sf_vsample_ms_workspace_bytes(const sf_unet *h, int B, int L0, int two_pass, int num_steps);
int sf_vsample_ms(sf_unet *h, float *x_inout, const float *const *ctx, const float *emb, int B, int L0, int num_steps, float embedding_scale,
                  const float *sigmas, const float *table, int use_graph, void *ws, int64_t ws_bytes, void *stream);

/* sf_vsample_ms with a guidance schedule ("Guidance schedules"; an addition, not part of the reference):
 *   scales: HOST, num_steps rows of B finite floats, scales[i * B + b] = guidance scale of clip b at step i; NULL = 1 everywhere.
 *   rescale: phi in [0, 1].  Step i uses  g = s == 1 ? v_c : v_u + (v_c - v_u) * s  and, where phi > 0,  v = g * (1 + phi * (std(v_c) / std(g) - 1))
 *   with the standard deviations over all elements of the clip; v enters the solver row as in sf_vsample_ms.
 *   No scale other than 1 in the call: the unconditional half is not evaluated (B rows per step, not 2 B) and the call is sf_vsample_ms's at
 *   embedding_scale 1, step graph included.  Otherwise every step evaluates 2 B rows; its graph is cached apart, keyed on phi but not on the
 *   scales: a later table of the same shape replays it.
 *   hist_io: device, B * in_channels * L0 floats, or NULL.  Non-NULL: the history X_{i-1} the loop starts from and, on return, the one it ended
 *   with, so that a schedule can be cut into consecutive calls -- each with its slice of sigmas, scales and of the table built for the WHOLE
 *   schedule (row 0 of a continuing call has c1 != 0).  NULL: X_{-1} = 0, as in sf_vsample_ms.
 *   Workspace: sf_vsample_gx_workspace_bytes (two_pass = any scale != 1). */
int64_t sf_vsample_gx_workspace_bytes(const sf_unet *h, int B, int L0, int two_pass, int num_steps);
int sf_vsample_gx(sf_unet *h, float *x_inout, const float *const *ctx, const float *emb, int B, int L0, int num_steps, const float *sigmas,
                  const float *table, const float *scales, float rescale, float *hist_io, int use_graph, void *ws, int64_t ws_bytes, void *stream);

/* Debug taps (tests only): after the next sf_unet_forward, every block-level activation is
 * copied as fp32 channels-last rows into `buf` (device).  Query the table afterwards. */
int sf_unet_debug_enable(sf_unet *h, float *buf, int64_t cap_floats);
int sf_unet_debug_count(const sf_unet *h);
int sf_unet_debug_info(const sf_unet *h, int i, char *name_out, int name_cap, int64_t *offset, int64_t *rows, int32_t *cols);

/* Per-kernel launch accounting of the last forward (host side, for bench.py's roofline):
 * number of kernel launches in one evaluation. */
int sf_unet_launch_count(const sf_unet *h);
/* Step graphs captured and instantiated by sf_vsample so far.  Graphs are cached per (shape, workspace, guidance) -- the active set
 * plus three stashed ones -- so a server alternating between a few request shapes stops adding to this after its first round. */
int sf_unet_graph_captures(const sf_unet *h);
/* Number of clip-parallel branches (independent slices of the batch run concurrently on separate HIP streams,
 * forked/joined with events): 0 = automatic (2 for >= 4 clips), 1 = off, up to 8. */
int sf_unet_set_branches(sf_unet *h, int n);
/* Per-launch timing of the next sf_unet_forward: HIP events recorded on `stream` around every kernel launch
 * (label = kernel / tile variant; flops, bytes = ALGORITHMIC work of that launch). */
int sf_unet_profile_enable(sf_unet *h, int on);
int sf_unet_profile_count(const sf_unet *h);
int sf_unet_profile_get(const sf_unet *h, int i, char *name_out, int name_cap, float *ms, double *flops, double *bytes);
/* U-Net depth (block index, 0 = outermost) of profile record i; -1 for per-step features, -2 for a bad index.  Feeds the
 * per-depth-group roofline SURVEY.md section 8d asks for (HBM side for depths 0-3, MFMA side for depths 4-7). */
int sf_unet_profile_depth(const sf_unet *h, int i);

/* ------------------------------------------------------------------------------------------
 * Encoder1d (onset-track feature pyramid)
 *   replaces: audio_encoders_pytorch.Encoder1d as instantiated by exp/model/diffusion.yaml:35-43
 *   and called as onsets_encoder(y, with_info=True) at main/generation.py:71,
 *   main/module_diffusion.py:76,196.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_layers; /* len(factors) */
  int32_t in_channels;
  int32_t channels;
  int32_t multipliers[SF_MAX_DEPTH + 1];
  int32_t factors[SF_MAX_DEPTH];
  int32_t num_blocks[SF_MAX_DEPTH];
  int32_t resnet_groups;
  int32_t patch_size; /* must be 1 */
} sf_encoder1d_config;

typedef struct sf_encoder1d sf_encoder1d;

int sf_encoder1d_create(const sf_encoder1d_config *cfg, const sf_tensor *weights, int n_weights, void *stream, sf_encoder1d **out);
void sf_encoder1d_destroy(sf_encoder1d *h);
int64_t sf_encoder1d_workspace_bytes(const sf_encoder1d *h, int B, int L0);
/* y: (B, in_channels, L0).  xs_out[0] = to_in(y), xs_out[1+i] = downsample_i output, each
 * (B, C_i, L_i) fp32 channels-first: n_layers + 1 pointers (info["xs"][1:-1] of the reference). */
int sf_encoder1d_forward(sf_encoder1d *h, const float *y, int B, int L0, float *const *xs_out,
                         void *ws, int64_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * VideoOnsetNet (R(2+1)D-18 with the temporal stride removed + FC head)
 *   replaces: main/onset_net.py:46-63 (VideoOnsetNet.forward), main/resnet.py:234-251.
 *   Weights use the reference's own state_dict names (net.model.stem.0.weight ... fc.2.bias),
 *   BatchNorm in eval mode (running statistics are folded into the convolutions).
 * ---------------------------------------------------------------------------------------- */
typedef struct sf_onsetnet sf_onsetnet;

int sf_onsetnet_create(const sf_tensor *weights, int n_weights, int dtype, void *stream, sf_onsetnet **out);
void sf_onsetnet_destroy(sf_onsetnet *h);
int64_t sf_onsetnet_workspace_bytes(const sf_onsetnet *h, int N, int T, int H, int W);
/* frames: (N, 3, T, H, W); logits: (N, T) raw (no sigmoid), as the reference returns them. */
int sf_onsetnet_forward(sf_onsetnet *h, const float *frames, int N, int T, int H, int W, float *logits,
                        void *ws, int64_t ws_bytes, void *stream);
int sf_onsetnet_debug_enable(sf_onsetnet *h, float *buf, int64_t cap_floats);
int sf_onsetnet_debug_count(const sf_onsetnet *h);
int sf_onsetnet_debug_info(const sf_onsetnet *h, int i, char *name_out, int name_cap, int64_t *offset, int64_t *rows, int32_t *cols);
/* Detail mode of the debug taps (tests only).  With enable != 0 every later forward with a debug buffer records, besides the five stage
 * taps (stem, layer1 .. layer4), the output of each of the 37 convolutions as (rows, cout) fp32, named after the convolution's
 * state_dict prefix without "net.model.": stem.0, stem.3, layerL.B.conv1.0.0, layerL.B.conv1.0.3, layerL.B.conv2.0.0, layerL.B.conv2.0.3
 * and layerL.0.downsample.0 (L = 2, 3, 4).  Rows are ordered ((n T + t) H + h) W + w, so a clip is one contiguous row range: with
 * n_clips > 0 every tap of such a forward, the stage taps included, holds only the rows of clips[0 .. n_clips) (host array of clip
 * indices, copied by the call), back to back in that order; n_clips == 0 keeps all clips.  enable == 0 restores the five stage taps over
 * all clips.  The taps are copies made after a convolution's launches: the dispatch and the logits do not depend on the mode. */
int sf_onsetnet_debug_detail(sf_onsetnet *h, int enable, const int32_t *clips, int n_clips);
/* The launch sequence behind tap i of the last forward (-1: no such tap; stage taps report 0). */
#define SF_ONSET_PATH_GEMM 0       /* one conv_gemm launch (generic / macro-tile implicit GEMM) */
#define SF_ONSET_PATH_GEMM_SPLIT 1 /* two conv_gemm launches: whole 192-column tiles, then the remaining columns */
#define SF_ONSET_PATH_SP 2         /* frame-walk (1,3,3) kernel (conv_sp.hip) */
#define SF_ONSET_PATH_TW 3         /* temporal-walk (3,1,1) kernel (conv_tw.hip) */
#define SF_ONSET_PATH_STEM 4       /* RGB (1,7,7) stride-2 stem kernel (onset_stem.hip) */
int sf_onsetnet_debug_path(const sf_onsetnet *h, int i);

/* ------------------------------------------------------------------------------------------
 * Onset glue on device: logits -> one-hot impulse track
 *   replaces: main/module_onset.py:160-183 (threshold raw logits > 0.5, t = (idx+start)/fps,
 *   "%.4f" rounding) + main/dataset_diffusion.py:69-72 (track[:, int(t*sr)] = 1).
 *   logits: (N, T); track: (N, 1, L) is zero-filled then set. */
int sf_onsets_to_track(const float *logits, int N, int T, const int32_t *start_frame /* (N) or NULL */,
                       float frame_rate, float sample_rate, float threshold, float *track, int L, void *stream);

/* ------------------------------------------------------------------------------------------
 * Post-sampling cut_prefix + crop on device
 *   replaces: main/generation.py:86-89 (gen[i, :, :nonzero(y[i][0])[0]] = 0) and :100 (gen[..., :cut_length]).
 *   gen: (B, C, L); y: (B, 1, L) impulse track; out: (B, C, cut_length); first_onset: (B) int32 device array that
 *   receives the index of the first onset of every clip, L when the track is empty (the reference raises IndexError
 *   there: the caller checks). */
int sf_cut_prefix_crop(const float *gen, const float *y, int B, int C, int L, int cut_length, float *out, int32_t *first_onset,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Post-sampling resampler
 *   replaces: torchaudio.functional.resample(gen[i, :, :cut_length].cpu(), orig_freq=sample_rate,
 *   new_freq=downsample_rate) at main/generation.py:91-98 (torchaudio==0.13.1 defaults: windowed-sinc, Hann,
 *   lowpass_filter_width 6, rolloff 0.99).  x: (R, L) fp32 rows; out: (R, ceil(new*L/orig)).
 * ---------------------------------------------------------------------------------------- */
typedef struct sf_resampler sf_resampler;
int sf_resampler_create(int orig_freq, int new_freq, int lowpass_filter_width, float rolloff, sf_resampler **out);
void sf_resampler_destroy(sf_resampler *h);
int sf_resampler_out_length(const sf_resampler *h, int L);
int sf_resampler_forward(sf_resampler *h, const float *x, int R, int L, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Input side
 *   sf_frames_preprocess replaces the per-frame transform of main/dataset_onset.py:47-50,152-165
 *     (ToTensor -> Resize((112,112), antialias=True) -> Normalize(mean, std) -> (C,T,H,W)) for a batch of decoded frames:
 *     frames:(N,T,H,W,3) uint8 device memory -> out:(N,3,T,out_h,out_w) fp32; mean3 / std3 are HOST arrays of 3 floats.
 *   sf_times_to_track replaces the impulse-track construction of main/dataset_diffusion.py:58-72
 *     (`onset[:, int(t * sr)] = 1.0`): times:(n_times) float64 seconds and clip_of:(n_times) clip indices, device memory.
 *   sf_frames_augment replaces the TRAINING transform of the onset data, cfg/data/data-onset-greatesthit-augment.yaml:8-28 as
 *     main/dataset_onset.py:152-165 applies it to the (T,C,H,W) stack of one clip (variants: main/datamodule_onset.py:138-156):
 *     ToTensor -> Resize((resize_h, resize_w), antialias=True) -> RandomCrop / CenterCrop((out_h, out_w)) -> ColorJitter -> Normalize ->
 *     (C,T,H,W), torchvision 0.14.1 semantics for float tensors, for a batch of clips with per-clip parameters:
 *     frames:(N,T,H,W,3) uint8 device memory -> out:(N,3,T,out_h,out_w) fp32.  The resized image is never materialised: the antialiased
 *     filter (scale = in / resized) is evaluated at the pixels that survive the crop.  The random draws stay with the caller: one
 *     sf_augment_clip per clip -- crop origin in the resized image, the order of the four colour operations (0 brightness, 1 contrast,
 *     2 saturation, 3 hue: ColorJitter.forward's fn_idx), one factor per operation and a presence mask (bit op set: applied; an absent
 *     operation is skipped, not applied with a neutral factor).  table_host is validated HERE, before anything is launched (crop inside
 *     the resized image, order a permutation, finite factors, brightness / contrast / saturation >= 0, |hue| <= 0.5); table_dev is the
 *     caller's device copy of the same N entries, which the kernels read.  Contrast blends with the mean gray of one frame's cropped
 *     pixels AFTER the operations before it, so a clip with contrast takes two passes (the second in place on `out`); the per-frame sums
 *     are reduced in a fixed order without atomics: equal inputs give equal bits.  ws: sf_frames_augment_workspace_bytes() bytes of
 *     device scratch.  mean3 / std3 are HOST arrays of 3 floats.
 * ---------------------------------------------------------------------------------------- */
typedef struct sf_augment_clip {
  int32_t top, left;
  int32_t order[4];
  float factor[4];
  int32_t mask;
  int32_t reserved;
} sf_augment_clip;
int64_t sf_frames_augment_workspace_bytes(int N, int T, int out_h, int out_w);
int sf_frames_augment(const uint8_t *frames, int N, int T, int H, int W, int resize_h, int resize_w, int out_h, int out_w,
                      const sf_augment_clip *table_host, const sf_augment_clip *table_dev, const float *mean3, const float *std3, float *out,
                      void *ws, int64_t ws_bytes, void *stream);
int sf_frames_preprocess(const uint8_t *frames, int N, int T, int H, int W, int out_h, int out_w, const float *mean3, const float *std3,
                         float *out, void *stream);
int sf_times_to_track(const double *times, const int32_t *clip_of, int n_times, double sample_rate, int B, int L, float *track, void *stream);

/* ------------------------------------------------------------------------------------------
 * Op-level entry points (channels-last, used by tests/ to localise kernel bugs).
 *   dtype selects the storage type of x / w / out (fp32 or bf16 bit patterns).
 * ---------------------------------------------------------------------------------------- */
/* Counter-based device noise (the inpainting loop's randn_like): out[i], i in [0, n), is the standard normal of element e = elem_offset + i
 * at iteration k -- a pure function of (seed, k, e).  r[0..3] = Philox4x32-10(counter = (g lo, g hi, k, 0), key = (seed lo, seed hi)) with
 * g = e >> 2;  u(w) = ((w >> 9) + 0.5) * 2^-23;  (z0, z1) = sqrt(-2 ln u(r0)) * (cos, sin)(2 pi u(r1)), (z2, z3) likewise from r2, r3;
 * element e takes z[e & 3].  out: device, fp32. */
int sf_op_philox_normal(uint64_t seed, uint32_t k, int64_t elem_offset, int64_t n, float *out, void *stream);
/* One launch of the inpainting loop's update on the elements [e0, e1) of whole (B, C, L) tensors (every pointer is the base of the WHOLE tensor;
 * device memory): with k = *step_idx and (a0, b0, a1, b1) = sched[4k .. 4k+3],
 *   x[e] <- mask[e] ? a1 * source[e] + b1 * z(seed, k, e) : a1 * (a0 x - b0 v) + b1 * (b0 x + a0 v),   v = v_uncond ? v_u + (v - v_u) * scale : v
 * (z as sf_op_philox_normal; seed: two 32-bit words lo, hi).  The result of an element does not depend on how [0, n) is cut into ranges, nor on
 * the alignment of the pointers (16-byte accesses only where every base allows them). */
int sf_op_vinpaint_update(float *x, const float *v, const float *v_uncond, float scale, const float *source, const uint8_t *mask,
                          const float *sched, const int32_t *step_idx, const uint32_t *seed, int64_t e0, int64_t e1, void *stream);
/* One launch of the multistep sampler's update on the elements [e0, e1) of whole tensors (every pointer is the base of the WHOLE tensor; device
 * memory): with k = *step_idx and (al, be, cx, c0, c1) = table[8k .. 8k+4] (rows of 8 floats, three unused),
 *   X = al x - be v,   x[e] <- cx x + c0 X + c1 hist[e],   hist[e] <- X,        v = v_uncond ? v_u + (v - v_u) * scale : v
 * The result of an element does not depend on how [0, n) is cut into ranges, nor on the alignment of the pointers. */
int sf_op_vsampler_update_ms(float *x, const float *v, const float *v_uncond, float scale, float *hist, const float *table,
                             const int32_t *step_idx, int64_t e0, int64_t e1, void *stream);
/* Guidance schedules at op level ("Guidance schedules").  gtab: device, rows of B guidance scales, row k = *step_idx; clip_len: elements
 * per clip; every tensor pointer is the base of the WHOLE (B, clip_len) tensor.
 * sf_op_guidance_stats: for every clip, (count, mean, M2) of v and of the guided direction  g = s == 1 ? v : v_uncond + (v - v_uncond) * s
 * (v_uncond may be NULL: g = v), reduced in fp64 without atomics into `part` (device, 8-byte aligned, sf_op_guidance_stats_bytes(B, clip_len)).
 * sf_op_vsampler_update_g: sf_op_vsampler_update_ms with that g and, where rescale = phi > 0,  v = g * (1 + phi * (std(v) / std(g) - 1))  per
 * clip, the factor combined from `part` in fp64 and rounded once to fp32 (exactly 1 where std(g) == 0).  rescale == 0: `part` is not read and may
 * be NULL.  factor_out: device, B floats, or NULL.  e1 <= B * clip_len.  The result of an element does not depend on how [0, n) is cut into
 * ranges, nor on the alignment of the pointers; a clip whose scale is exactly 1 gets the bits it gets with v_uncond == NULL. */
int64_t sf_op_guidance_stats_bytes(int B, int64_t clip_len);
int sf_op_guidance_stats(const float *v, const float *v_uncond, const float *gtab, const int32_t *step_idx, int B, int64_t clip_len, void *part,
                         int64_t part_bytes, void *stream);
int sf_op_vsampler_update_g(float *x, const float *v, const float *v_uncond, float *hist, const float *table, const float *gtab,
                            const int32_t *step_idx, const void *part, float rescale, int B, int64_t clip_len, float *factor_out, int64_t e0,
                            int64_t e1, void *stream);
/* out = conv1d(silu(groupnorm(x))) + bias (+ residual).  x:(B,L,C) and out/residual:(B,Lout,N) channels-last in
 * `dtype`; w:(N,C,taps) fp32 in PyTorch layout (packed internally); groups==0 -> no norm/activation;
 * upsample = nearest-neighbour factor applied before the convolution.  Lout = (L*upsample + 2*pad - taps)/stride + 1. */
int sf_op_conv1d_cl(int dtype, const void *x, const float *w, const float *bias, const float *gamma, const float *beta,
                    int groups, float eps, const void *residual, int B, int L, int C, int N, int taps, int stride,
                    int pad, int upsample, void *out, void *ws, int64_t ws_bytes, void *stream);
/* Training backward, first slice (the reference's training step is main/module_diffusion.py:73-82 under
 * exp/train_diffusion_gh.yaml:84-96, fp32): gradients of  y = conv1d(act(x)) + bias  with  act = silu(groupnorm(x)) when
 * groups > 0 (a ResnetItem convolution) or the identity when groups == 0 (the 1x1 InjectChannels convolution), stride 1,
 * 2 * pad == taps - 1, everything fp32 channels-last: x, dx:(B,L,C); dy:(B,L,N); w, dw:(N,C,taps) PyTorch layout; db:(N) or NULL;
 * dgb:(2C) = [dgamma | dbeta] (groups > 0).  dx may be NULL when groups == 0 and dw may be NULL (the caller needs no such gradient:
 * that part of the work is skipped).  No atomics: results are bit-reproducible. */
int64_t sf_op_conv1d_bwd_workspace_bytes(int B, int L, int C, int N, int taps, int groups);
int sf_op_conv1d_bwd_cl(const float *x, const float *w, const float *gamma, const float *beta, int groups, float eps, const float *dy,
                        int B, int L, int C, int N, int taps, int pad, float *dx, float *dw, float *db, float *dgb, void *ws,
                        int64_t ws_bytes, void *stream);
/* The training forward of the GroupNorm convolutions keeps a = silu(groupnorm(x)) and the chunk statistics the GroupNorm backward reads:
 *   sf_op_gn_silu_train: act:(B,L,C) fp32, stats: sf_op_gn_silu_train_stats_floats() floats (0: none are kept for this shape, stats may be NULL);
 *   sf_op_conv1d_bwd_cl_act = sf_op_conv1d_bwd_cl with act (and optionally stats) handed in: nothing is recomputed. */
int64_t sf_op_gn_silu_train_stats_floats(int B, int L, int C, int groups);
int sf_op_gn_silu_train(const float *x, const float *gamma, const float *beta, int groups, float eps, int B, int L, int C, float *act, float *stats,
                        void *stream);
int sf_op_conv1d_bwd_cl_act(const float *x, const float *act, const float *stats /* or NULL */, const float *w, const float *gamma, const float *beta,
                            int groups, float eps, const float *dy, int B, int L, int C, int N, int taps, int pad, float *dx, float *dw, float *db,
                            float *dgb, void *ws, int64_t ws_bytes, void *stream);
/* The same with the arithmetic of the two GEMMs chosen by `dtype`: SF_F32 (v_mfma_f32_32x32x2_f32) or SF_F32X (fp32 tensors, products from
 * split fp16 operands: data gradient through the forward kernels' split mode, weight gradient with both operands split while staged).
 * act / stats may be NULL (recomputed). */
int sf_op_conv1d_bwd_cl_x(int dtype, const float *x, const float *act, const float *stats, const float *w, const float *gamma, const float *beta,
                          int groups, float eps, const float *dy, int B, int L, int C, int N, int taps, int pad, float *dx, float *dw, float *db,
                          float *dgb, void *ws, int64_t ws_bytes, void *stream);
/* One weight-pack launch per convolution and training step.  sf_op_conv1d_train_fwd = sf_op_conv1d_cl for fp32 tensors (dtype SF_F32 /
 * SF_F32X, stride 1, no upsampling, taps <= 9) that ALSO writes the images of `w` the data-gradient GEMM of the backward pass reads into
 * dgrad_pack (>= sf_op_conv1d_dgrad_pack_bytes(C, N, taps) bytes: the flipped / transposed matrix [C][taps][N] in fp32, then its split
 * bf16 image); dgrad_pack may be NULL (then it is sf_op_conv1d_cl).  sf_op_conv1d_bwd_cl_p = sf_op_conv1d_bwd_cl_x reading those
 * images instead of packing its own (dgrad_pack NULL: packs its own).  The caller keeps dgrad_pack alive and `w` unchanged between the
 * two calls (the reference's training step: main/module_diffusion.py:79-82, optimizer step after backward). */
int64_t sf_op_conv1d_dgrad_pack_bytes(int C, int N, int taps);
int sf_op_conv1d_train_fwd(int dtype, const float *x, const float *w, const float *bias, const float *gamma, const float *beta, int groups, float eps,
                           const float *residual, int B, int L, int C, int N, int taps, int pad, float *out, void *dgrad_pack, int64_t dgrad_pack_bytes,
                           void *ws, int64_t ws_bytes, void *stream);
int sf_op_conv1d_bwd_cl_p(int dtype, const float *x, const float *act, const float *stats, const float *w, const void *dgrad_pack, const float *gamma,
                          const float *beta, int groups, float eps, const float *dy, const float *dx_add, int B, int L, int C, int N, int taps, int pad,
                          float *dx, float *dw, float *db, float *dgb, void *ws, int64_t ws_bytes, void *stream);
/* The whole weight set of a training step in ONE pack launch.  sf_op_conv1d_train_images: which images of `w` the convolution (forward, and
 * its data gradient) reads at this geometry -- bit 0 fw = [N][taps][C] fp32, bit 1 fwx = its split fp16 image, bit 2 dg = [C][taps][N] fp32
 * (taps flipped), bit 3 dgx = its split bf16 image; bit 4: not plannable (the launch wants the fragment-ordered image: use
 * sf_op_conv1d_train_fwd); < 0 on error.  `w` is read for its address alignment only (an aligned fp32 1x1 weight IS its own fw).
 * sf_train_pack_many: desc_dev = n_items x 7 64-bit words in DEVICE memory per weight -- the addresses w, fw, fwx, dg, dgx (0 = not
 * written), then N | C << 32, then taps | first_tile << 32 -- sorted by first_tile; a weight has ceil(C / 32) * ceil(N / 32) tiles,
 * total_tiles is their sum.  sf_op_conv1d_train_fwd_pk = sf_op_conv1d_train_fwd reading fw / fwx instead of packing; the backward pass
 * takes the weight's [dg | dgx] region (dgx at dg + 4 * C * taps * N bytes) as the dgrad_pack of sf_op_conv1d_bwd_cl_p. */
int sf_op_conv1d_train_images(int dtype, const float *w, int B, int L, int C, int N, int taps, int pad, int groups);
/* Which kernel sf_op_conv1d_cl(dtype, ...) launches for this geometry: writes its label (the profiling label of the GEMM variant, or
 * "conv_direct" for the thin path, C % 32 != 0) into label[label_bytes].  Query only: nothing is launched and no device is needed.  The
 * label comes from the same finished launch arguments as the real call's (tests pin a case to the kernel family it is meant for). */
int sf_op_conv1d_variant(int dtype, int B, int L, int C, int N, int taps, int stride, int pad, int upsample, int groups, char *label, int label_bytes);
/* The launches sf_op_conv1d_bwd_cl_x(dtype, ..., groups = 0) makes for this geometry (dtype SF_F32 or SF_F32X), as one string
 *   "dgrad <kernel> | <wgrad kernel> S=<row splits> <reducer> | db <column-sum kernel> Sb=<bias slices>"
 * <kernel>: the data-gradient GEMM's variant label ("<x3" in it: the split bf16 weight image is read), "conv_direct" (N % 32 != 0), or
 * "refused" (N % 32 != 0 with C > 32: the entry computes no dx for it); <wgrad kernel>: wgrad_thin<1,TQ>, or wgrad_lds<TW>/tap|rows,
 * wgrad_x3<TW>/tap|rows (single-tap or whole-rows staging); <reducer>: direct (S = 1: no reduce pass), vec or scalar; <column-sum
 * kernel>: vec4, vec1 or generic.  Query only: nothing is launched and no device is needed; it calls the plan functions the launchers
 * switch on. */
int sf_op_conv1d_bwd_variant(int dtype, int B, int L, int C, int N, int taps, int pad, char *label, int label_bytes);
int sf_train_pack_many(const void *desc_dev, int n_items, int total_tiles, void *stream);
int sf_op_conv1d_train_fwd_pk(int dtype, const float *x, const float *w, const float *fw, const void *fwx, const float *bias, const float *gamma,
                              const float *beta, int groups, float eps, const float *residual, int B, int L, int C, int N, int taps, int pad, float *out,
                              void *ws, int64_t ws_bytes, void *stream);
/* dx_add (or NULL), in sf_op_conv1d_bwd_cl_p (GroupNorm convolutions only) and sf_op_ln_modulate_bwd_add: a second gradient of x -- the one
 * arriving through the residual connection that bypasses the op (ResnetItem: x + conv2(...conv1(x)); attention: x + to_out(attn(LN(x)))) --
 * is added to dx inside the normalisation backward's own pass over the tensor, instead of by a separate element-wise launch. */
int sf_op_ln_modulate_bwd_add(const float *x, const float *scale_shift, const float *dy, const float *dx_add, float eps, int B, int L, int C, float *dx,
                              float *dss, void *ws, int64_t ws_bytes, void *stream);
/* Length reductions of the training composition (fp32, channels-last): out[b][c] = sum_l x[b][l][c] * (y ? y[b][l][c] : 1) -- the
 * gradient of a per-clip broadcast add (cross-attention over one context token) and of the SkipModulate scale
 * (a-unet SkipModulate: x + scale[:, None, :] * h).  Two deterministic stages, no atomics.
 * Any C >= 1 (16-byte vector passes where C / 4 divides 256, one column per lane otherwise).  ws >= sf_op_length_sums_workspace_bytes. */
int64_t sf_op_length_sums_workspace_bytes(int B, int L, int C);
int sf_op_length_sums(const float *x, const float *y /* or NULL */, int B, int L, int C, float *out /* (B, C) */, void *ws, int64_t ws_bytes,
                      void *stream);
/* backward of sf_op_ln_modulate (fp32): dx:(B,L,C); dss:(B,2C) = [dscale | dshift] or NULL; ws >= sf_op_ln_modulate_bwd_workspace_bytes */
int64_t sf_op_ln_modulate_bwd_workspace_bytes(int B, int L, int C);
int sf_op_ln_modulate_bwd(const float *x, const float *scale_shift, const float *dy, float eps, int B, int L, int C, float *dx, float *dss,
                          void *ws, int64_t ws_bytes, void *stream);
/* backward of sf_op_attention (fp32 matrix cores, head_dim 64): out = the forward result; dq:(B,L,H*D), dkv:(B,L,2*H*D);
 * ws >= 2 * B * H * L floats (log-sum-exp and dO.O per query) */
int sf_op_attention_bwd(const float *q, const float *kv, const float *out, const float *dout, int B, int L, int heads, int head_dim, float *dq,
                        float *dkv, void *ws, int64_t ws_bytes, void *stream);
/* The same pair with the log-sum-exp of the scaled scores, lse:(B, heads, L), kept by the forward pass and handed to the backward pass
 * (one score pass less there); fp32, head_dim 64; ws >= B * heads * L * 4 bytes. */
int sf_op_attention_fwd_lse(const float *q, const float *kv, int B, int L, int heads, int head_dim, float *out, float *lse, void *stream);
/* the same with the arithmetic chosen by `dtype` (SF_F32, or SF_F32X: products from split fp16 operands) */
int sf_op_attention_fwd_lse_x(int dtype, const float *q, const float *kv, int B, int L, int heads, int head_dim, float *out, float *lse, void *stream);
int sf_op_attention_bwd_lse(const float *q, const float *kv, const float *out, const float *dout, const float *lse, int B, int L, int heads, int head_dim,
                            float *dq, float *dkv, void *ws, int64_t ws_bytes, void *stream);
/* the same with the arithmetic chosen by `dtype` (SF_F32, or SF_F32X: scores from split fp16 operands, the gradient products from split bf16 operands) */
int sf_op_attention_bwd_lse_x(int dtype, const float *q, const float *kv, const float *out, const float *dout, const float *lse, int B, int L, int heads,
                              int head_dim, float *dq, float *dkv, void *ws, int64_t ws_bytes, void *stream);
/* Kernel tuning aid: average milliseconds of `iters` back-to-back launches of one channels-last conv1d
 * (x:(B,L,C) -> (B,L*upsample,N), `taps` taps, bias + residual epilogue) with a forced kernel family
 * (path 0 auto, 1 classic, 2 wave-split-K, 4 v2), tile variant (-1 auto) and grid split-K factor (-1 auto). */
int sf_bench_conv1d(int dtype, int B, int L, int C, int N, int taps, int upsample, int path, int tile, int sk, int iters,
                    float *ms_out);
/* The deep-level item head as the small-batch engine runs it (conv_cb.hip; a-unet ResnetItem + ModulationItem, SURVEY appendix A.3
 * items 1-2), 16-bit dtypes, C a multiple of 128, L >= 44:
 *   h = conv3(silu(groupnorm(x; gn1)), w1) + b1;  y = x + conv3(silu(groupnorm(h; gn2)), w2) + b2;
 *   m = layer_norm(y; eps_ln, no affine) * (1 + scale[b]) + shift[b]          (scale_shift (B, 2C) or NULL -> plain normalise)
 * as: gn_silu -> channel-block split-K convolution (fp32 partial slabs) -> slab reduction + bias + GroupNorm chunk sums -> the same
 * convolution with the GroupNorm+SiLU panel prologue -> slab reduction + bias + residual + LayerNorm + Modulation.
 * x, h_out (optional), m_out: (B, L, C) channels-last in `dtype`; w1, w2: (C, C, 3) fp32 PyTorch layout. */
int64_t sf_op_resnet_mod_cb_workspace_bytes(int B, int L, int C);
int sf_op_resnet_mod_cb(int dtype, const void *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *gn1_g,
                        const float *gn1_b, const float *gn2_g, const float *gn2_b, int groups, float eps_gn, const float *scale_shift,
                        float eps_ln, int B, int L, int C, int kb /* 128-channel blocks per workgroup: 1 or 2 */, void *h_out, void *m_out,
                        void *ws, int64_t ws_bytes, void *stream);
/* The same item head at the 128-channel level (C = 128: one channel block is the whole reduction and the whole row), 16-bit dtypes,
 * L a multiple of 32 and at most 1024: the convolutions finish their own results, no partial slab and no reducer launch --
 *   gn_silu -> convolution [+ b1 -> h, GroupNorm chunk statistics of the stored h] -> convolution [GroupNorm+SiLU panel prologue from
 *   those statistics; + b2 + x, LayerNorm over the row, Modulation -> m]
 * and, with w_inj set, the InjectChannels GEMM the engine launches behind them:
 *   z = m + Conv1x1(cat[m, ctx]) + b_inj (+ badd[b])     w_inj:(C, C + C2) fp32, ctx:(B, L, ctx_ld) in `dtype` (first C2 columns), badd:(B, C) or NULL
 * h_out, m_out, z_out: (B, L, C) channels-last in `dtype` (h_out, and m_out when z_out is asked for, optional).  stats_out (optional):
 * (B, nch, groups, 2) floats = (mean, M2) of h per chunk and group, as the second convolution reads them: chunks of 8 rows up to
 * L = 256, 16 up to 512, 32 beyond (nch = L / rows), the chunking and the bits of sf_op_resnet_mod_cb's reducer.
 * SF_ERR_UNSUPPORTED, before anything is launched, outside that coverage (fp32 / fp32x, C != 128, other L). */
int64_t sf_op_resnet_mod_cbd_workspace_bytes(int B, int L, int C, int C2);
int sf_op_resnet_mod_cbd(int dtype, const void *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *gn1_g,
                         const float *gn1_b, const float *gn2_g, const float *gn2_b, int groups, float eps_gn, const float *scale_shift,
                         float eps_ln, int B, int L, int C, const float *w_inj, const float *b_inj, const void *ctx, int ctx_ld, int C2,
                         const float *badd, void *h_out, void *m_out, void *z_out, float *stats_out, void *ws, int64_t ws_bytes, void *stream);
/* The item tail of the thin levels in one launch (conv_thin.hip, thin_tail: the second half of a ResnetItem, the ModulationItem and the
 * InjectChannelsItem on the 8-, 32- and 64-channel levels), as the engine launches it behind the item's first convolution:
 *   y = x + conv3(silu(groupnorm(h; gn)), w2) + b2;  m = layer_norm(y; eps_ln, no affine) * (1 + scale[b]) + shift[b];
 *   z = m + Conv1x1(cat[m, ctx]) + b_inj (+ badd[b])
 * h, x, z_out: (B, L, C) channels-last in `dtype`; ctx: (B, L, ctx_ld), its first C2 columns are read, of which c2_real carry weights
 * (w_inj: (C, C + c2_real) fp32, zero-extended to C2 columns here; the engine pads its context rows to whole octets); w2: (C, C, 3) fp32;
 * scale_shift: (B, 2C), required; badd: (B, C) or NULL.  The GroupNorm statistics of h are not computed here: stats_in is
 * (B, nch_in, groups, 2) floats = (mean, M2) of h per chunk of chunk_in rows (the last chunk short) and group, as the producing
 * convolution leaves them.  rw: positions per workgroup, a multiple of 32; 0 takes the engine's plan (*rw_out, optional, receives the
 * value used).  stats_out (optional): (B, ceil(L / rw), groups, 2) = (mean, M2) of the stored z per workgroup and group.
 * C / C2: 8 / 8, 32 / 32, 64 / 32 or 64 / 64 with 4 or 8 channels per group (one at C = 8); anything else, or an rw the kernel cannot
 * stage, is SF_ERR_UNSUPPORTED before anything is launched. */
int64_t sf_op_thin_tail_workspace_bytes(int dtype, int C, int C2);
int sf_op_thin_tail(int dtype, const void *h, const void *x, const void *ctx, int ctx_ld, int c2_real, int C2, const float *stats_in, int nch_in,
                    int chunk_in, const float *w2, const float *b2, const float *gn_g, const float *gn_b, int groups, float eps_gn,
                    const float *scale_shift, float eps_ln, const float *w_inj, const float *b_inj, const float *badd, int B, int L, int C, int rw,
                    void *z_out, float *stats_out, int *rw_out, void *ws, int64_t ws_bytes, void *stream);
/* InjectChannels followed by the attention pre-norm projection, as the engine chains the two GEMMs of an item (a-unet InjectChannelsItem
 * + the LayerNorm / to_q | to_kv Linear of AttentionItem), 16-bit dtypes:
 *   z = m + Conv1x1(cat[m, ctx]) + b_inj            m:(B,L,C), ctx:(B,L,C2) channels-last in `dtype`; w_inj:(C, C + C2) fp32
 *   q = Linear(LayerNorm_C(z; gamma, beta, eps))    w_q:(N, C) fp32, bias-free
 * The first GEMM's epilogue leaves per-row LayerNorm partials per 32-column tile, the second multiplies the RAW rows of z and
 * normalises its accumulator, rstd * (acc - mean * colsum) -- no LayerNorm launch in between.  Which kernel family runs (macro tiles at
 * long activations, the 32x32 families at short ones) follows the engine's dispatch, except that the macro-tile form is always offered
 * here (the engine does not take it: in the two-branch step it measured no gain); SF_ERR_UNSUPPORTED where no kernel fits.
 * fused_out (optional): set to 1 when the fused pair ran, 0 when the op fell back to z -> ln_modulate -> plain projection. */
int64_t sf_op_inject_prenorm_proj_workspace_bytes(int B, int L, int C, int C2, int N);
int sf_op_inject_prenorm_proj(int dtype, const void *m, const void *ctx, const float *w_inj, const float *b_inj, const float *gamma,
                              const float *beta, float eps, const float *w_q, int B, int L, int C, int C2, int N, void *z_out, void *q_out,
                              int *fused_out, void *ws, int64_t ws_bytes, void *stream);
/* ONE implicit-GEMM launch with the whole epilogue of the small-batch kernels exposed, for element-wise tests of the epilogue operands and
 * of the statistics a launch leaves for the next one (tests/gemm_epilogue_ref.py; no reference counterpart).  Channels-last rows:
 *   out = act((conv(nearest_up(x)) | x2 . w + bias) * bscale[b] + residual + badd[b])        Lout = (L * upsample + 2 pad - taps) / stride + 1
 * x (B, L, C) and x2 (B, Lout, C2; optional, taps == 1) and residual (B, Lout, N) in `dtype`; w is the GEMM's own matrix (N, taps * C + C2)
 * in fp32, column tap * C + c for the first source and taps * C + c2 for the second, 16-byte aligned; bias (N), bscale and badd (B, N) fp32;
 * act 0 none, 1 relu, 2 gelu(erf), 3 silu(gelu); out (B, Lout, N) in `dtype`, or fp32 when out_f32.  C, C2 multiples of 32.
 * Optional outputs, written only where the dispatcher's plan for these arguments honours them (the *_done flags say so; a declined one is
 * left untouched):  rowpart (B * Lout, N / 32, 2) = (mean, M2) of each row's 32 STORED values per column tile;  gnpart
 * (ceil(B * Lout / 32), N / 32, 2, 2) = (mean, M2) of the stored values of each 32 x 32 tile over its rows of the first row's clip
 * (segment 0) and of the next clip (segment 1); an empty segment is (0, 0).
 * The LayerNorm-consumer launch (sf_op_conv1d_ln, taps == 1): the first source is read as LayerNorm_C(x; ln_eps), its row statistics pooled
 * from ln_part (B * L, C / 32, 2) in rowpart's layout.  ln_operand == 0: accumulator side -- the raw rows are multiplied and the epilogue
 * applies rstd * (acc - mean * colsum(w)), the column sums taken of the packed weight as the engine takes them.  ln_operand == 1: the operand
 * is transformed, LayerNorm(x) * (1 + ln_ss[b][c]) + ln_ss[b][C + c] with ln_ss (B, 2 C) fp32 or NULL; res_ln: the residual (N == C) gets
 * the same transform.  mt_ln offers the macro-tile form of both fusions; solo says that nothing runs beside the launch.
 * Both launches size their workspace with sf_op_conv1d_epi_workspace_bytes.  Every entry refuses with SF_ERR_UNSUPPORTED before anything is
 * launched (the weight images are packed behind the plan) where no kernel takes the arguments.  The _variant queries need
 * no device and take no data pointers' contents: only whether an optional pointer is set enters the plan; they return the label of the
 * kernel and the flags from the same finished launch arguments as the real call.
 * src_x3 != 0 (sf_op_conv1d_epi and its query only): x holds pre-split rows, as a producer with xfmt writes them (sf_op_gn_silu_rows below):
 * row m is C * 4 bytes, [C / 32][hi 32 x fp16 | lo' 32 x fp16] with hi = fp16(v), lo' = fp16((v - hi) * 2048).  Honoured only by the
 * macro-tile kernel on SF_F32X with C2 == 0: every other dtype, a second source, or a shape whose plan does not read pre-split rows is
 * SF_ERR_UNSUPPORTED before anything is packed or launched, from the launch and from the query alike. */
typedef struct {
  int32_t dtype, B, L, C, C2, N, taps, stride, pad, upsample, act, out_f32, mt_ln, res_ln, ln_operand, solo;
  float ln_eps;
  int32_t src_x3;
  const void *x, *x2;
  const float *w, *bias, *bscale, *badd;
  const void *residual;
  void *out;
  float *rowpart, *gnpart;
  const float *ln_part, *ln_ss;
} sf_conv1d_epi_desc;
int64_t sf_op_conv1d_epi_workspace_bytes(const sf_conv1d_epi_desc *d);
int sf_op_conv1d_epi(const sf_conv1d_epi_desc *d, int *rowpart_done, int *gnpart_done, void *ws, int64_t ws_bytes, void *stream);
int sf_op_conv1d_epi_variant(const sf_conv1d_epi_desc *d, char *label, int label_bytes, int *rowpart_done, int *gnpart_done);
int sf_op_conv1d_ln(const sf_conv1d_epi_desc *d, int *rowpart_done, void *ws, int64_t ws_bytes, void *stream);
int sf_op_conv1d_ln_variant(const sf_conv1d_epi_desc *d, char *label, int label_bytes, int *rowpart_done);
/* The channel-block convolution behind the TILE statistics a producing GEMM leaves (conv_cb prologue 2, then cb_reduce_gn), bf16 / fp16 /
 * fp32x:   h = Conv1d_k3(SiLU(GroupNorm(x; groups, gn_g, gn_b, eps))) + bias        x, h: (B, L, C) channels-last in `dtype`, w (C, C, 3) fp32.
 * tile_stats is read in gnpart's layout, (ceil(B * L / 32), C / 32, 2, 2) fp32: (mean, M2) of x per 32-row x 32-column tile and clip segment.
 * stats_out (B, nch, groups, 2) receives the reducer's chunk statistics of the stored h ((mean, M2) per chunk of chunk_rows rows; the two
 * counts are returned, nch <= 32).  SF_ERR_UNSUPPORTED before anything is launched where the convolution or its prologue does not take the
 * shape (C a power-of-two multiple of 128 up to 1024, L >= 44, C / groups a power of two >= 32, at most 32 tiles per clip and group). */
int64_t sf_op_conv_cb_tiles_workspace_bytes(int dtype, int B, int L, int C);
int sf_op_conv_cb_tiles(int dtype, const void *x, const float *w, const float *bias, const float *gn_g, const float *gn_b, int groups, float eps,
                        const float *tile_stats, int B, int L, int C, void *h_out, float *stats_out, int *nch_out, int *chunk_rows_out, void *ws,
                        int64_t ws_bytes, void *stream);
/* Kernel tuning aid: average milliseconds of the four launches of that chain on random data (ms[0] convolution, ms[1] reduction +
 * GroupNorm sums, ms[2] convolution with prologue, ms[3] reduction + LayerNorm); cold != 0 streams the weights from HBM. */
int sf_bench_conv_cb(int dtype, int B, int L, int C, int groups, int kb, int cold, int iters, float *ms /* [4] */);
/* y = layer_norm(x; eps, no affine) * (1 + scale[b]) + shift[b]   (scale/shift NULL -> plain normalise) */
/* materialised SiLU(GroupNorm(x)) on channels-last rows (B, L, C), as the wide U-Net levels run it in front of their convolutions
 * (a-unet ResnetItem).  ws (optional, >= B * 32 * groups * 2 floats): long sequences then take the
 * chunked form (per-chunk statistics + one streaming pass) instead of one workgroup per (clip, group). */
int sf_op_gn_silu(int dtype, const void *x, const float *gamma, const float *beta, int groups, float eps, int B, int L, int C, void *out,
                  void *ws, int64_t ws_bytes, void *stream);
int sf_op_ln_modulate(int dtype, const void *x, const float *scale_shift /* (B, 2C) or NULL */, float eps,
                      int B, int L, int C, void *out, void *stream);
/* multi-head attention on packed projections: q:(B,L,H*D), kv:(B,L,2*H*D) -> out:(B,L,H*D) */
int sf_op_attention(int dtype, const void *q, const void *kv, int B, int L, int heads, int head_dim, void *out, void *stream);
/* The three operations above as the engine launches them in front of a GEMM, with the output row stride and the row format exposed.
 * xfmt != 0: the output rows are written pre-split for a GEMM that takes sf_conv1d_epi_desc::src_x3 (the layout is described there)
 * instead of as floats; the buffer has the same size either way.  What the launcher does not take is SF_ERR_UNSUPPORTED before anything
 * is launched: with xfmt, any dtype but SF_F32 (norms) / SF_F32X (attention), C % 32 != 0, out_ld != C (ldo != heads * head_dim),
 * (C / groups) % 4 != 0.
 * sf_op_attention_rows takes the row strides of q, kv and out in elements: kv points at the row's keys, its values follow heads * head_dim
 * columns later, and kv may point into the buffer q points into (the engine's packed q | k | v rows: ldq = ldkv = 3 * heads * head_dim,
 * kv = q + heads * head_dim). */
int sf_op_gn_silu_rows(int dtype, const void *x, const float *gamma, const float *beta, int groups, float eps, int B, int L, int C, void *out,
                       int out_ld, int xfmt, void *stream);
int sf_op_ln_modulate_rows(int dtype, const void *x, const float *scale_shift /* (B, 2C) or NULL */, float eps, int B, int L, int C, void *out,
                           int out_ld, int xfmt, void *stream);
int sf_op_attention_rows(int dtype, const void *q, int ldq, const void *kv, int ldkv, int B, int L, int heads, int head_dim, void *out, int ldo,
                         int xfmt, void *stream);


/* ---- VideoOnsetNet training (fp32; main/module_onset.py trains main/onset_net.py:46-63 in fp32) ----------------------------------------
 * Video activations are channels-last rows: x row ((n*T + t)*Hi + hi)*Wi + wi with cin_ld columns, y row ((n*T + t)*Ho + ho)*Wo + wo with cout_ld
 * columns; columns past the real channel count hold zeros (inputs must, outputs are written so).  Weights and their gradients are PyTorch's
 * Conv3d layout (cout, cin, kt, kh, kw), fp32, no bias.  Temporal stride 1, 2 pt == kt - 1; Ho = (Hi + 2 ph - kh) / sh + 1 (likewise Wo).
 * Needs cin_ld % 4 == 0, cout_ld % 8 == 0.  ws >= sf_op_vconv_workspace_bytes(desc) (the same bound for the forward and backward calls).
 * sf_op_vconv_bwd: dx (input rows, cin_ld columns) and / or dw (either may be NULL); the data gradient supports stride-1 'same' convolutions and
 * (1, kh, kw) kernels of any spatial stride.  No atomics: the results are bit-reproducible. */
typedef struct {
  int32_t N, T, Hi, Wi;      /* clips, frames per clip, input frame size */
  int32_t cin, cin_ld;       /* input channels, input row length (floats) */
  int32_t cout, cout_ld;     /* output channels, output row length (floats) */
  int32_t kt, kh, kw;        /* kernel */
  int32_t sh, sw;            /* spatial stride */
  int32_t pt, ph, pw;        /* zero padding */
} sf_vconv_desc;
int64_t sf_op_vconv_workspace_bytes(const sf_vconv_desc *desc /* host */);
int sf_op_vconv_fwd(const sf_vconv_desc *desc, const float *x, const float *w, float *y, void *ws, int64_t ws_bytes, void *stream);
int sf_op_vconv_bwd(const sf_vconv_desc *desc, const float *x, const float *w, const float *dy, float *dx, float *dw, void *ws, int64_t ws_bytes,
                    void *stream);
/* BatchNorm3d in train mode over channels-last rows (rows, ld), C real channels (rows >= 2, ld % 4 == 0):
 *   y = act(xhat * gamma + beta + res),  xhat = (x - mean) / sqrt(var + eps),  mean / var (biased) over all rows;  res (rows, ld) or NULL,
 *   act = ReLU when relu != 0.  save_mean / save_invstd (C): mean and 1 / sqrt(var + eps) for the backward call.  running_mean / running_var
 *   (C, or NULL) <- (1 - momentum) * running + momentum * (mean | var * rows / (rows - 1));  *num_batches_tracked (int64, or NULL) += 1.
 * sf_op_bn_train_bwd: dy = the gradient of y;  y = the forward output when relu was on (its mask), else NULL;  dx = gamma * invstd *
 *   (dz - mean(dz) - xhat * mean(dz * xhat)) with dz = dy masked;  dres (or NULL) = dz, the residual's gradient;  dgamma / dbeta (C, or NULL).
 *   Per-channel sums are taken per row slice and merged in a fixed order (deterministic).  ws >= sf_op_bn_train_workspace_bytes. */
int64_t sf_op_bn_train_workspace_bytes(int64_t rows, int C);
int sf_op_bn_train_fwd(const float *x, const float *res, int64_t rows, int C, int ld, const float *gamma, const float *beta, float eps, float momentum,
                       float *running_mean, float *running_var, int64_t *num_batches_tracked, int relu, float *y, float *save_mean, float *save_invstd,
                       void *ws, int64_t ws_bytes, void *stream);
int sf_op_bn_train_bwd(const float *x, const float *y, const float *dy, int64_t rows, int C, int ld, const float *gamma, const float *save_mean,
                       const float *save_invstd, float *dx, float *dres, float *dgamma, float *dbeta, void *ws, int64_t ws_bytes, void *stream);
/* The same BatchNorm with statistics shared by the `world` ranks of a data-parallel group (torch.nn.SyncBatchNorm), in split phases: each direction
 * is cut where the per-channel numbers are small, and the CALLER runs one all-gather of 2 * C floats there (this library links no collective library).
 *   sf_op_bn_sync_stats      local_stats (C, 2) = (mean, M2 = sum (x - mean)^2) of this rank's rows; rows >= 1 (a rank may hold a single row)
 *   sf_op_bn_sync_fwd_apply  gathered_stats (world, C, 2): every rank's local_stats in rank order;  row_counts (world) int64, DEVICE memory: every
 *                            rank's row count (exact integers; their sum must be >= 2).  Merges the table in rank order (the mean about rank 0's mean,
 *                            then M2 = sum M2_r + n_r (mean_r - mean)^2), then as sf_op_bn_train_fwd: save_mean / save_invstd, the running statistics
 *                            (unbiased over the TOTAL row count), *num_batches_tracked += 1, y.  Identical input gives identical bits on every rank.
 *   sf_op_bn_sync_bwd_sums   local_sums (C, 2) = (sum dz, sum dz * xhat) of this rank's rows;  dgamma / dbeta (C, or NULL) are these LOCAL sums, as
 *                            in torch.nn.SyncBatchNorm (the gradient all-reduce averages them afterwards)
 *   sf_op_bn_sync_bwd_apply  gathered_sums (world, C, 2) added in rank order, divided by the total row count, then dx / dres as sf_op_bn_train_bwd
 * No atomics; the merge order is fixed, so the results are bit-reproducible.  ws >= sf_op_bn_sync_workspace_bytes(rows, C) for all four calls. */
int64_t sf_op_bn_sync_workspace_bytes(int64_t rows, int C);
int sf_op_bn_sync_stats(const float *x, int64_t rows, int C, int ld, float *local_stats, void *ws, int64_t ws_bytes, void *stream);
int sf_op_bn_sync_fwd_apply(const float *x, const float *res, int64_t rows, int C, int ld, const float *gathered_stats, const int64_t *row_counts, int world,
                            const float *gamma, const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                            int64_t *num_batches_tracked, int relu, float *y, float *save_mean, float *save_invstd, void *ws, int64_t ws_bytes,
                            void *stream);
int sf_op_bn_sync_bwd_sums(const float *x, const float *y, const float *dy, int64_t rows, int C, int ld, const float *save_mean, const float *save_invstd,
                           float *local_sums, float *dgamma, float *dbeta, void *ws, int64_t ws_bytes, void *stream);
int sf_op_bn_sync_bwd_apply(const float *x, const float *y, const float *dy, int64_t rows, int C, int ld, const float *gathered_sums,
                            const int64_t *row_counts, int world, const float *gamma, const float *save_mean, const float *save_invstd, float *dx,
                            float *dres, void *ws, int64_t ws_bytes, void *stream);
/* layout step: frames (N, C, T, H, W) fp32 -> channels-last rows (N*T*H*W, ld), zeros in columns [C, ld) */
int sf_op_video_to_cl(const float *x, int N, int C, int T, int H, int W, int ld, float *out, void *stream);
/* AdaptiveAvgPool3d((None, 1, 1)): x rows (NT*HW, ld) -> out (NT, C);  _bwd: dx rows (NT*HW, ld) = dout[nt] / HW (zeros in [C, ld)) */
int sf_op_video_pool(const float *x, int64_t NT, int HW, int C, int ld, float *out, void *stream);
int sf_op_video_pool_bwd(const float *dout, int64_t NT, int HW, int C, int ld, float *dx, void *stream);

/* The end of the onset training step (main/module_onset.py:268-354, BCLoss) from device memory to device memory: nothing is read back and
 * nothing that changes per step is an argument, so the calls can sit inside a captured graph.  z: n fp32 logits, t: n fp32 labels (0 / 1).
 *   sf_op_onset_bce_fwd   *loss = mean(pw t softplus(-z) + (1 - t) softplus(z)), pw = (n - sum t) / sum t computed on the device;
 *                         stats[2] = (sum t, pw) for the backward call.  sum t == 0 gives pw = inf and a NaN loss, as the reference does.
 *   sf_op_onset_bce_bwd   dz = *g / n * ((1 - t) sigmoid(z) - pw t (1 - sigmoid(z)));  g: the upstream scalar gradient, DEVICE memory.
 *   sf_op_onset_metrics   z, t as (N, T) rows, N * T <= 2^24;  out[3] (fp64, device) = AP, Acc, OnsNumAcc of BCLoss.evaluate: scores are the
 *                         fp32 sigmoid of z; the balanced subset is the first b = min(#(t == 1), #(t == 0)) positives and negatives in
 *                         row-major order; AP = 1/b sum over the subset's positives i of TP(s >= s_i) / CNT(s >= s_i) (sklearn's step-wise
 *                         average precision, tied scores as one threshold, in integer counts); Acc = share of the subset with
 *                         (s > threshold) == t; OnsNumAcc = share of rows whose thresholded predictions, each run of L consecutive ones
 *                         reduced to ceil(L / 2) (the reference's left-to-right suppression), count as many as the row's labels.
 *                         b == 0 (one class only): AP = Acc = NaN, OnsNumAcc as usual.
 * Every reduction runs in a fixed order without floating-point atomics: identical input gives identical bits.  ws: 8-byte aligned,
 * >= sf_op_onset_loss_workspace_bytes(n) (one bound for the three calls at n = N * T; -1 for n < 1 or n >= 2^31). */
int64_t sf_op_onset_loss_workspace_bytes(int64_t n);
int sf_op_onset_bce_fwd(const float *z, const float *t, int64_t n, float *loss, float *stats, void *ws, int64_t ws_bytes, void *stream);
int sf_op_onset_bce_bwd(const float *z, const float *t, const float *stats, const float *g, int64_t n, float *dz, void *stream);
int sf_op_onset_metrics(const float *z, const float *t, int N, int T, float threshold, double *out, void *ws, int64_t ws_bytes, void *stream);

/* The device step of the onset net's test stage (main/module_onset.py:99-125 test_step, :142-183 log_annotations) for one batch of (N, T)
 * fp32 logits and fp32 0 / 1 labels, from device memory to device memory: nothing is read back, nothing synchronises.
 *   rows   table row r = clip0 + n of clip n: pred_frames[r, 0 .. pred_count[r]) = the frames t with logits[n, t] > logit_threshold in
 *          ascending order (the reference thresholds the RAW logit at 0.5, :160-162; a NaN logit is no onset), the rest of the row -1;
 *          target_count / target_frames the same for labels[n, t] != 0 (np.nonzero).  Tables: (capacity) and (capacity, T) int32; rows
 *          outside [clip0, clip0 + N) are not touched.  A clip's rows depend on that clip only.
 *   sums   sums[5] (fp64) += (N loss, N AP, N Acc, N OnsNumAcc, N): loss as sf_op_onset_bce_fwd, the metrics as sf_op_onset_metrics at
 *          metric_threshold (0.75, on the sigmoid) give them for this batch, bit for bit; one thread adds in this order, NaN and inf
 *          propagate (a one-class batch: NaN AP / Acc).  sums[k] / sums[4] is the epoch mean weighted by batch size.
 * N * T <= 2^24 (SF_ERR_UNSUPPORTED above), clip0 + N <= capacity (SF_ERR_SHAPE), ws and sums 8-byte aligned,
 * ws_bytes >= sf_op_onset_test_workspace_bytes(N, T) (-1 for N < 1, T < 1 or N * T > 2^24). */
int64_t sf_op_onset_test_workspace_bytes(int N, int T);
int sf_op_onset_test_step(const float *logits, const float *labels, int N, int T, float logit_threshold, float metric_threshold, int64_t clip0,
                          int64_t capacity, int32_t *pred_count, int32_t *pred_frames, int32_t *target_count, int32_t *target_frames,
                          double *sums, void *ws, int64_t ws_bytes, void *stream);

/* The optimizer stage of a training step: clip-by-global-norm and the AdamW update of EVERY listed tensor in three launches (two without
 * clipping).  Replaces torch.nn.utils.clip_grad_norm_ (a per-tensor norm pass and a read-modify-write scaling pass over the gradients)
 * followed by torch.optim.AdamW(fused=True).step() (exp/train_diffusion_gh.yaml:91-92 gradient_clip_val, main/module_diffusion.py:53-62 and
 * main/module_onset.py AdamW), for fp32 contiguous tensors, amsgrad = False, maximize = False.
 *   desc_dev   DEVICE memory, n_tensors records of 8 64-bit words, sorted by first_chunk: the addresses p, g, exp_avg, exp_avg_sq, step (an
 *              fp32 scalar per tensor, as torch keeps it for its fused path), then the element count, then group | first_chunk << 32, then 0.
 *              A tensor of n elements has ceil(n / SF_OPTIM_CHUNK) chunks; first_chunk is the running sum, total_chunks the total.
 *   hyper_dev  DEVICE memory, (1 + n_groups) * 8 doubles: [0] max_norm; group g at 8 + 8 g: lr, beta1, beta2, eps, weight_decay.  Read by
 *              the kernels at every call: a new learning rate is one small copy, also for a captured graph.
 *   clip       1: total_norm = global L2 norm of the g, clip_coef = min(1, max_norm / (total_norm + 1e-6)); the update uses g * clip_coef,
 *              g in memory is NOT scaled (clip_grad_norm_ scales .grad in place).  0: no norm pass, clip_coef = 1.
 *   result_dev two floats: total_norm (written when clip = 1), clip_coef.
 * Every step is incremented once per call; per element  p -= lr wd p;  m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;
 * p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps).  No atomics: identical input gives identical bits.  Non-finite
 * gradients get no special treatment.  ws: 16-byte aligned, >= sf_optim_workspace_bytes(total_chunks) (-1 for total_chunks < 1). */
#define SF_OPTIM_CHUNK 16384
int64_t sf_optim_workspace_bytes(int total_chunks);
int sf_optim_adamw_step(const void *desc_dev, int n_tensors, int total_chunks, const void *hyper_dev, int n_groups, int clip, float *result_dev,
                        void *ws, int64_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Audio front end of the onset-sync evaluation (syncfusion_amd/audio_features.py, evaluation.py)
 *   replaces: librosa.onset.onset_detect(y=wav, sr=22050, units='samples', delta=0.3) at script/evaluate_onset.py:30 (log-mel spectrogram,
 *   spectral flux, peak picking), the waveform confidences of eval_osnets (script/evaluate_onset.py:52-54), and the
 *   torchaudio.transforms.MelSpectrogram + power_to_db pair of SampleLogger (main/module_diffusion.py:120-152).
 * All tensors fp32 (counts and positions int32), contiguous, on the device; T = 1 + L / hop frames (center = True).
 *
 * sf_audio_features_create   HOST-only: checks the configuration and builds the periodic Hann window and the twiddle table in fp64
 *     (rounded once to fp32).  n_fft: a power of two in [256, 4096]; hop, n_mels >= 1; pad_mode 0 = constant (zeros), 1 = reflect (no
 *     edge repeat, as torch.stft).  The mel filterbank comes from the host in compact form: filter m touches bins first_bin[m] ..
 *     first_bin[m] + bin_count[m] - 1 (bin_count >= 1, inside 0 .. n_fft / 2) with the weights packed one filter after the other
 *     (n_weights = sum of bin_count).  The tables are copied to the device once, at the first forward call on the handle.
 * sf_audio_features_workspace_bytes   one bound for both calls (monotone in B and L; -1 for a null handle, B < 1 or L < 1).
 * sf_logmel_forward   wav (B, L) -> mel_power (B, n_mels, T) and / or db (B, n_mels, T), either may be NULL (not both):
 *     frame t = samples [t hop - n_fft / 2, t hop + n_fft / 2) of the padded clip, times the window, n_fft-point real DFT, |X_k|^2,
 *     filterbank;  db = max(10 log10(max(amin, P)), max over the clip's plane - top_db)  (power_to_db with ref = 1).
 * sf_onset_detect     the whole detector in one call: envelope (B, T), count (B), positions / confidence / strength (B, capacity).
 *     d[t] = mean_m max(0, db[m, t] - db[m, t - lag]) for t >= lag; envelope = lag + n_fft / (2 hop) zero frames followed by those
 *     values, cut to T frames (d[t] lands at frame t + n_fft / (2 hop)).  An all-zero envelope has no onsets.  Otherwise
 *     x = (e - min e) / (max(e - min e) + FLT_MIN) and frame n is an onset when x[n] is the maximum of x[max(0, n - pre_max) :
 *     min(T, n + post_max)], x[n] >= mean(x[max(0, n - pre_avg) : min(T, n + post_avg)]) + delta, and n - previous onset > wait.
 *     positions = n hop (samples, ascending; unused slots -1); confidence = max(w[max(0, o - conf_interval) : min(L, o + conf_interval)])
 *     and strength = w[o] (0 where o == L) with w = (|wav| - min |wav|) / (max |wav| - min |wav|); unused slots 0.
 *     count[b] = -1 when clip b has more than `capacity` onsets (nothing is truncated silently; capacity = T can never overflow).
 * Refused before any HIP call: null pointers, B < 1, L < 1 (SF_ERR_INVALID); reflect padding with L <= n_fft / 2, B > 65535 or
 * B n_mels T >= 2^31 (SF_ERR_SHAPE); a workspace below the query (SF_ERR_WORKSPACE); lag, post_max, post_avg, conf_interval,
 * capacity < 1, pre_max, pre_avg, wait < 0, amin <= 0, top_db < 0 (SF_ERR_INVALID).  A clip's results do not depend on the rest of
 * the batch (fixed-order reductions, no atomics). */
typedef struct sf_audio_features sf_audio_features;
enum { SF_PAD_CONSTANT = 0, SF_PAD_REFLECT = 1 };
int sf_audio_features_create(int n_fft, int hop, int n_mels, int pad_mode, const int32_t *first_bin /*host*/, const int32_t *bin_count /*host*/,
                             const float *weights /*host*/, int64_t n_weights, sf_audio_features **out);
void sf_audio_features_destroy(sf_audio_features *h);
int64_t sf_audio_features_workspace_bytes(const sf_audio_features *h, int B, int L);
int sf_logmel_forward(sf_audio_features *h, const float *wav, int B, int L, float amin, float top_db, float *mel_power, float *db, void *ws,
                      int64_t ws_bytes, void *stream);
int sf_onset_detect(sf_audio_features *h, const float *wav, int B, int L, float amin, float top_db, int lag, int pre_max, int post_max,
                    int pre_avg, int post_avg, int wait, float delta, int conf_interval, int capacity, float *envelope, int32_t *count,
                    int32_t *positions, float *confidence, float *strength, void *ws, int64_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Complex STFT, inverse STFT and the spectral-gating denoiser (syncfusion_amd/denoise.py)
 *   replaces: noisereduce.reduce_noise(x, sr, n_fft=1024, hop_length=256) of the --audio_denoise step at script/gh_preprocess_videos.py:91-100.
 * All tensors fp32, contiguous, on the device.  A spectrum is stored (B, T, F, 2): F = n_fft / 2 + 1 interleaved complex bins per frame.
 *
 * sf_spectral_gate_create   HOST-only: checks the configuration and builds the periodic Hann window of win_length points (zeros behind it
 *     up to n_fft, as scipy pads a frame at its END) and the twiddle table in fp64, rounded once.  n_fft: a power of two in [256, 4096];
 *     2 <= win_length <= n_fft; hop >= 1; center != 0 pads win_length / 2 samples on each side of the clip (pad_mode 0 = zeros, 1 =
 *     reflect) and gives T = (L + 2 (win_length / 2) - win_length) / hop + 1 frames, center == 0 gives T = (L - win_length) / hop + 1;
 *     samples behind the last whole frame are not transformed.  scale_spectrum != 0 divides the bins by sum(w) (scipy's "spectrum") and the
 *     inverse undoes it.  freq_taps / time_taps (host): the two odd-length factors of the separable mask filter, each summing to 1; {1}
 *     is the identity.
 * sf_spectral_gate_frames   T for a row of L samples; -1 for a null handle or L < win_length.
 * sf_spectral_gate_workspace_bytes   one bound for every call below on (B, L) (-1 for a null handle, B < 1 or L < win_length);
 *     for sf_istft_forward take L = win_length + (T - 1) hop - 2 pad.
 * sf_stft_forward    wav (B, L) -> spec (B, T, F, 2).
 * sf_istft_forward   spec (B, T, F, 2) -> out (B, out_len): per frame the inverse real transform (the imaginary parts of bins 0 and
 *     n_fft / 2 do not enter), times the window; each output sample is the sum, in ascending frame order, of the frames that cover it
 *     divided by the sum of their squared window values (1 where that sum is below 1e-10).  win_length + (T - 1) hop - 2 pad samples
 *     exist; out is cut there or filled with zeros up to out_len.  hop need not divide win_length.
 * sf_spectral_gate_noise_threshold   noise (B, L) -> thresh (B, F) = mean_t dB + n_std std_t dB (ddof 0, two passes) with
 *     dB = 20 log10(max(|S|, 1e-20)) floored at the row's plane maximum - 80.
 * sf_spectral_gate   the whole denoiser on B independent rows: spec = STFT(wav);
 *     stationary == 0: sm = |spec| filtered forward and then backward over frames by y = smooth_b x + (1 - smooth_b) y_prev, each pass
 *       started from its first input; mask_raw = sigmoid(((|spec| - sm) / sm - thresh_mult) slope), 0 where sm == 0;
 *     stationary != 0: mask_raw = (dB > thresh[row, bin]) as 0 / 1;
 *     mask_smooth = filter(mask_raw) prop_decrease + (1 - prop_decrease), or, with prop_before_smoothing != 0,
 *       filter(mask_raw prop_decrease + (1 - prop_decrease)) (the two differ where the filter reaches outside the plane);
 *     filter = freq_taps over bins, then time_taps over frames, zeros outside the plane;  out (B, L) = ISTFT(spec mask_smooth).
 *     spec, mask_raw (B, T, F) and mask_smooth (B, T, F) are outputs as well.
 * Refused before any HIP call: null pointers, B < 1, L < 1, n_std < 0, smooth_b outside (0, 1], prop_decrease outside [0, 1], and in the
 * two calls that invert a window / hop pair that violates NOLA (min over n < hop of sum_k w[n + k hop]^2 <= 1e-10, evaluated in fp64 at
 * create) (SF_ERR_INVALID); L < win_length, reflect padding with L <= win_length / 2, B > 65535 or B T F >= 2^31 (SF_ERR_SHAPE); a
 * workspace below the query (SF_ERR_WORKSPACE).  A row's results do not depend on the rest of the batch (fixed-order sums, no atomics). */
typedef struct sf_spectral_gate_handle sf_spectral_gate_handle;
int sf_spectral_gate_create(int n_fft, int win_length, int hop, int center, int pad_mode, int scale_spectrum, const float *freq_taps /*host*/,
                            int n_freq_taps, const float *time_taps /*host*/, int n_time_taps, sf_spectral_gate_handle **out);
void sf_spectral_gate_destroy(sf_spectral_gate_handle *h);
int sf_spectral_gate_frames(const sf_spectral_gate_handle *h, int L);
int64_t sf_spectral_gate_workspace_bytes(const sf_spectral_gate_handle *h, int B, int L);
int sf_stft_forward(sf_spectral_gate_handle *h, const float *wav, int B, int L, float *spec, void *stream);
int sf_istft_forward(sf_spectral_gate_handle *h, const float *spec, int B, int T, float *out, int out_len, void *ws, int64_t ws_bytes, void *stream);
int sf_spectral_gate_noise_threshold(sf_spectral_gate_handle *h, const float *noise, int B, int L, float n_std, float *thresh, void *ws,
                                     int64_t ws_bytes, void *stream);
int sf_spectral_gate(sf_spectral_gate_handle *h, const float *wav, int B, int L, int stationary, float smooth_b, float thresh_mult, float slope,
                     float prop_decrease, int prop_before_smoothing, const float *thresh, float *spec, float *mask_raw, float *mask_smooth, float *out, void *ws,
                     int64_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * FAD evaluation (syncfusion_amd/fad.py)
 *   replaces: main.evaluation.evaluate_fad (main/evaluation.py:7-28, the config.evaluation target of script/evaluate_diffusion.py:31-36):
 *   frechet_audio_distance.FrechetAudioDistance(model_name="vggish", use_pca=False, use_activation=False) -- the VGGish input features
 *   (vggish_input.py / mel_features.py), the torch.hub VGGish network and the embedding statistics.  The Frechet distance itself is
 *   host arithmetic (fad.py).  All tensors fp32 unless stated, contiguous, on the device.
 *
 * sf_audio_features_create_framed   HOST-only, like sf_audio_features_create, for frames WITHOUT centring or clip padding: frame t covers
 *     samples [t hop, t hop + win_length), is multiplied by a periodic Hann window of win_length points and zero-padded at its end to
 *     n_fft points.  Same handle type, destroyed by sf_audio_features_destroy; sf_logmel_forward and sf_onset_detect refuse such a
 *     handle (SF_ERR_INVALID) and sf_logmel_examples_forward refuses a centred one.  Refused: null pointers, n_fft not a power of two
 *     in [256, 4096], win_length outside 1 .. n_fft, hop or n_mels < 1, a filter with an empty or out-of-range bin range, n_weights
 *     that is not the sum of the bin counts (SF_ERR_INVALID).
 * sf_logmel_examples_count     E = F / frames_per_example examples per clip of L samples, F = 1 + (L - win_length) / hop frames (0 for
 *     L < win_length); the remainder of the frames is dropped.  -1 for a null or centred handle, L < 1 or frames_per_example < 1.
 * sf_logmel_examples_forward   wav (B, L) -> examples: rows ((b E + e) frames_per_example + frame) n_mels + band of 4 columns, column 0 =
 *     log(mel + log_offset) (natural log), columns 1 .. 3 = 0 -- the channels-last rows sf_vggish_forward reads -- and / or
 *     mel (B, E frames_per_example, n_mels), the mel MAGNITUDE: filterbank times |X_k| (not power).  Either may be NULL (not both).
 *     Refused before any HIP call: null pointers, B, L, frames_per_example < 1, log_offset <= 0 (SF_ERR_INVALID); E = 0, B > 65535,
 *     an output of 2^31 bytes or more (SF_ERR_SHAPE).  No workspace.  A clip's rows do not depend on the rest of the batch.
 *
 * sf_vggish_create   stages[i] > 0: Conv2d(k = 3, pad = 1) to that many channels + bias + ReLU; stages[i] == 0: MaxPool2d(2, 2) (floor).
 *     Input: one channel, H x W (96 frames x 64 bands).  Then n_fc Linear layers of fc_widths[i] outputs, ReLU after each but the last,
 *     after the last only with final_relu (use_activation).  conv_w / conv_b / fc_w / fc_b: DEVICE pointers in layer order, PyTorch
 *     layouts (cout, cin, 3, 3), (cout), (out, in), (out); the first Linear's columns run (h, w, c) over the last map, as torchvggish
 *     flattens it.  Everything is packed into the engine's own memory before the call returns (on `stream`, synchronised): the
 *     caller's tensors are not referenced afterwards.  Channel counts are padded to multiples of 8 columns (zeros) in the activations;
 *     the packed weights hold zeros at those positions.  Refused before any HIP call: null pointers, counts outside 1 .. 64, channel
 *     counts outside 0 .. 8192, no convolution, widths outside 1 .. 65536 (SF_ERR_INVALID); a pool of a map below 2 x 2 (SF_ERR_SHAPE);
 *     a null weight or bias (SF_ERR_MISSING_WEIGHT).
 * sf_vggish_max_examples / sf_vggish_workspace_bytes   the largest n of one call (every activation below 2^31 bytes) and the workspace
 *     of n examples (monotone in n; -1 for a null handle or n outside 1 .. max).
 * sf_vggish_forward  examples (n H W, 4) as written by sf_logmel_examples_forward -> embeddings (n, D) dense, D = fc_widths[n_fc - 1].
 *     pool_taps: NULL, or one device pointer (or NULL) per max-pool that receives a copy of its output, rows (n, h, w) x padded
 *     channels (tests).  Convolutions and Linears run on the implicit-GEMM launcher (fp32 MFMA, fp32 accumulation), Linears as 1x1
 *     convolutions with one row per example.  Refused before any HIP call: null pointers, n < 1 (SF_ERR_INVALID), n above the maximum
 *     (SF_ERR_SHAPE), a workspace below the query (SF_ERR_WORKSPACE).
 * sf_op_maxpool2x2_cl   the engine's pool alone: x rows (n, H, W) x ld -> y rows (n, H / 2, W / 2) x ld, every column alike (padding
 *     columns stay zero), the last row / column of an odd extent dropped.  Refused: null pointers, n, ld < 1, H, W < 2 (SF_ERR_INVALID).
 * sf_op_moments   x (n, D), D <= 128 -> sum (D) and scatter (D, D) in fp64: sum[d] = sum_r x[r][d], scatter[i][j] = sum_r (x[r][i] -
 *     sum[i] / n)(x[r][j] - sum[j] / n) (two passes about the mean).  np.cov(x, rowvar=False) = scatter / (n - 1).  Fixed summation order,
 *     no atomics: identical input gives identical bits; scatter is exactly symmetric.  Refused: null pointers, n < 1 (SF_ERR_INVALID),
 *     D outside 1 .. 128 (SF_ERR_SHAPE). */
typedef struct sf_vggish sf_vggish;
int sf_audio_features_create_framed(int n_fft, int win_length, int hop, int n_mels, const int32_t *first_bin /*host*/,
                                    const int32_t *bin_count /*host*/, const float *weights /*host*/, int64_t n_weights, sf_audio_features **out);
int sf_logmel_examples_count(const sf_audio_features *h, int L, int frames_per_example);
int sf_logmel_examples_forward(sf_audio_features *h, const float *wav, int B, int L, int frames_per_example, float log_offset, float *examples,
                               float *mel, void *stream);
int sf_vggish_create(int n_stages, const int32_t *stages /*host*/, int n_fc, const int32_t *fc_widths /*host*/, int H, int W, int final_relu,
                     const void *const *conv_w, const void *const *conv_b, const void *const *fc_w, const void *const *fc_b, void *stream,
                     sf_vggish **out);
void sf_vggish_destroy(sf_vggish *h);
int sf_vggish_max_examples(const sf_vggish *h);
int64_t sf_vggish_workspace_bytes(const sf_vggish *h, int n);
int sf_vggish_forward(sf_vggish *h, const float *examples, int n, float *embeddings, float *const *pool_taps, void *ws, int64_t ws_bytes,
                      void *stream);
int sf_op_maxpool2x2_cl(const float *x, int64_t n, int H, int W, int ld, float *y, void *stream);
int sf_op_moments(const float *x, int64_t n, int D, double *sum, double *scatter, void *stream);

/* ------------------------------------------------------------------------------------------
 * CLAP audio embedder (syncfusion_amd/clap.py)
 *   replaces: laion_clap.CLAP_Module(enable_fusion=False, amodel='HTSAT-tiny').get_audio_embedding_from_data(x, use_tensor=True)
 *   (exp/model/diffusion.yaml:45-48, main/module_diffusion.py:64-67): the log-mel "image", a Swin transformer and a two-layer projection.
 *   The mel power itself comes from sf_logmel_forward.  All tensors fp32, contiguous, on the device; fp32 MFMA GEMMs, fp32 accumulation.
 *
 * sf_op_logmel_image   mel_power (B, n_mels, T) -> image (B, S, S), S = n_mels ratio:  v[f][t] = 10 log10(max(P, amin)) scale[f] + shift[f]
 *     (one fma; the BatchNorm of the mel bins folded by the caller), stretched along time to S ratio frames when T is smaller (bicubic,
 *     PyTorch's kernel: A = -0.75, align_corners, clamped borders; T == S ratio copies), folded: image[r n_mels + f][t'] = v[f][r S + t'].
 *     A stretch over equal values (the zero-padded tail of a short clip: P <= amin) is exact: fma(fp32(10 log10 amin), scale, shift).
 *     Refused before any HIP call: null pointers, B, n_mels, ratio < 1, T < 2, amin <= 0 (SF_ERR_INVALID); S > 4096, S ratio > 32768,
 *     T > S ratio (nothing is shrunk), a tensor of 2^31 elements or more (SF_ERR_SHAPE).
 * sf_op_window_attention   qkv (B H W, 3 C) rows in raster order, columns [q | k | v] each (heads, D) -> out (B H W, C): attention inside
 *     8 x 8 windows of the map rolled by (-shift, -shift), softmax(q k^T D^-1/2 + bias_table[(dy + 7) 15 + dx + 7][head] + mask) v with
 *     (dy, dx) = query - key inside the window; shifted windows add mask_value between tokens of different regions (region 3 hr + wr,
 *     hr / wr in {0, 1, 2} for a rolled-frame coordinate < H - 8, < H - 4, else).  Partition, roll and their inverses are index arithmetic:
 *     nothing is copied and no mask tensor is read.  bias_table (225, heads).  One wave per (clip, window, head), fixed-order sums: a
 *     clip's rows do not depend on the batch.  Refused before any HIP call: null pointers, arguments < 1 (SF_ERR_INVALID); heads that do
 *     not divide C, H or W no multiple of 8, a shift with H or W == 8, 2^31 elements or more (SF_ERR_SHAPE); a head dim that is no multiple
 *     of 4 or above 32, a shift other than 0 or 4 (SF_ERR_UNSUPPORTED).
 * sf_clap_audio_create   the network behind the image.  Named weights (DEVICE pointers, copied before the call returns), with every
 *     LayerNorm affine already folded into the weights that follow it (clap.py does that in fp64):
 *       patch.w (E, 16)  patch.b  patch.g  patch.beta                         Conv2d(1, E, 4, 4) + LayerNorm(E)
 *       s{i}.b{j}.qkv.w (3 C, C)  .qkv.b   .rpb (225, heads)  .proj.w (C, C)  .proj.b
 *       s{i}.b{j}.fc1.w (r C, C)  .fc1.b   .fc2.w (C, r C)    .fc2.b          C = E 2^i, r = mlp_ratio
 *       s{i}.merge.w (2 C, 4 C)   s{i}.merge.b                                 every stage but the last
 *       head.g  head.beta  proj0.w (J, C_last)  proj0.b  proj2.w (J, J)  proj2.b
 *     block j of a stage is shifted by window / 2 for odd j unless the stage's map is one window.  Refused before any HIP call: null
 *     pointers, counts out of range (SF_ERR_INVALID); a window other than 8, a head dim that is no multiple of 4 or above 32
 *     (SF_ERR_UNSUPPORTED); spec_size no multiple of 32 2^(stages - 1), embed_dim no multiple of 32 in 32 .. 256, a final width or
 *     joint_dim above 1024, more than 256 final tokens (SF_ERR_SHAPE); a missing or mis-sized weight (SF_ERR_MISSING_WEIGHT, named).
 * sf_clap_audio_max_batch / sf_clap_audio_workspace_bytes   the largest B of one call and the workspace of B clips (-1 outside 1 .. max).
 * sf_clap_audio_forward   image (B, S, S) -> embedding (B, joint_dim).  taps: NULL, or n_stages + 1 device pointers (each may be NULL)
 *     that receive the token matrix behind the patch embed and behind every stage (after its PatchMerging), for tests.  Refused before
 *     any HIP call: null pointers, B < 1 (SF_ERR_INVALID), B above the maximum (SF_ERR_SHAPE), a workspace below the query
 *     (SF_ERR_WORKSPACE), a GEMM shape no kernel takes (SF_ERR_UNSUPPORTED).  Nothing is allocated and nothing synchronises.
 * sf_clap_audio_describe   HOST-only: one line per GEMM of the network at batch B with the kernel family the dispatcher gives it. */
#define SF_CLAP_MAX_STAGES 8
typedef struct {
  int32_t spec_size, embed_dim, n_stages;
  int32_t depths[SF_CLAP_MAX_STAGES], heads[SF_CLAP_MAX_STAGES];
  int32_t window, mlp_ratio, joint_dim;
  float ln_eps, mask_value;
  int32_t projection_relu, normalize;
} sf_clap_audio_config;
typedef struct sf_clap_audio sf_clap_audio;
int sf_op_logmel_image(const float *mel_power, int B, int n_mels, int T, int ratio, const float *scale, const float *shift, float amin, float *image,
                       void *stream);
int sf_op_window_attention(const float *qkv, int B, int H, int W, int C, int heads, int shift, const float *bias_table, float mask_value, float *out,
                           void *stream);
int sf_clap_audio_create(const sf_clap_audio_config *cfg, const sf_tensor *weights, int n_weights, void *stream, sf_clap_audio **out);
void sf_clap_audio_destroy(sf_clap_audio *h);
int sf_clap_audio_max_batch(const sf_clap_audio *h);
int64_t sf_clap_audio_workspace_bytes(const sf_clap_audio *h, int B);
int sf_clap_audio_forward(sf_clap_audio *h, const float *image, int B, float *embedding, float *const *taps, void *ws, int64_t ws_bytes, void *stream);
int sf_clap_audio_describe(const sf_clap_audio_config *cfg, int B, char *text /*host*/, int64_t capacity);

/* ------------------------------------------------------------------------------------------
 * CLAP text embedder (syncfusion_amd/clap_text.py)
 *   replaces: laion_clap.CLAP_Module(...).get_text_embedding(text, use_tensor=True)
 *   (main/module_diffusion.py:69-71; the text-conditioned generation of exp/evaluate_gh_gen_text.yaml:29, cond_text: True): RoBERTa
 *   (post-LN encoder, key-padding mask, pooler) and a two-layer projection on token ids.  Tokenisation is the caller's (host).  ids and
 *   mask are int32 (B, S), contiguous, on the device; everything else fp32; fp32 MFMA GEMMs, fp32 accumulation.
 *
 * sf_op_text_embed   ids (B, S) -> out (B S, C): LayerNorm_C(word[id] + pos[p] + type[:]; gamma, beta), p = pad_id + (the number of
 *     ids != pad_id in the row up to and including this column) for a real token and pad_id for a pad.  One wave per row, two-pass
 *     statistics.  id and p are clamped into their tables (vocab, n_pos rows): memory safety only.  Refused before any HIP call: null
 *     pointers, B, S, vocab, n_pos < 1, eps <= 0 (SF_ERR_INVALID); C no multiple of 64 or above 1024 (SF_ERR_UNSUPPORTED); 2^31 elements
 *     or more (SF_ERR_SHAPE).
 * sf_op_layernorm_affine   y = LN_C(x) gamma + beta on `rows` rows, one wave per row, two passes.  Refusals as above.
 * sf_op_masked_attention   qkv (B S, 3 C) rows, columns [q | k | v] each (heads, 64), C = 64 heads; mask (B, S), non-zero = a real
 *     token -> out (B S, C): softmax(q k^T / 8) v over the keys the mask admits.  A masked key carries weight exactly 0 and its K and V
 *     rows never enter the arithmetic (they may hold anything); masked QUERY rows are computed like any other; a text whose mask admits no
 *     key gives zeros.  One workgroup per (text, head), fixed-order sums: a text's rows do not depend on the batch.  Refused before any
 *     HIP call: null pointers, B, S, heads < 1 (SF_ERR_INVALID); S > 128 (SF_ERR_UNSUPPORTED); 2^31 elements or more (SF_ERR_SHAPE).
 * sf_clap_text_create   the network.  Named weights (DEVICE pointers, copied before the call returns):
 *       emb.word (vocab, C)  emb.pos (max_positions, C)  emb.type (C)  emb.g  emb.beta
 *       l{i}.qkv.w (3 C, C)  .qkv.b (3 C)          query | key | value concatenated by the caller
 *       l{i}.ao.w (C, C)  .ao.b  .ln1.g  .ln1.beta  the attention output and the LayerNorm behind its residual add
 *       l{i}.fc1.w (I, C)  .fc1.b  .fc2.w (C, I)  .fc2.b  .ln2.g  .ln2.beta
 *       pool.w (C, C)  pool.b                       pooling == 0 only
 *       proj0.w (J, C)  proj0.b  proj2.w (J, J)  proj2.b
 *     Refused before any HIP call: null pointers, counts out of range (SF_ERR_INVALID); hidden != 64 heads, hidden above 1024,
 *     max_length above 128 (SF_ERR_UNSUPPORTED); max_length + pad_id + 1 above max_positions, joint_dim above 1024 (SF_ERR_SHAPE); a
 *     missing or mis-sized weight (SF_ERR_MISSING_WEIGHT, named).
 * sf_clap_text_workspace_bytes   the workspace of B texts of S columns (-1 out of range).
 * sf_clap_text_forward   ids, mask (B, S) -> embedding (B, joint_dim).  taps: NULL, or layers + 2 device pointers (each may be NULL) that
 *     receive the (B S, C) hidden state behind the embeddings and behind every layer, and the (B, C) pooled rows, for tests.  Refused
 *     before any HIP call: null pointers, B or S < 1 (SF_ERR_INVALID); S above 128 (SF_ERR_UNSUPPORTED); S above max_length or the
 *     position table, too many rows (SF_ERR_SHAPE); a workspace below the query (SF_ERR_WORKSPACE); a GEMM shape no kernel takes
 *     (SF_ERR_UNSUPPORTED).  Nothing is allocated and nothing synchronises.
 * sf_clap_text_describe   HOST-only: one line per GEMM of a layer at (B, S) with the kernel family the dispatcher gives it. */
typedef struct {
  int32_t vocab_size, hidden, layers, heads, intermediate, max_positions, pad_id, max_length, joint_dim;
  float ln_eps;
  int32_t pooling; /* 0: tanh(Linear) of token 0 (pooler_output); 1: token 0 as it is */
  int32_t projection_relu, normalize;
} sf_clap_text_config;
typedef struct sf_clap_text sf_clap_text;
int sf_op_text_embed(const int32_t *ids, int B, int S, int C, int vocab, int n_pos, int pad_id, const float *word, const float *pos, const float *type,
                     const float *gamma, const float *beta, float eps, float *out, void *stream);
int sf_op_layernorm_affine(const float *x, int64_t rows, int C, const float *gamma, const float *beta, float eps, float *y, void *stream);
int sf_op_masked_attention(const float *qkv, const int32_t *mask, int B, int S, int heads, float *out, void *stream);
int sf_clap_text_create(const sf_clap_text_config *cfg, const sf_tensor *weights, int n_weights, void *stream, sf_clap_text **out);
void sf_clap_text_destroy(sf_clap_text *h);
int64_t sf_clap_text_workspace_bytes(const sf_clap_text *h, int B, int S);
int sf_clap_text_forward(sf_clap_text *h, const int32_t *ids, const int32_t *mask, int B, int S, float *embedding, float *const *taps, void *ws,
                         int64_t ws_bytes, void *stream);
int sf_clap_text_describe(const sf_clap_text_config *cfg, int B, int S, char *text /*host*/, int64_t capacity);

/* ------------------------------------------------------------------------------------------
 * JPEG frames on the device (syncfusion_amd/jpeg.py)
 *   replaces: PIL.Image.open(path).convert("RGB") of main/dataset_onset.py:155 for the files script/gh_preprocess_videos.py:122-123
 *   writes (baseline sequential, one interleaved scan).  The output is libjpeg's default decode, byte for byte: Huffman decode, the
 *   integer "islow" IDCT, fancy h2v1 / h2v2 chroma upsampling, integer YCbCr -> RGB.  Exact for streams an encoder writes (IDCT
 *   outputs inside +-512 around the level shift); beyond that the result is clamped and unspecified.
 *
 * sf_jpeg_parse   HOST only (no HIP call).  bytes: the N files back to back; offsets: N + 1 positions, file i is
 *     bytes[offsets[i] .. offsets[i + 1]).  Fills one descriptor per file and, when segs_out is given, the segment table: a file
 *     without a restart interval is one segment, otherwise every restart interval is one (DC prediction restarts there, so segments
 *     decode independently); the count per file follows from its header, ceil(MCUs / interval), the RSTn markers are found by a byte
 *     scan, and the last segment of a file runs to the end of its entropy-coded data.  desc.status says what the device may do with
 *     the file: SF_JPEG_OK; SF_JPEG_UNSUPPORTED (a valid stream outside the kernels' coverage, desc.reason names why: progressive,
 *     arithmetic, lossless or 12-bit frames, 2 or 4 components, several scans, Huffman table ids above 1, sampling other than luma
 *     1x1 / 2x1 / 2x2 over 1x1 chroma, an Adobe marker with transform != 1, component ids R G B) or SF_JPEG_MALFORMED (desc.reason
 *     names the defect).  Unsupported and malformed files have no segments and take no workspace.  coef_offset / plane_offset are
 *     the file's places in the workspace of ONE decode call over exactly these N descriptors.  *n_segs_out: the segment count.
 *     Returns SF_ERR_WORKSPACE when seg_capacity is below it (descriptors are complete, no segment is written), SF_ERR_INVALID
 *     when a file is malformed (the first one is named in the message; all descriptors are complete), SF_OK otherwise.  No byte
 *     outside bytes[offsets[0] .. offsets[N]) is read, whatever the files hold.
 * sf_jpeg_decode_workspace_bytes   HOST only: the workspace of one decode call over these descriptors (-1: bad argument) --
 *     int16 coefficient blocks in natural order, each component padded to whole MCUs, then the uint8 component planes of the same
 *     padded extent.
 * sf_jpeg_decode   bytes_dev: the same bytes on the device (n_bytes = offsets[N], offsets[0] = 0); desc_host / desc_dev: the
 *     descriptors as the parser filled them, on the host (checked before any launch: sizes, sampling, table selectors, offsets and
 *     ranges) and the same bytes on the device; segs_dev: the segment table on the device.  Every SF_JPEG_OK file must be
 *     width x height = W x H.  out: (N, H, W, 3) uint8; the slots of files that are not SF_JPEG_OK are written as zeros.
 *     status_dev: N int32, zeroed by the call, then the first problem the entropy decoder met per file (SF_JPEG_ST_*); a flagged file
 *     leaves the others alone, its own pixels are unspecified.  The call zeroes what it needs of the workspace.  One wave per
 *     segment; no read outside bytes_dev[0 .. n_bytes), no write outside a wave's own blocks, for any bytes.  Nothing synchronises.
 * ---------------------------------------------------------------------------------------- */
enum { SF_JPEG_OK = 0, SF_JPEG_UNSUPPORTED = 1, SF_JPEG_MALFORMED = 2 };
enum {
  SF_JPEG_ST_OUT_OF_BITS = 1,     /* the segment ended (or a marker came) before its MCUs were complete */
  SF_JPEG_ST_BAD_CODE = 2,        /* a bit pattern no Huffman code of the table matches, or a DC category above 15 */
  SF_JPEG_ST_INDEX_OVERFLOW = 3,  /* a run past coefficient 63 */
  SF_JPEG_ST_TRAILING_BYTES = 4,  /* bytes left in the segment behind its last MCU */
  SF_JPEG_ST_BAD_SEGMENT = 5      /* a segment table entry outside its file or its MCUs */
};
typedef struct {
  int32_t status;              /* SF_JPEG_OK / SF_JPEG_UNSUPPORTED / SF_JPEG_MALFORMED */
  int32_t width, height, ncomp;
  int32_t h[3], v[3];          /* sampling factors (1 x 1 for a one-component file, whatever its header says) */
  int32_t tq[3], td[3], ta[3]; /* quantisation / DC / AC table selectors */
  int32_t restart_interval;    /* MCUs, 0: none */
  int32_t mcus_x, mcus_y;
  int32_t quant_precision[4];  /* -1: absent, 0: 8-bit, 1: 16-bit */
  int32_t huff_present;        /* bit 0, 1: DC tables 0, 1; bit 2, 3: AC tables 0, 1 */
  int32_t seg_count;
  int64_t seg_begin;           /* first entry of this file in the segment table */
  int64_t data_begin, data_end;/* entropy-coded bytes, positions in the concatenated buffer */
  int64_t coef_offset;         /* int16 elements from the start of the workspace */
  int64_t plane_offset;        /* bytes from the start of the plane area of the workspace */
  int64_t reserved;            /* (keeps quant, and an array of descriptors, on 16-byte boundaries) */
  uint16_t quant[4][64];       /* natural (de-zigzagged) order */
  uint8_t huff_counts[4][16];  /* [0], [1]: DC tables 0, 1; [2], [3]: AC tables 0, 1 */
  uint8_t huff_values[4][256];
  char reason[64];
} sf_jpeg_desc;
typedef struct {
  int32_t image, first_mcu, mcu_count, reserved;
  int64_t byte_begin, byte_end; /* positions in the concatenated buffer; the RSTn marker behind the segment is outside */
} sf_jpeg_segment;
int sf_jpeg_parse(const uint8_t *bytes /*host*/, const int64_t *offsets /*host*/, int N, sf_jpeg_desc *desc_out /*host*/,
                  sf_jpeg_segment *segs_out /*host*/, int64_t seg_capacity, int64_t *n_segs_out /*host*/);
int64_t sf_jpeg_decode_workspace_bytes(const sf_jpeg_desc *desc /*host*/, int N);
int sf_jpeg_decode(const uint8_t *bytes_dev, int64_t n_bytes, const sf_jpeg_desc *desc_host, const sf_jpeg_desc *desc_dev,
                   const sf_jpeg_segment *segs_dev, int64_t n_segs, int N, int H, int W, uint8_t *out, int32_t *status_dev, void *ws,
                   int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SYNCFUSION_AMD_H */
