/*
 * si_hip.h -- C ABI of libsi_hip.so: the MI355X (gfx950) implementation of the I_ea predict hot path.
 *
 * The reference (Fireflies-17/Speech-Inpainting) has no FFI; its seam is three Python module calls.
 * Each entry point below replaces one of them (paths relative to /root/reference):
 *
 *   si_hubert_forward    <- CustomModel.forward                I_ea/model.py:80-89 (called at I_ea/predict.py:163)
 *                           + the zero-mask + processor normalise in front of it (I_ea/predict.py:132-141)
 *   si_codebook_splice   <- frame gather + LossFunction.cos_sim arg-max + centroid splice
 *                           I_ea/predict.py:164-168,171,184-187 ; I_ea/loss_fn.py:44-47
 *   si_codebook_metrics  <- LossFunction.cos_sim loss + cos_sim_target_labels (row f-4)
 *                           I_ea/loss_fn.py:29-62 ; I_ea/predict.py:171-173
 *   si_mel_metrics       <- Metrics.avg_cosine_sim / avg_d2_dist / rmse (row f-4)   I_ea/metrics.py:38-62
 *   si_sisdr             <- Metrics.sisdr (row f-4)                                 I_ea/metrics.py:127-142
 *   si_unit_frontend     <- CodeGenerator.forward's embedding / _upsample / concat front (row f-2)   I_da/src/model.py:79-119,148-189
 *   si_f0_encoder_forward <- FoVQVAE.encoder(fo) inside CodeGenerator.forward (row f-2)   I_da/src/model.py:160-163 ; I_da/src/modules/jukebox.py:11-116,200-262
 *   si_hubert_extract_features <- HubertFeatureReader.get_feats (row f-2)   I_da/src/hubert_feature_reader.py:44-67 (called at
 *                           I_da/scripts/inpainting.py:195-198) + the corruption `(y + 1e-6) * mask` in front of it (:186-192)
 *   si_code_splice       <- the unit splice (row f-2)                        I_da/scripts/inpainting.py:209-214
 *   si_kmeans_assign     <- kmeans_model.predict(feats) (row f-2)   I_da/scripts/inpainting.py:204-205 ;
 *                           ApplyKmeans.__call__                    I_ea/dataset/km_label.py:20-24
 *   si_resample_poly     <- librosa.load(..., sr=22050 / 16000) resampling (row f-3)   I_ea/predict.py:79-80
 *   si_mel_frontend      <- 22.05 kHz masking + normalize*0.95 + get_mel
 *                           I_ea/predict.py:99-106 ; I_ea/dataset/mel_dump.py:40-98
 *   si_hifigan_forward   <- extend_mel + Generator.forward     I_ea/hifi_gan/inference_modified.py:16-19 ;
 *                           I_ea/hifi_gan/models.py:107-123 (called at I_ea/predict.py:189,203)
 *   si_wave_peak / si_gather_windows / si_patch_compose  <- the whole-clip generator call and int16 write-out, for a recording
 *                           that keeps its own samples outside the gaps      I_ea/predict.py:104,189,203-207
 *   si_cut_clips / si_patch_regions  <- the same lines for a recording LONGER than one clip: the slices that turn one file into the
 *                           clips the script takes one per run, and the write-out of many clips' gaps into the one long file
 *                                                                             I_ea/predict.py:79-80,104,203-207
 *   si_quiet_runs        <- nothing the reference computes: it has no detection.  The call supplies the `mask:` values
 *                           (start_pos_in_sec, end_pos_in_sec) that a user of the script types by hand      I_ea/predict.py:85-90
 *   si_dead_runs         <- nothing the reference computes either: si_quiet_runs for dropouts that are not digital silence -- held
 *                           samples, mutes relative to the file's peak.  It has no detection                I_ea/predict.py:85-90
 *   si_level_runs        <- nothing the reference computes either: si_dead_runs for a dropout that is a NOISE FLOOR (dither, a
 *                           concealer's comfort noise), found by windowed RMS level.  It has no detection     I_ea/predict.py:85-90
 *   si_burst_runs        <- nothing the reference computes either: the detector for damage that is LOUDER than the speech -- a block
 *                           of corrupted PCM (random data, swapped or misaligned bytes), found by the windowed level of the second
 *                           difference.  It has no detection                                          I_ea/predict.py:85-90
 *   si_invalid_runs      <- nothing the reference computes either: the detector for a FLOAT file whose damage is the sample values
 *                           themselves -- NaN, +-inf, absurd magnitudes -- which no other detector sees.  It has no detection
 *                                                                             I_ea/predict.py:85-90
 *   si_impulse_runs, si_impulse_residual  <- nothing the reference computes either: the detector for clicks and pops of one to a few
 *                           IN-RANGE samples, by a short-time AR prediction error against that of its own neighbourhood, and that
 *                           prediction error itself.  It has no detection                              I_ea/predict.py:85-90
 *   si_cut_rate_valid / si_cut_pair_valid / si_cut_clips_valid  <- nothing the reference computes: si_cut_rate[_ch], si_cut_pair[_ch] and
 *                           si_cut_clips with such a sample entering as +0.0, so that one NaN costs its gap and not its whole context.
 *                           The script's loads (I_ea/predict.py:79-80) pass every value on; its mask is typed by hand (:85-90)
 *   si_mend_runs         <- nothing the reference computes: runs of at most 64 samples filled in place from their own neighbourhood
 *                           by least-squares AR interpolation, instead of a generated 20 ms frame each.  It has no detection
 *                                                                             I_ea/predict.py:85-90
 *   si_patch_rate        <- the same write-out for a file at ANY sample rate, which the script resamples on the way in and never
 *                           brings back                                       I_ea/predict.py:79-80,203-207
 *   si_cut_rate          <- that resampling on the way in, for the context clips alone instead of the whole file (with si_cut_clips'
 *                           slicing)                                          I_ea/predict.py:79-80
 *   si_quiet_runs_ch / si_cut_rate_ch / si_patch_rate_ch  <- the three above on an interleaved multi-channel file, channel by channel,
 *                           where the script mixes its input down to one channel on load      I_ea/predict.py:79
 *   si_cut_pair / si_cut_pair_ch  <- the script's TWO loads of the one file, at 22.05 kHz for the mel and at 16 kHz for HuBERT, each
 *                           straight from the file's samples, for the context clips alone and in one launch    I_ea/predict.py:79-80
 *   si_load_weights      <- model.load_state_dict / generator.load_state_dict + remove_weight_norm + ApplyKmeans
 *                           I_ea/predict.py:117-122,149 ; I_ea/hifi_gan/models.py:125-132 ; I_ea/dataset/km_label.py:12-24
 *
 * Conventions: plain C types only; every function returns 0 on success and a negative SI_E* code on
 * failure (message via si_last_error); no exceptions cross the boundary.  A context is bound to one device,
 * is not thread-safe and enqueues all work on the caller's HIP stream: every kernel, memset and copy of a call that takes a
 * si_stream_t is ordered on that stream and on no other (a context is driven from one stream at a time).  A call does not wait
 * for the stream, with three exceptions (tests/test_gpu_side_stream.py holds every entry point to this behind a delayed stream):
 *   - growth of library-owned scratch: the call of si_kmeans_assign or of a detector (si_quiet_runs .. si_impulse_runs) whose K or
 *     n no longer fits the scratch the context holds synchronises the stream before it frees the old block; the next call of
 *     that size does not;
 *   - reuse of a pinned slot: the ragged passes (sample_len / mel_len as a HOST array) upload their length table through 4 pinned
 *     slots in turn; the fifth such call waits until the copy that the first one queued has left its slot;
 *   - calls documented to wait or to return host values: si_profile_stop, si_weights_check, si_load_weights, si_destroy, and the
 *     first mel front-end call of a context, which uploads its tables.
 * All data pointers are DEVICE pointers owned by the caller unless the parameter says "host".
 * Activations are fp32.  Layouts are the reference's: wave (B, N); feats (B, T, D); mel (B, D, Tm)
 * channels-first; waveform (B, Tm' * hop).
 */
#ifndef SI_HIP_H
#define SI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SI_ABI_VERSION 3

enum {
    SI_OK = 0,
    SI_EINVAL = -1,      /* bad argument / unsupported shape */
    SI_ENOMEM = -2,      /* workspace too small or device allocation failed */
    SI_EHIP = -3,        /* a HIP runtime call failed */
    SI_ESTATE = -4,      /* call order violated (e.g. forward before weights) */
    SI_EWEIGHTS = -5     /* missing / mis-shaped tensor in the checkpoint index */
};

/* arithmetic of the contraction (accumulation is always fp32) */
enum {
    SI_MATH_F32 = 0,     /* v_mfma_f32_32x32x2_f32: exact fp32 fma chain */
    SI_MATH_BF16 = 1,    /* v_mfma_f32_32x32x16_bf16, operands rounded to bf16 */
    SI_MATH_BF16X3 = 2,  /* hi/lo split bf16, 3 MFMAs per product: ~2^-16 relative operand error */
    SI_MATH_F16 = 3      /* v_mfma_f32_32x32x16_f16, operands rounded to fp16 (saturating): 2^-12 relative operand error */
};

#define SI_MAX_CONV 8
#define SI_MAX_UPS 8
#define SI_MAX_RB 4
#define SI_MAX_DIL 4

typedef struct si_ctx si_ctx;
typedef void* si_stream_t;      /* hipStream_t */

/* Architecture + arithmetic of one model pair.  HuBERT fields follow the HuggingFace config.json
 * (I_ea/dataset/config.json:62-124), vocoder fields the HiFi-GAN json (I_ea/hifi_gan/config_v1.json). */
typedef struct si_model_desc {
    int32_t struct_size;            /* = sizeof(si_model_desc), ABI check */
    /* encoder */
    int32_t hidden_size, num_layers, num_heads, intermediate_size;
    int32_t num_conv;
    int32_t conv_dim[SI_MAX_CONV], conv_kernel[SI_MAX_CONV], conv_stride[SI_MAX_CONV];
    int32_t conv_bias;              /* 0 base / 1 large */
    int32_t feat_norm_layer;        /* 0 = "group" (GroupNorm on conv0 only), 1 = "layer" (LayerNorm on every conv) */
    int32_t stable_layer_norm;      /* 0 post-LN (base), 1 pre-LN (large) */
    int32_t pos_conv_kernel, pos_conv_groups;
    int32_t feat_proj_layer_norm;
    float   layer_norm_eps;
    int32_t codebook_dim;           /* final_layers Linear(H -> codebook_dim), 80 */
    int32_t num_clusters;           /* K centroids, 100 or 500 */
    /* vocoder */
    int32_t num_mels;
    int32_t num_ups;
    int32_t up_rates[SI_MAX_UPS], up_kernels[SI_MAX_UPS];
    int32_t up_initial_channel;
    int32_t num_rb;                 /* resblocks per stage (3) */
    int32_t rb_kernels[SI_MAX_RB];
    int32_t num_dil;                /* dilations per resblock (3) */
    int32_t rb_dilations[SI_MAX_RB][SI_MAX_DIL];
    /* arithmetic */
    int32_t encoder_math;           /* SI_MATH_* for the encoder GEMMs/convs (attention + head stay fp32) */
    int32_t vocoder_math;           /* SI_MATH_* for the generator convs */
    int32_t vocoder_chunk;          /* clips per vocoder pass (0 = library default; sized to the Infinity Cache) */
    int32_t resblock_type;          /* 1 (or 0): ResBlock1 -- num_dil (conv_dilated, conv) pairs per block (config_v1 / v2, I_da);
                                       2: ResBlock2 -- num_dil single dilated convs per block, x = x + conv(lrelu(x))
                                       (I_ea/hifi_gan/models.py:52-73, selected at :89 by config_v3.json:2) */
} si_model_desc;

int si_version(void);

/* Create a context on `device_id`.  No device memory is allocated until weights are loaded. */
int si_create(si_ctx** out, int device_id, const si_model_desc* desc);
void si_destroy(si_ctx* ctx);

/* Last error text of this context (or of si_create when ctx == NULL).  Never NULL. */
const char* si_last_error(const si_ctx* ctx);

/* Load a checkpoint.  `host_blob` (host memory) holds fp32 tensors; `index` is text, one tensor per line:
 *     <name> <byte_offset> <ndim> <d0> ... <d(ndim-1)>
 * Names are the reference's state-dict keys: "base_model.<hf key>", "final_layers.{0,1}.{weight,bias}",
 * "generator.<Generator key>" (folded ".weight" or weight-norm ".weight_g"/".weight_v"; ResBlock1 blocks hold
 * "convs1.<n>" / "convs2.<n>", ResBlock2 blocks "convs.<n>"), "codebook" (K, D).
 * Weight-norm is folded here (dim 0 for the generator, dim 2 for the positional conv, in either the
 * "parametrizations.weight.original{0,1}" or the legacy "weight_g/weight_v" spelling).  The tensors are
 * re-laid-out for the kernels into one packed device blob owned by the context. */
int si_load_weights(si_ctx* ctx, const void* host_blob, size_t nbytes, const char* index);

/* Multi-GPU: ranks that do not read the checkpoint allocate the (identically laid out) packed blob with
 * si_alloc_weights and receive its bytes by an RCCL broadcast into si_weights_device_ptr. */
int si_alloc_weights(si_ctx* ctx);
int si_weights_device_ptr(si_ctx* ctx, void** ptr, size_t* nbytes);
/* The blob starts with a fingerprint of the layout it was packed for (model desc + the context's arithmetic-path options).
 * si_weights_check compares it with THIS context's plan (one small synchronous device-to-host copy): SI_EWEIGHTS when the
 * source rank planned a different layout or the bytes have not arrived.  Call it after the broadcast; the forwards also
 * run it once before the first use of a blob that came from si_alloc_weights. */
int si_weights_check(si_ctx* ctx);

/* The plan and the packer WITHOUT a device (csrc/weights_host.cpp: plain host code; both calls work with zero visible devices and
 * read the SI_VOC_OPREADY / SI_VOC_RES16 options from the environment exactly as si_create does).
 * si_plan_weights: the descriptor check of si_create (SI_EINVAL with a message that names the field, through si_last_error(NULL);
 * the bounds are listed in csrc/weights_host.h) and the byte size of the packed blob.
 * si_pack_weights_host: the bytes si_load_weights copies to the device -- it calls the same function -- header included, into
 * out[0 .. *needed).  *needed (may be NULL) is set as soon as the desc is accepted.  Order of the checks: desc (SI_EINVAL), capacity
 * (SI_ENOMEM when out is NULL or capacity < *needed), index and tensors (SI_EWEIGHTS, naming the tensor or the index line), host
 * memory for the image (SI_ENOMEM).  Every required tensor is looked up and its shape compared BEFORE the image is allocated.
 * Refused with SI_EWEIGHTS besides missing / mis-shaped tensors: an empty or malformed index, a name listed twice, dims that
 * overflow, an offset that is negative, misaligned or past the blob, a weight-norm row of zero norm, a non-finite value in anything
 * that is packed (a FINITE weight beyond +-65504 is clamped silently in the fp16 mode).  On failure nothing is written to `out`;
 * the message goes to err[0 .. errcap) (may be NULL).  No C++ exception leaves either call. */
int si_plan_weights(const si_model_desc* desc, size_t* total_bytes);
int si_pack_weights_host(const si_model_desc* desc, const void* host_blob, size_t nbytes, const char* index, void* out, size_t capacity,
                         size_t* needed, char* err, size_t errcap);

/* Workspace (device scratch) needed for a batch of B clips of N samples and Tm mel frames. */
int si_workspace_bytes(si_ctx* ctx, int B, int N, int Tm, size_t* out);

/* Encoder: 16 kHz clips -> (B, T, codebook_dim).  Samples [mask_start[b], mask_start[b]+mask_len[b])
 * are zeroed, then (normalize != 0) each clip is normalised to zero mean / unit variance (eps 1e-7); both are
 * fused into the load of the first conv.  normalize = 0 takes `wav` as the processor's input_values
 * (already normalised), which is what CustomModel.forward receives in the reference.
 * mask_start / mask_len: device int32 (B), may be NULL (no mask).
 * T = the conv-stack length of N (modeling_hubert.py:664-677). */
int si_hubert_forward(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len, int normalize,
                      int B, int N, float* out_feats, void* workspace, size_t workspace_bytes, si_stream_t stream);

/* The same for RIGHT-PADDED batches -- `CustomModel.forward(input_values, attention_mask)` with a mask that is not all ones
 * (I_ea/model.py:80-85 -> modeling_hubert.py:921-932): valid_len (device int32 (B), samples) marks the real part of each clip.
 * normalize != 0 reproduces the processor's padded normalisation (statistics over the real samples, padding = 0 after it);
 * the feature extractor and the projection run over the whole padded input (HuBERT-base's GroupNorm therefore sees the
 * padding, exactly as the reference's does), the padded frames of the projected states are zeroed and excluded as
 * attention keys (:428-437, frame lengths by :664-689).  Outputs are defined on ALL T frames, as in the reference.
 * valid_len = NULL is si_hubert_forward. */
int si_hubert_forward_padded(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len,
                             const int32_t* valid_len, int normalize, int B, int N, float* out_feats, void* workspace,
                             size_t workspace_bytes, si_stream_t stream);

/* RAGGED batches (BASELINE configs[4]: clips of different lengths, I_ea/config.yaml:11 "10.1 s", I_ea/mask_pos_len.py:28-35): B clips
 * of DIFFERENT lengths in one call, each clip's result EQUAL to that clip run alone -- the reference's script handles one file of
 * any length per invocation (I_ea/predict.py:76-207) -- and not the padded semantics of si_hubert_forward_padded (whose GroupNorm
 * sees the padding, as HuggingFace's does).  wav (B, N): clip b occupies the first sample_len[b] samples of its row, the rest is
 * ignored (held for every ragged entry point, with NaN and 1e30 there: tests/test_gpu_scratch.py).
 * sample_len: HOST int32 (B) (launch grids depend on it).  mask_start / mask_len as si_hubert_forward.
 * Per clip: the processor's statistics over its own samples, conv0's GroupNorm statistics over its own conv rows, every strided
 * convolution stops at its own length (modeling_hubert.py:664-677), the transformer runs on the packed rows of all clips (the
 * positional conv's zero padding begins at the clip's own last frame, attention sees its own frames only).
 * out_feats (B, T, codebook_dim) with T = si_num_frames(N): rows >= si_num_frames(sample_len[b]) of clip b are zero. */
int si_hubert_forward_varlen(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len, const int32_t* sample_len,
                             int normalize, int B, int N, float* out_feats, void* workspace, size_t workspace_bytes, si_stream_t stream);

/* I_da's encoder call: `HubertFeatureReader.get_feats` (I_da/src/hubert_feature_reader.py:44-67) =
 * optional `F.layer_norm(x, x.shape)` over the whole clip (:53-54, when the checkpoint's task.cfg.normalize is set) followed by
 * fairseq's `model.extract_features(source, padding_mask=None, mask=False, output_layer=L)` (:60-65): the feature extractor,
 * LayerNorm + projection, positional conv, then transformer layers 0..L-1 ONLY; the output is layer L-1's output (B, T, H) --
 * in the pre-LN ("layer_norm_first") flavour the residual stream WITHOUT the encoder's final LayerNorm, which fairseq
 * applies only when no layer is requested.  No head, no codebook.
 * fairseq is not in the build image and the reference pins no version of it; the arithmetic is the HuBERT architecture
 * this library already implements for I_ea (the transformers port of the same checkpoints), so the entry is pinned
 * against `HubertModel(..., output_hidden_states=True).hidden_states[L]` (tests/golden/hidden_layers.npz).
 * mask_start / mask_len (device int32 (B), samples, or NULL) and pre_mask_add (device fp64 (B) or NULL) restate the
 * script's corruption `y_inpainting = (y + 1e-6) * mask` on the float64 clip (I_da/scripts/inpainting.py:186-192): the
 * addend is applied in fp64 to every sample of clip b and rounded to fp32 once, then the span is zeroed -- fused into
 * the first conv's loaders like I_ea's mask.  Clips of the clean stream pass mask_len = 0 and pre_mask_add = 0. */
typedef struct si_extract_desc {
    int32_t struct_size;        /* = sizeof(si_extract_desc) */
    int32_t output_layer;       /* L in 1..num_layers */
    int32_t normalize;          /* 0: wav is used as is; 1: HF processor (x - mean) / sqrt(var + 1e-7) (I_ea);
                                   2: F.layer_norm(x, x.shape): (x - mean) / sqrt(var + 1e-5) (I_da, task.cfg.normalize) */
    int32_t reserved;
} si_extract_desc;
int si_hubert_extract_features(si_ctx* ctx, const si_extract_desc* x, const float* wav, const int32_t* mask_start,
                               const int32_t* mask_len, const double* pre_mask_add, int B, int N, float* out_hidden,
                               void* workspace, size_t workspace_bytes, si_stream_t stream);

/* I_da's code splice (I_da/scripts/inpainting.py:209-214): the units predicted from the corrupted clip survive only
 * inside the mask -- `code_inpainting[: fs // hop] = code[: fs // hop]; code_inpainting[(fs + ms) // hop :] = code[...]`:
 * out[b][t] = (t < first[b] || t >= last[b]) ? code_clean[b][t] : code_masked[b][t], first = frame_start // code_hop_size,
 * last = (frame_start + mask_size) // code_hop_size.  code_* / out device int64 (B, T) (out may alias code_masked);
 * first / last device int32 (B).  Needs no weights. */
int si_code_splice(si_ctx* ctx, const int64_t* code_clean, const int64_t* code_masked, const int32_t* first, const int32_t* last,
                   int B, int T, int64_t* out, si_stream_t stream);

/* Codeword decision + splice: for b, j < Lm:  label = argmax_k cos(feats[b, pos_b + j], C_k - mean(C));
 * mel[b, :, pos_b + j] = C_label.   feats (B, T, D); frame_pos device int32 (B); mel (B, D, Tm) in/out;
 * labels device int64 (B, Lm), may be NULL. */
int si_codebook_splice(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_pos, int Lm,
                       float* mel, int Tm, int64_t* labels, si_stream_t stream);

/* The same with a per-clip frame COUNT (ragged batches; blind inpainting replaces all of a clip's own frames): frame_cnt device
 * int32 (B), 0 <= frame_cnt[b] <= Lm; labels (B, Lm) get -1 past a clip's count. */
int si_codebook_splice_varlen(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_pos, const int32_t* frame_cnt, int Lm,
                              float* mel, int Tm, int64_t* labels, si_stream_t stream);

/* Splice GIVEN codewords: mel[b, :, pos_b + j] = C[labels[b, j]] -- the script's `expected_inpaint` branch, which puts the
 * ground-truth centroids where si_codebook_splice puts the predicted ones (I_ea/predict.py:177-189: all_embeds_t_c[0, labels]
 * + center_).  labels device int64 (B, Lm); a label outside [0, K) or a frame outside [0, Tm) leaves that column untouched. */
int si_codebook_splice_labels(si_ctx* ctx, const int64_t* labels, int B, const int32_t* frame_pos, int Lm, float* mel, int Tm,
                              si_stream_t stream);

/* Loss half of the same LossFunction call: `loss, pred = cos_sim(values, labels)` and
 * `cos_sim_target_labels(pred, labels)` (I_ea/loss_fn.py:29-62, called at I_ea/predict.py:171-173).  feats / frame_pos / Lm
 * as si_codebook_splice (pass the gathered values with T = Lm and frame_pos = 0 to mirror the call exactly).
 * target_labels: device int64 (B, Lm).  Outputs (device): loss_terms fp32 (B, Lm) = 1 - cos(v, centred target centroid);
 * loss fp32 (1) = their sum in a fixed order; pred_labels int64 (B, Lm) or NULL; cos_pred_target fp32 (B, Lm) =
 * cos(centred predicted centroid, centred target centroid).  A target outside [0, K) gives NaN for that frame. */
int si_codebook_metrics(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_pos, int Lm,
                        const int64_t* target_labels, float* loss_terms, float* loss, int64_t* pred_labels,
                        float* cos_pred_target, si_stream_t stream);

/* k-means unit assignment: labels[r] = argmin_k ||feats[r] - centroids[k]||^2, first minimum on
 * ties -- what `kmeans_model.predict(feats)` returns at I_da/scripts/inpainting.py:204-205 (sklearn minimises
 * ||c||^2 - 2 x.c) and `ApplyKmeans.__call__` at I_ea/dataset/km_label.py:20-24.  feats device fp32 (rows, D),
 * centroids device fp32 (K, D) (caller-owned: I_da's unit codebook lives in HuBERT feature space, not in the context),
 * labels device int64 (rows), sq_dist optional device fp32 (rows).  Needs no weights.
 * The arg-min follows torch.argmin's rules (as `dist.argmin` / `np.argmin` do in the two scripts): a NaN score is the minimum, and
 * among equal scores, and among NaNs, the lowest index wins.  A stored label is therefore always in [0, K): a row that holds a NaN
 * gets label 0, as does a row whose scores are all NaN through inf - inf; a centroid that holds a NaN wins every row at the lowest
 * such index; a row whose scores all overflow to +inf gets label 0.  sq_dist of such a row is NaN or +-inf.  Finite rows of the same
 * call are not affected. */
int si_kmeans_assign(si_ctx* ctx, const float* feats, int64_t rows, int D, const float* centroids, int K, int64_t* labels,
                     float* sq_dist, si_stream_t stream);

/* Mel-domain metrics (row f-4, `Metrics.avg_cosine_sim / avg_d2_dist / rmse`, I_ea/metrics.py:38-62) of two mel segments
 * per clip: mel_a, mel_b device fp32 (B, D, L) channels-first; center device fp32 (D) (the codebook mean the reference
 * subtracts before the cosine) or NULL.  out3 device fp32 (B, 3) = {mean over frames of cos over bins of the centred
 * frames; mean over frames of 20/ln10 * sqrt(mean over bins of ((a - mean_bins a) - (b - mean_bins b))^2); the same with one
 * global mean}.  Needs no weights. */
int si_mel_metrics(si_ctx* ctx, const float* mel_a, const float* mel_b, int B, int D, int L, const float* center, float* out3,
                   si_stream_t stream);

/* Scale-invariant SDR in dB (`Metrics.sisdr`, I_ea/metrics.py:127-142) of est against ref, device fp32 (B, n) each;
 * out device fp32 (B).  eps = float32 machine epsilon, as np.finfo(x_est.dtype).eps for float32 waveforms. */
int si_sisdr(si_ctx* ctx, const float* est, const float* ref, int B, int n, float* out, si_stream_t stream);

/* I_da `CodeGenerator` front (I_da/src/model.py:148-189 in the look-up-table configuration of
 * I_da/configs/LJSpeech/hubert_lut.json): out = concat_channels( emb_c[code], emb_p[f0_code], spk_emb ) with the shorter
 * index series repeated frame-wise up to the longer (`_upsample`, :79-119; the lengths must divide) and the speaker
 * embedding vector repeated over all frames.  code device int64 (B, Fc); f0_code device int64 (B, Fp) or NULL (no pitch
 * part; the indices are what the fixed F0 VQ-VAE emits at :163-165 -- its conv encoder is si_f0_encoder_forward, its quantiser
 * si_kmeans_assign's arg-min); spk_emb device fp32 (B, E) or NULL; emb_c (Kc, E) / emb_p (Kp, E) device fp32
 * tables owned by the caller (they live in the CodeGenerator checkpoint, not in this context).  out device fp32
 * (B, nparts * E, max(Fc, Fp)) channels-first = the input of si_hifigan_forward(stretch = 0) for a generator whose
 * num_mels = nparts * E (384 for hubert_lut.json).  An index outside its table yields NaN.  Needs no weights. */
int si_unit_frontend(si_ctx* ctx, const int64_t* code, int Fc, const int64_t* f0_code, int Fp, const float* spk_emb,
                     const float* emb_c, int Kc, const float* emb_p, int Kp, int E, int B, float* out, si_stream_t stream);

/* The conv encoder of the fixed F0 VQ-VAE that `CodeGenerator.forward` runs on the F0 track (SURVEY 8(f) row f-2;
 * I_da/src/model.py:160-163 -> `FoVQVAE.encoder` = I_da/src/modules/jukebox.py `Encoder` :200-262 with one level of
 * `EncoderConvBlock` :11-116 and `Resnet1D` / `ResConv1DBlock` I_da/src/modules/resnet.py:29-97; configuration
 * I_da/configs/LJSpeech/hubert_lut.json:42-52): down_t x [Conv1d(k = 2 s (2 s + 1 for odd s), stride s, pad s / 2 (+ 1)) ->
 * depth x (x + Conv1d_k1(ReLU(Conv1d_k3, dilation growth^j, padding = dilation (ReLU(x)))))] -> Conv1d(width -> out_width, 3, 1, 1).
 * n_state = int(m_conv * width).  The quantiser behind it (`Bottleneck`, vq.py:117-127: arg-min of |x|^2 - 2 x.k + |k|^2)
 * is si_kmeans_assign on this function's output rows; the look-up + concat is si_unit_frontend.
 * weights: device fp32, packed in module order -- per down block: conv weight [width][cin][k], bias [width], then per
 * res block: k3 weight [n_state][width][3], bias, k1 weight [width][n_state][1], bias; last: weight [out_width][width][3],
 * bias (si_f0_encoder_weight_floats values).  f0: device fp32 (B, in_width, T).  h_out: device fp32 (B, T', out_width),
 * CHANNELS-LAST (the (N T, C) rows the bottleneck's `preprocess` builds at vq.py:92-95), T' = si_f0_encoder_frames(T). */
typedef struct si_f0enc_desc {
    int32_t in_width, out_width, width, n_state, depth, down_t, stride_t, dilation_growth;
} si_f0enc_desc;
size_t si_f0_encoder_weight_floats(const si_f0enc_desc* d);
int si_f0_encoder_frames(const si_f0enc_desc* d, int T);
size_t si_f0_encoder_workspace_bytes(const si_f0enc_desc* d, int B, int T);
int si_f0_encoder_forward(si_ctx* ctx, const si_f0enc_desc* d, const float* weights, const float* f0, int B, int T, float* h_out,
                          void* workspace, size_t workspace_bytes, si_stream_t stream);

/* Polyphase FIR resampler: the sample-rate conversions in front of the path, `librosa.load(path,
 * sr=22050)` / `sr=16000` at I_ea/predict.py:79-80.  y = upfirdn(taps, x, up, down)[pre_remove : pre_remove + n_out], i.e.
 * scipy.signal.resample_poly's arithmetic with a caller-designed filter: taps (device fp32) are the low-pass FIR
 * multiplied by `up` and already zero-pre-padded as resample_poly pads them; the host helper that designs them is
 * speech_inpainting_amd/audio.py::design_resampler.  x device fp32 (B, n_in), y device fp32 (B, n_out).  librosa's own
 * resampler (soxr / resampy) is a different filter; it is absent from the build image, so parity is against scipy. */
int si_resample_poly(si_ctx* ctx, const float* x, int B, int n_in, const float* taps, int ntaps, int up, int down,
                     int pre_remove, int n_out, float* y, si_stream_t stream);

/* librosa's OWN resampler: `librosa.load(path, sr=16000)` at I_ea/predict.py:79-80 is, in the pinned
 * librosa==0.9.1 (requirements.txt:3), `resample(..., res_type='kaiser_best')` = resampy's band-limited interpolation with its
 * `kaiser_best` table.  resampy is a third-party dependency absent from the build image (no version pinned by the reference); its
 * published algorithm is restated (oracle/ref_cpu.py::resample_kaiser_best) and pinned bit for bit by the fixture the reference
 * holds: I_ea/hifi_gan/test_files/LJ001-0001_{22k,16k}.wav (tests/golden/lj001_resample.npz).
 * The caller designs the tables on the host (speech_inpainting_amd/audio.py::design_kaiser_best) and owns them on the device:
 * win / dwin float64 (nwin): the windowed sinc's right wing (scaled by the ratio when down-sampling) and its forward differences;
 * time_reg float64 (n_time): output sample t's input time, 1 / ratio accumulated by repeated addition as resampy's loop does.
 * x (B, n_in) fp32; n_len device int32 (B) or NULL: ragged batches, clip b holds n_len[b] samples; y (B, n_out) fp32: samples
 * >= int(len_b * ratio) are zero (librosa's fix_length padding up to ceil(len * ratio)). */
typedef struct si_sinc_filter {
    int32_t struct_size;        /* = sizeof(si_sinc_filter) */
    int32_t nwin, num_table, step, n_time;
    int32_t reserved;
    double scale, ratio;
    const double* win;
    const double* dwin;
    const double* time_reg;
} si_sinc_filter;
int si_resample_sinc(si_ctx* ctx, const float* x, const int32_t* n_len, int B, int n_in, const si_sinc_filter* f, int n_out, float* y,
                     si_stream_t stream);

/* B6 on the device (I_ea/predict.py:204-206: `audio * 32768`, `.astype('int16')`): out[i] = the fp32 product truncated toward
 * zero; 32768.0 (an exactly saturated +1.0 sample, where the reference's cast is undefined behaviour) gives 32767, NaN gives 0.
 * wav device fp32 (n), out device int16 (n). */
int si_pcm16(si_ctx* ctx, const float* wav, int64_t n, int16_t* out, si_stream_t stream);

/* Vocoder: mel (B, D, Tm) -> time-stretch x441/256 -> generator -> wav_out (B, floor(Tm*441/256) * hop).
 * stretch = 0 skips extend_mel (mel already at the generator's frame rate; output (B, Tm * hop)). */
int si_hifigan_forward(si_ctx* ctx, const float* mel, int B, int Tm, int stretch, float* wav_out,
                       void* workspace, size_t workspace_bytes, si_stream_t stream);

/* `extend_mel` alone (I_ea/hifi_gan/inference_modified.py:16-19): mel (B, num_mels, Tm) -> out (B, num_mels, floor(Tm * 441 / 256)),
 * both channels-first -- the stretch si_hifigan_forward(stretch = 1) applies internally, as a separate step so that a WINDOW of the
 * stretched frames can be vocoded with stretch = 0 (the script's three generator passes differ only around the mask,
 * I_ea/predict.py:123-128,196-207: speech_inpainting_amd/engine.py::vocode_window). */
int si_extend_mel(si_ctx* ctx, const float* mel, int B, int Tm, float* out, si_stream_t stream);

/* Ragged batches: clip b holds mel_len[b] (HOST int32 (B), 1..Tm) frames of its (D, Tm) slab.  The stretch clamps at the clip's
 * own last frame and every convolution's zero padding begins at its own end, so the first si_vocoder_samples(mel_len[b]) samples
 * of row b equal that clip's waveform alone; the rest of the row (rows are si_vocoder_samples(Tm) long) is zero. */
int si_hifigan_forward_varlen(si_ctx* ctx, const float* mel, const int32_t* mel_len, int B, int Tm, int stretch, float* wav_out,
                              void* workspace, size_t workspace_bytes, si_stream_t stream);

/* Log-mel front-end of the vocoder side.  wave22: device fp32 (B, N22), the RAW 22.05 kHz clip.  Per clip the span
 * [mask_start[b], mask_end[b]) (device int32, samples; both NULL = no masking) is zeroed, the clip is divided by its
 * max |x| and scaled by 0.95 (normalize != 0; I_ea/predict.py:99-104), then get_mel (I_ea/dataset/mel_dump.py:40-98,
 * constants :11-20: n_fft = win = 1024, hop 441, reflect pad 312, 80 Slaney bands 0-8 kHz at 22.05 kHz) is applied.
 * mel_out: device fp32 (B, 80, Tm), Tm = si_mel_frames(N22): the layout si_codebook_splice / si_hifigan_forward take.
 * Needs no weights.  Workspace: si_mel_workspace_bytes. */
int si_mel_frames(int n22);                              /* (n22 + 2*312 - 1024) / 441 + 1, <= 0 when too short */
int si_mel_workspace_bytes(si_ctx* ctx, int B, int N22, size_t* out);
int si_mel_frontend(si_ctx* ctx, const float* wave22, const int32_t* mask_start, const int32_t* mask_end, int normalize,
                    int B, int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream);

/* Ragged batches: clip b holds sample_len[b] (HOST int32 (B)) samples of its row of N22; peak, reflect padding and frame count
 * are the clip's own.  mel_out (B, 80, si_mel_frames(N22)): frames >= si_mel_frames(sample_len[b]) of clip b are zero. */
int si_mel_frontend_varlen(si_ctx* ctx, const float* wave22, const int32_t* mask_start, const int32_t* mask_end, const int32_t* sample_len,
                           int normalize, int B, int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream);

/* ---- Several gaps per clip -------------------------------------------------------------------------------------------------
 * The reference's script zeroes ONE span per file (I_ea/predict.py:132-134 at 16 kHz, :99-102 at 22.05 kHz) and decides / splices the
 * frames of that one span (:164-168,184-187).  The calls below generalise exactly those lines to 0 .. SI_MAX_SPANS spans per clip,
 * different per clip of a batch; one span per clip reproduces the single-span entry points bit for bit.
 *
 * si_span_table: the zeroed sample spans of a batch as a CSR table.  Clip b owns entries [off[b], off[b + 1]) of start / len
 * (samples of the side the call works on: 16 kHz for the encoder, 22.05 kHz for the mel front-end), sorted by start, disjoint
 * (touching is allowed), every len >= 0 and start >= 0; the part of a span past the clip's end is ignored.  The table is given
 * twice: host_* (HOST int32) is what the call validates -- a table it refuses is never launched -- and span_* (DEVICE int32, the
 * same values, owned by the caller) is what the kernels read.  The library cannot see the device copy: keeping the two equal is the
 * CALLER's duty.  A device copy that differs from the validated host copy is read unvalidated -- the kernels stay inside the clip
 * (the span walk ends at off[b + 1], the conv0 fix-up is clamped to its window), so the result is WRONG OUTPUT, not a fault, and
 * no error is reported.  SI_MAX_SPANS is the cap on spans per clip. */
#define SI_MAX_SPANS 16
typedef struct si_span_table {
    int32_t struct_size;            /* = sizeof(si_span_table) */
    int32_t num_clips;              /* B of the call */
    int32_t num_spans;              /* = host_off[num_clips] */
    int32_t reserved;
    const int32_t* host_off;        /* HOST (num_clips + 1), host_off[0] = 0, non-decreasing */
    const int32_t* host_start;      /* HOST (num_spans) */
    const int32_t* host_len;        /* HOST (num_spans) */
    const int32_t* span_off;        /* DEVICE copies of the three */
    const int32_t* span_start;
    const int32_t* span_len;
} si_span_table;

/* si_hubert_forward / si_hubert_forward_varlen with a span table in place of mask_start / mask_len: the zero-mask of
 * I_ea/predict.py:132-134 for every span of the clip, then the processor's normalisation (:135-141) and CustomModel.forward
 * (I_ea/model.py:80-89).  sample_len: HOST int32 (B) = ragged batch as si_hubert_forward_varlen, or NULL = every clip holds N samples. */
int si_hubert_forward_spans(si_ctx* ctx, const float* wav, const si_span_table* spans, const int32_t* sample_len, int normalize,
                            int B, int N, float* out_feats, void* workspace, size_t workspace_bytes, si_stream_t stream);

/* si_mel_frontend / si_mel_frontend_varlen with a span table in place of [mask_start, mask_end): `wave_22[start:end] = 0` of
 * I_ea/predict.py:99-102 for every span, then normalize * 0.95 and get_mel (:104-106).  sample_len as above. */
int si_mel_frontend_spans(si_ctx* ctx, const float* wave22, const si_span_table* spans, const int32_t* sample_len, int normalize,
                          int B, int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream);

/* si_codebook_splice over a FRAME TABLE: entry f < F names frame frame_pos[f] of clip frame_clip[f] (device int32 (F) each) -- the
 * masked frames of all gaps of all clips, flattened; the gather + arg-max + centroid splice of I_ea/predict.py:164-168,171,184-187 per
 * entry.  labels device int64 (F), in table order, may be NULL; an entry outside the batch or the clip's T frames gets -1.
 * The table lives in device memory and is NOT validated: its entries must be distinct.  Two entries naming the same (clip, frame)
 * write the same mel column concurrently -- the same values here, an unordered pair of writes in si_codebook_splice_labels_spans
 * when their labels differ. */
int si_codebook_splice_spans(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_clip, const int32_t* frame_pos, int F,
                             float* mel, int Tm, int64_t* labels, si_stream_t stream);

/* si_codebook_splice_labels over a frame table (the `expected_inpaint` branch, I_ea/predict.py:177-189): labels device int64 (F). */
int si_codebook_splice_labels_spans(si_ctx* ctx, const int64_t* labels, int B, const int32_t* frame_clip, const int32_t* frame_pos, int F,
                                    float* mel, int Tm, si_stream_t stream);

/* si_codebook_metrics over a frame table (I_ea/loss_fn.py:29-62, called at I_ea/predict.py:171-173): target_labels, loss_terms,
 * pred_labels, cos_pred_target are flat (F), in table order; loss (1) = the fixed-order sum of the F terms. */
int si_codebook_metrics_spans(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_clip, const int32_t* frame_pos, int F,
                              const int64_t* target_labels, float* loss_terms, float* loss, int64_t* pred_labels, float* cos_pred_target,
                              si_stream_t stream);

/* ---- Patch mode: generated audio spliced into the original recording -----------------------------------------------------------
 * The reference's script writes the generator's waveform for the WHOLE clip (I_ea/predict.py:189,203-207: `generator(extend_mel(...))`,
 * `audio * MAX_WAV_VALUE`, `.astype('int16')`), at the level `librosa.util.normalize(wave_22) * 0.95` gave its input (:104).  The calls
 * below replace those lines for a caller who wants the recording back with only the gaps filled: the generator runs over windows of
 * the stretched mel, and its samples are cross-faded into the caller's own 22.05 kHz samples at the caller's own level.
 * Generator sample n IS 22.05 kHz input sample n (extend_mel centres stretched frame t at input sample (t + 0.5) * 256; 256 samples
 * per stretched frame), so a window row that starts at stretched frame w0 starts at input sample w0 * 256. */

/* The peak that si_mel_frontend(normalize != 0) divides by (I_ea/predict.py:104, `librosa.util.normalize`): peak_out[b] = max |x| over
 * clip b with its spans zeroed (:99-102) -- the existing front-end pass, exposed.  gain = peak / 0.95 undoes `x / peak * 0.95`.
 * spans: a 22.05 kHz si_span_table or NULL (no masking); sample_len: DEVICE int32 (B) or NULL (every clip holds N22 samples);
 * peak_out device fp32 (B).  Needs no weights. */
int si_wave_peak(si_ctx* ctx, const float* wave22, const si_span_table* spans, const int32_t* sample_len, int B, int N22, float* peak_out,
                 si_stream_t stream);

/* Windows of the stretched mel as the ragged generator batch (replaces the per-window slice copies in front of
 * si_hifigan_forward_varlen(stretch = 0); the stretch itself is si_extend_mel, I_ea/hifi_gan/inference_modified.py:16-19).
 * ext device fp32 (B, num_mels, Tout) channels-first; window w < W = stretched frames [w0[w], w1[w]) of clip clip[w], given twice as
 * [clip (W) | w0 (W) | w1 (W)]: host_win (HOST int32, validated: 0 <= clip < B, 0 <= w0 < w1 <= Tout, w1 - w0 <= Wmax; a table that
 * fails is never launched) and win (DEVICE int32, the same values, read by the kernel; keeping the two equal is the caller's duty, as
 * for si_span_table).  out device fp32 (W, num_mels, Wmax): row (w, d) = ext[clip, d, w0:w1], zero past it. */
int si_gather_windows(si_ctx* ctx, const float* ext, int B, int Tout, const int32_t* host_win, const int32_t* win, int W, int Wmax,
                      float* out, si_stream_t stream);

/* si_patch_table: where the generated samples of each span lie.  Window w < num_windows is one row of `gen`: it belongs to clip
 * win_clip[w], its first sample is 22.05 kHz sample win_start[w] of that clip and it holds win_len[w] samples.  Span k of the span
 * table (same order) takes its samples from window span_win[k].  lim[b] = min(clip b's samples, clip b's generated samples): nothing
 * at or past it is replaced.  ramp: DEVICE fp32 (fade), the rising half of the cross-fade, w[i] = 0.5 (1 - cos(pi (i + 0.5) / fade))
 * rounded once from float64 (speech_inpainting_amd/gaps.py::fade_ramp); the kernel reads it and evaluates no cosine.
 * host_* (HOST) are validated, the DEVICE copies are read: the si_span_table rule. */
typedef struct si_patch_table {
    int32_t struct_size;            /* = sizeof(si_patch_table) */
    int32_t num_clips;              /* B of the call */
    int32_t num_windows;            /* W: rows of gen */
    int32_t num_spans;              /* = the span table's num_spans */
    int32_t fade;                   /* cross-fade length in samples, >= 0 (0 = hard splice) */
    int32_t reserved;
    const int32_t* host_win_clip;   /* HOST (num_windows) */
    const int32_t* host_win_start;  /* HOST (num_windows) */
    const int32_t* host_win_len;    /* HOST (num_windows) */
    const int32_t* host_span_win;   /* HOST (num_spans) */
    const int32_t* host_lim;        /* HOST (num_clips) */
    const int32_t* win_start;       /* DEVICE copies of the last four */
    const int32_t* win_len;
    const int32_t* span_win;
    const int32_t* lim;
    const float* ramp;              /* DEVICE (fade), may be NULL when fade = 0 */
} si_patch_table;

/* The composition + B6 (replaces I_ea/predict.py:203-207 for a patched clip, and the host-side paste a caller of the whole-clip output
 * would write).  Per clip b and span [s, e) of `spans` (22.05 kHz; spans of length 0 or starting at / past lim[b] are skipped) the
 * blend region is [max(s - fade, 0), min(e + fade, lim[b])); the weight of sample m is ramp[m - (s - fade)] on the rise, 1 in [s, e),
 * ramp[e + fade - 1 - m] on the fall, the MAXIMUM over the clip's spans, 0 elsewhere.  Output sample m:
 *   weight 0:  orig's bits, unchanged (-0.0 and NaN payloads included);
 *   weight 1:  exactly the fp32 product gain[b] * gen;
 *   else:      fma(w, gain[b] * gen, (1 - w) * orig).
 * orig device fp32 (B, N22); sample_len HOST int32 (B) or NULL: ragged batch, lim[b] <= sample_len[b] <= N22 is checked; gen device
 * fp32 (num_windows, Lrow); gain device fp32 (B) or NULL (= 1); out_f32 device fp32 (B, N22) and / or out_pcm device int16 (B, N22) =
 * si_pcm16's arithmetic on the same values (one of them may be NULL).  Rows are copied whole: samples past a ragged clip's end too.
 * SI_EINVAL before any launch for: NULL / mis-sized structs; fade < 0; both outputs NULL; a window outside its clip (clip not in
 * [0, B), start < 0, len < 0 or > Lrow, start + len > N22); a span whose window index is outside [0, num_windows) or names a window of
 * another clip, or whose blend region leaves the window's row. */
int si_patch_compose(si_ctx* ctx, const float* orig, const si_span_table* spans, const int32_t* sample_len, const si_patch_table* patch,
                     const float* gen, int Lrow, const float* gain, int B, int N22, float* out_f32, int16_t* out_pcm, si_stream_t stream);

/* ---- Long recordings: many context clips cut from, and patched back into, ONE recording -------------------------
 * The reference's script handles one file of clip length per run (I_ea/predict.py:76-207).  A recording of any length is served as a
 * set of context clips that start on the recording's 20 ms frame grid (frame f = 22.05 kHz sample 441 f = 16 kHz sample 320 f), each
 * through the span-table calls above; the two calls below are the ends of that route. */

/* The clips, cut on the device (stands for the script's per-file `librosa.load`, I_ea/predict.py:79-80, when the files are slices of
 * one recording): out (C, L) row c = src[start[c] : start[c] + L].  src device fp32 (n_src), one channel, either sample rate.  start is
 * given twice, the si_span_table rule: host_start (HOST int32 (C)) is validated -- any start < 0 or start + L > n_src refuses the call
 * and nothing is launched -- and start (DEVICE int32 (C), the same values) is read.  n_src <= 2^31 - 1 - 2048.  Bits are copied
 * unchanged (-0.0, NaN payloads). */
int si_cut_clips(si_ctx* ctx, const float* src, int n_src, const int32_t* host_start, const int32_t* start, int C, int L, float* out,
                 si_stream_t stream);

/* si_region_table: the blend regions of MANY context clips on the recording's own 22.05 kHz sample axis.  Span k < num_spans is
 * samples [start[k], start[k] + len[k]) of the recording (len > 0; sorted by start, disjoint); its generated samples lie in row
 * span_win[k] of `gen`; nothing at or past span_lim[k] -- the recording sample where the audio its context generated ends,
 * start of the context + min(its samples, its generated samples), > start[k] -- is replaced.  Window w < num_windows is one row of
 * `gen`: it belongs to context win_ctx[w] (the index into `gain`), its first sample is recording sample win_start[w] and it holds
 * win_len[w] samples.  The kernel runs one workgroup per TOUCHED chunk of 2048 samples: entry q < num_chunks names chunk chunk[q]
 * (strictly increasing, chunk * 2048 < N22) and the spans [k0[q], k1[q]) whose regions [max(start - fade, 0), min(start + len + fade,
 * span_lim)) meet it (speech_inpainting_amd/gaps.py::region_chunks).  ramp as si_patch_table's.  host_* (HOST) are validated, the DEVICE
 * copies are read: the si_span_table rule. */
typedef struct si_region_table {
    int32_t struct_size;            /* = sizeof(si_region_table) */
    int32_t num_contexts;           /* C: entries of gain */
    int32_t num_windows;            /* W: rows of gen */
    int32_t num_spans;              /* K */
    int32_t num_chunks;             /* Q: workgroups of the launch */
    int32_t fade;                   /* cross-fade length in samples, >= 0 (0 = hard splice) */
    const int32_t* host_start;      /* HOST (num_spans) */
    const int32_t* host_len;        /* HOST (num_spans) */
    const int32_t* host_span_win;   /* HOST (num_spans) */
    const int32_t* host_span_lim;   /* HOST (num_spans) */
    const int32_t* host_win_ctx;    /* HOST (num_windows) */
    const int32_t* host_win_start;  /* HOST (num_windows) */
    const int32_t* host_win_len;    /* HOST (num_windows) */
    const int32_t* host_chunk;      /* HOST (num_chunks) */
    const int32_t* host_k0;         /* HOST (num_chunks) */
    const int32_t* host_k1;         /* HOST (num_chunks) */
    const int32_t* start;           /* DEVICE copies of the ten */
    const int32_t* len;
    const int32_t* span_win;
    const int32_t* span_lim;
    const int32_t* win_ctx;
    const int32_t* win_start;
    const int32_t* win_len;
    const int32_t* chunk;
    const int32_t* k0;
    const int32_t* k1;
    const float* ramp;              /* DEVICE (fade), may be NULL when fade = 0 */
} si_region_table;

/* The write-out of the gaps of many context clips into the one recording (replaces I_ea/predict.py:203-207 per clip plus the host-side
 * paste of each clip's gaps into the long file).  Per sample m of a listed chunk the weight is si_patch_compose's: the MAXIMUM over
 * the chunk's spans of ramp[m - (s - fade)] on the rise, 1 in [s, s + len), ramp[s + len + fade - 1 - m] on the fall, 0 at and past the
 * span's span_lim.  A sample of weight 0 is NOT WRITTEN: out_f32 / out_pcm keep what the caller put there (a copy of the recording).
 * Otherwise g = gain[win_ctx[win]] * gen[win, m - win_start[win]] and the sample is g (weight 1) or fma(w, g, (1 - w) * orig[m]):
 * si_patch_compose's roundings in its order, so every written sample equals what si_patch_compose writes for the context clip alone.
 * orig device fp32 (N22), read only (never out_f32: a repeated call gives the same result); gen device fp32 (num_windows, Lrow); gain
 * device fp32 (num_contexts) or NULL (= 1); out_f32 device fp32 (N22) and / or out_pcm device int16 (N22), si_pcm16's arithmetic on the
 * same values (one of them may be NULL).  Sample indices are int32: N22 <= 2^31 - 1 - 2048.
 * SI_EINVAL before any launch, naming the entry, for: NULL / mis-sized struct; fade < 0; both outputs NULL; N22 out of range; a span
 * with len <= 0, start < 0, span_lim <= start or span_lim > N22, or not after its predecessor's end; a window index or context index
 * out of range; a window with start < 0, len < 0 or > Lrow, start + len > N22; a span whose region leaves its window's row; chunks
 * not strictly increasing or at / past N22; k0 / k1 outside 0 <= k0 <= k1 <= num_spans; a region that meets a chunk the list lacks, or
 * whose span is outside that chunk's [k0, k1).  num_chunks = 0 launches nothing and succeeds. */
int si_patch_regions(si_ctx* ctx, const float* orig, int N22, const si_region_table* table, const float* gen, int Lrow, const float* gain,
                     float* out_f32, int16_t* out_pcm, si_stream_t stream);

/* ---- The sample types of the file-typed calls -------------------------------------------------------------------------
 * The sixteen calls that take a file as it lies on disk -- si_quiet_runs[_ch], si_dead_runs, si_level_runs, si_burst_runs, si_invalid_runs,
 * si_cut_rate[_ch], si_cut_pair[_ch], si_cut_rate_valid, si_cut_pair_valid, si_patch_rate[_ch] (si_cut_clips_valid takes fp32 alone) -- and, since DESIGN.md 4.33, si_impulse_runs and si_impulse_residual name its sample type in their `is_pcm16` argument.  Pass one of:
 *   SI_SAMPLE_F32 = 0   fp32
 *   SI_SAMPLE_S16 = 1   int16 PCM; a sample enters the cutters and the patch as (float)v / 32768, exact
 *   SI_SAMPLE_S24 = 2   packed little-endian signed 24-bit PCM, three bytes per sample, (n, ch) interleaved as a WAV data chunk holds
 *                       it (blockAlign = 3 ch).  A sample v in [-2^23, 2^23 - 1] enters every kernel as v * 2^-23, exact in fp32.
 *                       x / orig / out point at the first byte and may start at ANY byte; no byte before the base or at / after
 *                       3 n ch is read.  `threshold` and `held_tol` count 24-bit steps, as they count int16 steps for int16
 *                       (rel_threshold, half, min_len are not scaled): |v| and the held difference (2^24 - 1 at most) are taken in
 *                       int32 and are exact in fp32, si_level_runs' squares (2^46 at most) in int64 and are exact in float64, si_burst_runs'
 *                       second difference (below 2^26) in int32 and its square as a product of two doubles (below 2^52, exact), and
 *                       threshold_out receives T in 24-bit steps.  si_patch_rate[_ch] store a blend w as trunc(w * 8388608) clamped to
 *                       [-8388608, 8388607], NaN -> 0 (si_pcm16's statement at 24 bits), with stores of exactly the sample's three
 *                       bytes: no byte of a neighbouring sample or channel is written or rewritten.
 * Any other non-zero value means what it meant before 2 was given a meaning, int16; no caller should pass one.  n, n_file and channels
 * obey the same limits for every type; byte offsets ((i ch + channel) * 3) are 64-bit.  Every result for an s24 file V equals the
 * call's result on its fp32 image V * 2^-23 with threshold and held_tol times 2^-23: the runs row for row, the clips byte for byte, and
 * a patched sample is the store rule above applied to the fp32 the call writes for the image. */
#define SI_SAMPLE_F32 0
#define SI_SAMPLE_S16 1
#define SI_SAMPLE_S24 2

/* ---- Dropout detection: where the gaps of a damaged recording are -------------------------------------------------
 * The reference has no detection: the script's user types the one mask into predict.yaml (I_ea/predict.py:85-90).  This call finds
 * what a digital dropout leaves behind -- runs of (near) digital silence from lost packets, underruns or muted samples -- on the
 * device, where the recording already lies; gaps.runs_to_gaps turns the runs into gaps on the 20 ms grid.
 * x device, n samples, one channel, any sample rate: fp32 (is_pcm16 = SI_SAMPLE_F32), int16 PCM as it lies in a file (SI_SAMPLE_S16)
 * or packed 24-bit PCM (SI_SAMPLE_S24: threshold in 24-bit steps; see above); the base needs only its element's alignment, any
 * byte for s24.  Sample i is QUIET iff |x[i]| <= threshold: NaN is loud, -0.0 is quiet, |-32768| is taken in
 * int32, samples at and past n are loud.  The result is every MAXIMAL run of quiet samples of at least min_len samples, as int32
 * (start, len) rows SORTED BY START: rows [0, min(total, max_runs)) of runs (device int32 (max_runs, 2)) are written, rows at and past
 * that are not touched, and n_runs (device int32 (1)) receives the TOTAL number of such runs whether or not they all fit.  The same
 * input gives the same bytes (no atomics; plain stores).  max_runs = 0 counts only (runs may be NULL).  Needs no weights.  Scratch
 * (one bit per sample, six words per 2048 samples) is the context's own and is reused by the next call in stream order.
 * SI_EINVAL before any launch, naming the argument, for: NULL x or n_runs; NULL runs with max_runs > 0; n < 1 or n > 2^31 - 1 - 2048;
 * threshold negative or NaN; min_len < 1; max_runs < 0. */
int si_quiet_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, float threshold, int min_len, int32_t* runs, int max_runs,
                  int32_t* n_runs, si_stream_t stream);

/* ---- Repair at the file's own sample rate -----------------------------------------------------------------------------
 * The reference's script resamples its input to 22.05 kHz and writes 22.05 kHz (I_ea/predict.py:79-80,203-207); si_patch_regions keeps
 * the recording's own samples only when the file already is at that rate.  The call below replaces, for a file at ANY rate sr, the
 * `engine.resample(patched, 22050, sr)` over the whole repaired recording that would otherwise bring it back (si_resample_sinc, row f-3)
 * together with si_patch_regions' write-out: the recording stays at sr in its own sample type, and only the generated audio around each
 * gap is carried from 22.05 kHz to sr -- by si_resample_sinc's band-limited interpolation at the EXACT rational time -- and blended in.
 *
 * si_rate_table: si_region_table with the spans on the FILE's sample axis.  With g = gcd(22050, sr), P = 22050 / g, Q = sr / g, file
 * sample i sits at position i P / Q of the 22.05 kHz axis.  Span k < num_spans is FILE samples [start[k], start[k] + len[k]) (len > 0;
 * sorted, disjoint); nothing at or past file sample span_lim[k] is written; its generated samples lie in row span_win[k] of `gen`.
 * Window w < num_windows is one row of `gen` and stays on the 22.05 kHz axis: context win_ctx[w] (the index into `gain`), first sample =
 * 22.05 kHz sample win_start[w] of the recording, win_len[w] samples, and win_lim[w] = the 22.05 kHz sample where its context's
 * generated audio ends.  Chunks are chunks of 2048 FILE samples, listed as in si_region_table (gaps.region_chunks); fade and ramp are in
 * file samples.  host_* (HOST) are validated, the DEVICE copies are read: the si_span_table rule. */
typedef struct si_rate_table {
    int32_t struct_size;            /* = sizeof(si_rate_table) */
    int32_t num_contexts;           /* C: entries of gain */
    int32_t num_windows;            /* W: rows of gen */
    int32_t num_spans;              /* K */
    int32_t num_chunks;             /* Q: workgroups of the launch */
    int32_t fade;                   /* cross-fade length in FILE samples, >= 0 (0 = hard splice) */
    const int32_t* host_start;      /* HOST (num_spans), file samples */
    const int32_t* host_len;        /* HOST (num_spans), file samples */
    const int32_t* host_span_win;   /* HOST (num_spans) */
    const int32_t* host_span_lim;   /* HOST (num_spans), file samples */
    const int32_t* host_win_ctx;    /* HOST (num_windows) */
    const int32_t* host_win_start;  /* HOST (num_windows), 22.05 kHz samples */
    const int32_t* host_win_len;    /* HOST (num_windows), 22.05 kHz samples */
    const int32_t* host_win_lim;    /* HOST (num_windows), 22.05 kHz samples */
    const int32_t* host_chunk;      /* HOST (num_chunks) */
    const int32_t* host_k0;         /* HOST (num_chunks) */
    const int32_t* host_k1;         /* HOST (num_chunks) */
    const int32_t* start;           /* DEVICE copies of the eleven */
    const int32_t* len;
    const int32_t* span_win;
    const int32_t* span_lim;
    const int32_t* win_ctx;
    const int32_t* win_start;
    const int32_t* win_len;
    const int32_t* win_lim;
    const int32_t* chunk;
    const int32_t* k0;
    const int32_t* k1;
    const float* ramp;              /* DEVICE (fade), may be NULL when fade = 0 */
} si_rate_table;

/* Per file sample i of a listed chunk the weight w is si_patch_regions' on the file axis: the MAXIMUM over the chunk's spans of
 * ramp[i - (s - fade)] on the rise, 1 in [s, s + len), ramp[s + len + fade - 1 - i] on the fall, 0 at and past span_lim; the first span
 * of the greatest weight supplies the window.  A sample of weight 0 is NOT WRITTEN: `out` keeps the caller's copy of the recording.
 * The generated sample at file sample i: n, r = divmod(i P, Q) in 64-bit integers, frac = scale (r / Q), and with the tables of
 * `filt` (audio.design_kaiser_best(22050, sr, .): win, dwin, nwin, num_table, step, scale; time_reg, n_time and ratio are NOT read)
 *     left wing   off, eta = split(frac num_table):            taps k < min(n + 1, (nwin - off) / step) weigh x[n - k]
 *     right wing  off', eta' = split((scale - frac) num_table): taps k < (nwin - off') / step            weigh x[n + 1 + k]
 * by fma(eta, dwin[off + k step], win[off + k step]), accumulated by fma in float64 in that order (left ascending, then right ascending)
 * and rounded once to fp32 -- si_resample_sinc's arithmetic at the exact time, so a sample has the same bits wherever its window row
 * starts and however the chunks are listed.  x[j] is 22.05 kHz sample j of the recording's generated audio, read from the window's row;
 * j < 0 and j >= win_lim read as zero.  Then g = gain[win_ctx] * y and the sample is g (w = 1) or fma(w, g, (1 - w) * orig[i]):
 * si_patch_regions' roundings in its order.  orig / out: device, n_file samples of the SAME type, fp32 (is_pcm16 = SI_SAMPLE_F32), int16
 * PCM (SI_SAMPLE_S16: orig = (float)v / 32768, the result stored by si_pcm16's arithmetic) or packed 24-bit PCM (SI_SAMPLE_S24: orig =
 * v * 2^-23, the result stored by the 24-bit store rule above, three bytes per written sample); a base needs only its element's alignment;
 * orig is read only and must not be out.  gen device fp32 (num_windows, Lrow); gain device fp32 (num_contexts) or NULL (= 1).
 * SI_EINVAL before any launch, naming the entry, for: everything si_patch_regions refuses, on the file axis; sr outside 4000 .. 192000
 * or equal to 22050; n_file, or its 22.05 kHz length ceil(n_file P / Q), above 2^31 - 1 - 2048; a filter with nwin < 2, num_table < 1,
 * step < 1, scale outside (0, 1] or NULL tables; a window outside that 22.05 kHz length or with win_lim outside (win_start, length];
 * a span whose span_lim reaches a sample at or past its window's win_lim; a span whose region [max(s - fade, 0), min(s + len + fade,
 * span_lim)), mapped to 22.05 kHz samples [floor(a P / Q) - H, floor((b - 1) P / Q) + 1 + H) with H = ceil(nwin / step), leaves its
 * window's row other than before sample 0 or at or past win_lim.  num_chunks = 0 launches nothing and succeeds. */
int si_patch_rate(si_ctx* ctx, const void* orig, int is_pcm16, int n_file, int sr, const si_rate_table* table, const float* gen, int Lrow,
                  const float* gain, const si_sinc_filter* filt, void* out, si_stream_t stream);

/* ---- Context clips cut at the file's own sample rate ------------------------------------------------------------------
 * The reference's script resamples its whole input to 22.05 kHz before anything else (I_ea/predict.py:79-80).  For a long file with a
 * few gaps that pass -- si_resample_sinc over every sample, an fp32 copy of an int16 file, a 22.05 kHz copy of the recording and a
 * float64 time table of its length -- is the one cost that scales with the file instead of the damage.  The call below replaces it
 * together with si_cut_clips: it computes ONLY the 22.05 kHz samples of the context clips, straight from the file's own samples.
 *
 * With g = gcd(22050, sr), P = 22050 / g, Q = sr / g, sample j of the recording's 22.05 kHz axis sits at file position j Q / P, and the
 * recording has N22 = ceil(n_file P / Q) such samples (every j < N22 has its position inside the file).  out (C, L) fp32, row c =
 * samples [start[c], start[c] + L) of that axis; the starts are arbitrary (not tied to any frame grid), clips may overlap and come in
 * any order.  Sample j: n, r = divmod(j Q, P) in 64-bit integers, frac = scale (r / P), and with the tables of `filt`
 * (audio.design_kaiser_best(sr, 22050, .): win -- scaled by the ratio when down-sampling --, dwin, nwin, num_table, step, scale;
 * time_reg, n_time and ratio are NOT read)
 *     left wing   off, eta = split(frac num_table):            taps k < min(n + 1, (nwin - off) / step)           weigh x[n - k]
 *     right wing  off', eta' = split((scale - frac) num_table): taps k < min(n_file - n - 1, (nwin - off') / step) weigh x[n + 1 + k]
 * by fma(eta, dwin[off + k step], win[off + k step]), accumulated by fma in float64 in that order (left ascending, then right ascending)
 * and rounded once to fp32 -- si_resample_sinc's arithmetic at the EXACT time instead of 1 / ratio accumulated by repeated addition.  File
 * samples before 0 and at or past n_file do not exist (the tap counts say so).  Two deliberate differences from si_resample_sinc over
 * the whole file: (a) at exactly-integer times (j a multiple of P) frac is exactly 0, where the accumulated rounding picks the table
 * phase; elsewhere a result moves by at most an fp32 rounding; (b) the last sample j = N22 - 1 is interpolated when n_file P / Q is no
 * integer, where si_resample_sinc writes zero at and past int(n ratio).
 * x: device, n_file samples, fp32 (is_pcm16 = SI_SAMPLE_F32), int16 PCM (SI_SAMPLE_S16: a sample enters as (float)v / 32768, exact) or
 * packed 24-bit PCM (SI_SAMPLE_S24: v * 2^-23, exact; si_cut_pair takes the same three); the base
 * needs only its element's alignment.  host_start (HOST, C) is validated, start (DEVICE, C) is read: the si_span_table rule.  One
 * workgroup owns a tile of SI_CUT_RATE_TILE consecutive outputs of one clip.
 * SI_EINVAL before any launch, naming the argument, for: NULL pointers; sr outside 4000 .. 192000 or equal to 22050; n_file < 1; n_file
 * or N22 above 2^31 - 1 - 2048; a filter si_patch_rate would refuse (nwin < 2, num_table < 1, step < 1, scale outside (0, 1], NULL
 * tables, or so many taps per wing that a tile's staged samples exceed 64 KB); C < 0 or above 65535; L < 1; any start < 0 or
 * start + L > N22.  C = 0 launches nothing and succeeds. */
#define SI_CUT_RATE_TILE 512
int si_cut_rate(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int sr, const int32_t* host_start, const int32_t* start, int C, int L,
                const si_sinc_filter* filt, float* out, si_stream_t stream);

/* ---- Interleaved multi-channel files ----------------------------------------------------------------------------------
 * The reference's script mixes its input down to one channel on load (librosa.load, I_ea/predict.py:79).  The three calls below serve a
 * file as a WAV stores it: x is (n, channels) INTERLEAVED, element i * channels + c is channel c at sample time i, 1 <= channels <=
 * SI_MAX_CHANNELS.  n, n_file, runs, spans, chunks, fades and starts count SAMPLE TIMES and obey the mono limits (n <= 2^31 - 1 - 2048);
 * n * channels may pass 2^31, every element offset is 64-bit.  Each channel is a mono recording: whatever a call computes for channel c
 * is, byte for byte, what its mono sibling computes on the de-interleaved channel, and no de-interleaved copy is made.
 *
 * si_quiet_runs_ch: si_quiet_runs with sample time i quiet iff |x[i * channels + channel]| <= threshold (0 <= channel < channels), or,
 * for channel = -1, iff EVERY channel's element is (a joint dropout).  NaN, -0.0, -32768 and "past n is loud" as si_quiet_runs; the same
 * sorted (start, len) rows in sample times, the total in n_runs, max_runs = 0 counts only; the same input gives the same bytes.  With
 * channels = 1 (channel 0 or -1) the output bytes are si_quiet_runs'.  SI_EINVAL before any launch, naming the argument, for everything
 * si_quiet_runs refuses, channels outside 1 .. SI_MAX_CHANNELS, and channel outside [-1, channels).
 *
 * si_cut_rate_ch: si_cut_rate reading channel `channel` of the interleaved file x (n_file sample times).  A file sample time outside
 * [0, n_file) does not exist: it is never the neighbouring channel's element.  SI_EINVAL before any launch, naming the argument, for
 * everything si_cut_rate refuses, channels outside 1 .. SI_MAX_CHANNELS, and channel outside [0, channels).
 *
 * si_patch_rate_ch: si_patch_rate whose spans and chunks are sample times of channel `channel`; orig and out are interleaved, (n_file,
 * channels) of the same type.  Only elements i * channels + channel of sample times i with non-zero weight are written: the other
 * channels, and this channel outside its regions, keep what the caller put there.  The table may name windows and contexts that none of
 * its spans use (another channel's rows of gen and entries of gain, when the channels share a pass).  SI_EINVAL before any launch,
 * naming the entry, for everything si_patch_rate refuses, channels outside 1 .. SI_MAX_CHANNELS, and channel outside [0, channels). */
#define SI_MAX_CHANNELS 8
int si_quiet_runs_ch(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, float threshold, int min_len, int32_t* runs,
                     int max_runs, int32_t* n_runs, si_stream_t stream);
int si_cut_rate_ch(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_start,
                   const int32_t* start, int C, int L, const si_sinc_filter* filt, float* out, si_stream_t stream);
int si_patch_rate_ch(si_ctx* ctx, const void* orig, int is_pcm16, int n_file, int channels, int channel, int sr, const si_rate_table* table,
                     const float* gen, int Lrow, const float* gain, const si_sinc_filter* filt, void* out, si_stream_t stream);

/* ---- Both clip sets of a pass cut straight from the file, in one launch ------------------------------------------------
 * The reference loads its input twice, each time from the file's own samples: librosa.load(path, sr=22050) for the mel and
 * librosa.load(path, sr=16000) for HuBERT (I_ea/predict.py:79-80).  si_cut_rate serves the first; the calls below serve both, so that
 * the encoder's 16 kHz clips are not a second resampling of the 22.05 kHz clips (with nothing before or after each clip) but the file's
 * samples at the exact 16 kHz times -- and, for a 16 kHz file, the file's samples themselves, as librosa resamples nothing at equal rates.
 *
 * A clip starts on the 20 ms frame grid, the only grid the two rates share (gcd(22050, 16000) = 50): frame f is 22.05 kHz sample 441 f
 * and 16 kHz sample 320 f.  out22 (C, L22) row c = 22.05 kHz samples 441 frame[c] + [0, L22), by si_cut_rate's definition with filt22
 * (audio.design_kaiser_best(sr, 22050, .)): the bytes are si_cut_rate's.  out16 (C, L16) row c = 16 kHz samples j = 320 frame[c] +
 * [0, L16): with (P16, Q16) = (16000, sr) / gcd, sample j sits at file position j Q16 / P16, n, r = divmod(j Q16, P16) in 64-bit
 * integers, frac = scale (r / P16), and the two wings, their tap counts, the fma order and the single rounding to fp32 are si_cut_rate's
 * on the tables of filt16 (audio.design_kaiser_best(sr, 16000, .); time_reg, n_time and ratio are NOT read).  The recording has
 * N16 = ceil(n_file P16 / Q16) samples at 16 kHz; an output with j >= N16 lies at or past the file's end and is +0.0.
 * sr = 16000: the 16 kHz row is the file's own samples, x[j] (fp32) or (float)v / 32768 (int16); no filter is applied and filt16 must be
 * NULL, as it must be non-NULL at every other rate.  An int16 sample enters as (float)v / 32768; file samples outside [0, n_file) do not
 * exist; a sample has the same bits in whichever clip, tile or batch it is cut.
 * x as si_cut_rate's (si_cut_pair_ch: as si_cut_rate_ch's, channel `channel` of an interleaved file, never the neighbouring channel's
 * element).  host_frame (HOST, C) is validated, frame (DEVICE, C) is read: the si_span_table rule; a device table that differs gives
 * zeros, never a read outside the file.  One workgroup owns SI_CUT_PAIR_FRAMES consecutive frames of one clip (441 + 320 outputs each)
 * and stages the file samples both rates read for them once, ceil(SI_CUT_PAIR_FRAMES sr / 50) + 2 + 2 max(H22, H16) floats of LDS.
 * SI_EINVAL before any launch, naming the argument, for everything si_cut_rate[_ch] refuses (L is L22, start is 441 frame, filt is
 * filt22), and: L16 < 1; a frame with 441 f + L22 > N22 or 320 f + L16 > ceil(N22 320 / 441) (which exceeds N16 by at most 1); filt16
 * NULL when sr != 16000 or non-NULL when sr = 16000; a filt16 that fails filt22's checks; a staged tile above 64 KB.  C = 0 launches
 * nothing and succeeds. */
#define SI_CUT_PAIR_FRAMES 1
int si_cut_pair(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int sr, const int32_t* host_frame, const int32_t* frame, int C, int L22,
                int L16, const si_sinc_filter* filt22, const si_sinc_filter* filt16, float* out22, float* out16, si_stream_t stream);
int si_cut_pair_ch(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_frame,
                   const int32_t* frame, int C, int L22, int L16, const si_sinc_filter* filt22, const si_sinc_filter* filt16, float* out22,
                   float* out16, si_stream_t stream);

/* ---- Held-sample and peak-relative dropouts ---------------------------------------------------------------------------
 * The reference has no detection: the script's user types the one mask into predict.yaml (I_ea/predict.py:85-90).  si_quiet_runs finds
 * digital silence against a fixed number; this call finds the other two things an underrun leaves behind -- a sample that is HELD (the
 * last one repeated, a DC level) and a mute that is not exact zeros (dither, a noise floor), judged against the file's own peak -- with
 * si_quiet_runs' output and limits.  x is si_quiet_runs_ch's: (n, channels) interleaved, fp32 or int16; channels = 1 is a mono file
 * (channel 0 or -1) and gives the bytes of the mono layout.  For one channel x[0 .. n) (elements i * channels + c):
 *   peak      the largest |x[i]| over the FINITE samples (NaN and +-inf are skipped; int16 magnitudes are taken in int32, |-32768| =
 *             32768, exact in fp32); 0 when none qualifies.  Samples at and past n, and in front of the base, do not exist.
 *   T         max(threshold, fl32(rel_threshold * peak)), the product ONE fp32 multiply.  With rel_threshold == 0 the peak is not
 *             computed and T = threshold.
 *   quiet(i)  |x[i]| <= T, as si_quiet_runs: NaN is loud, -0.0 is quiet.
 *   link(i)   for 1 <= i < n: |x[i] - x[i - 1]| <= held_tol.  fp32: the subtraction in fp32, one rounding; a NaN neighbour and
 *             inf - inf give false.  int16: the subtraction in int32, the magnitude compared as a float (32767 - (-32768) = 65535, no
 *             wrap).  There is no link at i = 0 and none to x[n].
 *   held(i)   link(i) or link(i + 1): the sample equals a neighbour to within held_tol.
 *   dead(i)   (kind & SI_DEAD_QUIET and quiet(i)) or (kind & SI_DEAD_HELD and held(i)).
 * channel >= 0 scans that channel: its neighbours are elements (i +- 1) * channels + channel, never the adjacent elements, and the peak
 * is taken over that channel's elements.  channel = -1 is JOINT: a sample time is dead when EVERY channel's element is dead, each by
 * its own links, and the peak is one value over all elements of the file.
 * The result is every maximal run of dead samples of at least min_len samples: int32 (start, len) rows sorted by start, rows [0,
 * min(total, max_runs)) written and the rows past them untouched, the total in n_runs (device int32 (1)); the same input gives the same
 * bytes (no atomics; plain stores).  threshold_out, when not NULL, is a device fp32 word that receives T.  Scratch is si_quiet_runs'
 * (one more word per 2048 samples, and two).
 * SI_EINVAL before any launch, naming the argument, for: everything si_quiet_runs_ch refuses; kind outside 1 .. 3; rel_threshold NaN or
 * outside [0, 1]; held_tol negative or NaN (checked whether or not kind has SI_DEAD_HELD). */
#define SI_DEAD_QUIET 1
#define SI_DEAD_HELD 2
int si_dead_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int kind, float threshold, float rel_threshold,
                 float held_tol, int min_len, int32_t* runs, int max_runs, int32_t* n_runs, float* threshold_out, si_stream_t stream);

/* ---- Dropouts by windowed RMS level ------------------------------------------------------------------------------------
 * The reference has no detection: the script's user types the one mask into predict.yaml (I_ea/predict.py:85-90).  si_quiet_runs and
 * si_dead_runs judge a dropout sample by sample; a dropout that is a NOISE FLOOR -- dither, comfort noise from a codec's concealer, a
 * file re-encoded after the damage -- has peaks of about five sigma, where speech's own soft passages live, and one outlier splits
 * the run.  This call judges the RMS level of a window of 2 * half + 1 samples instead, with si_dead_runs' input, output and limits:
 * x is (n, channels) interleaved, fp32 or int16; channels = 1 is a mono file (channel 0 or -1) and gives the mono bytes.  For one
 * channel x[0 .. n) (elements k * channels + c), with h = half:
 *   peak, T   si_dead_runs': T = max(threshold, fl32(rel_threshold * peak)), the peak over the FINITE samples; with rel_threshold == 0
 *             the peak is not computed and T = threshold.
 *   sq(k)     (double)x[k] * (double)x[k], exact for every finite fp32 and every int16 (-32768 included).  bad(k): x[k] is NaN or +-inf.
 *   W(i)      [max(0, i - h), min(n - 1, i + h)], cnt(i) = |W(i)|: samples in front of the base and at or past n do not exist and are
 *             never read; a window at either end of the file is truncated, and so is its count.
 *   E(i)      the sum of sq(k) over k in W(i), in float64, BY ADDITIONS ONLY: no window is a difference of running sums (behind one
 *             3e38 sample such a difference is garbage, and one NaN would poison every window after it).  The order of the additions
 *             is the implementation's: E lies within cnt * 2^-52 * E of the exact sum, and is exact whenever every partial sum is
 *             representable -- always for int16 (E < 2^42), and for fp32 samples on a 2^-20 grid with |x| <= 1.
 *   low(i)    no bad sample lies in W(i), and E(i) <= lim(i) = fl64(((double)T * (double)T) * cnt(i)): the square exact, the product
 *             one rounding.  That is RMS(W(i)) <= T without a division or a root.
 *   dead(j)   low(i) for some i with |i - j| <= h and 0 <= i < n: the UNION of the low windows.  An exact-zero dropout [s, e) of at
 *             least 2 h + 1 samples in loud audio therefore comes back as exactly [s, e), not shrunk by h on each side.
 * channel >= 0 scans that channel: its window is elements k * channels + channel, never the adjacent elements, and the peak is taken
 * over that channel's elements.  channel = -1 is JOINT: a sample time is dead when EVERY channel's dead_c holds, each by its own
 * windows, against one T from the peak over all elements of the file.
 * Two consequences: with half = 0, low(i) <=> |x[i]| <= T exactly (both squares are exact) and the bytes are those of si_dead_runs(kind =
 * SI_DEAD_QUIET); a huge finite sample, 3e38 at position p, followed by zeros starts a run at exactly p + 1.
 * The result is si_quiet_runs': every maximal run of dead samples of at least min_len samples as int32 (start, len) rows sorted by
 * start, rows [0, min(total, max_runs)) written and the rows past them untouched, the total in n_runs (device int32 (1)); the same
 * input gives the same bytes (no atomics; plain stores).  threshold_out, when not NULL, is a device fp32 word that receives T.
 * Scratch is si_dead_runs'.  One workgroup stages 2048 + 4 * half squares in LDS (139 264 bytes at SI_LEVEL_MAX_HALF).
 * SI_EINVAL before any launch, naming the argument, for: everything si_dead_runs refuses for the arguments they share (x, n, channels,
 * channel, threshold negative or NaN, rel_threshold NaN or outside [0, 1], min_len, runs, max_runs, n_runs); half outside 0 ..
 * SI_LEVEL_MAX_HALF; a threshold that is not finite. */
#define SI_LEVEL_MAX_HALF 1024
int si_level_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int half, float threshold, float rel_threshold,
                  int min_len, int32_t* runs, int max_runs, int32_t* n_runs, float* threshold_out, si_stream_t stream);

/* ---- Corrupted blocks by second-difference level ---------------------------------------------------------------------
 * The reference has no detection (I_ea/predict.py:85-90).  si_quiet_runs, si_dead_runs and si_level_runs find damage that is QUIETER
 * than the speech around it.  A block of corrupted PCM -- a sector of random data, byte-swapped or byte-misaligned samples, a burst of
 * bit errors in the high bytes -- is louder: white noise at full scale.  This call judges the level of the SECOND DIFFERENCE over a
 * window of 2 * half + 1 centres, a high-pass under which such a block has an RMS of sqrt(2) of full scale and speech stays below
 * full scale.  Arguments, input layout, output rows, scratch and limits are si_level_runs'.  For one channel x[0 .. n) (elements
 * k * channels + c), with h = half:
 *   peak, T   si_dead_runs': T = max(threshold, fl32(rel_threshold * peak)); with rel_threshold == 0 the peak is not computed.
 *   d(k)      for 1 <= k <= n - 2 ONLY: nothing in front of the base or at or past n is read.
 *             int16, packed 24-bit: d = x[k - 1] - 2 x[k] + x[k + 1] in int32 from the integer sample values (|d| <= 131 070 for int16,
 *             < 2^26 for 24-bit: no wrap), sq(k) = (double)d * (double)d, exact (below 2^34 / 2^52).  24-bit thresholds count 24-bit steps.
 *             fp32: D = fl64(fl64((double)x[k - 1] + (double)x[k + 1]) - 2 * (double)x[k]), sq(k) = fl64(D * D): two roundings and one,
 *             in this order, and NO contraction into a fused multiply-add anywhere in it.
 *   bad(k)    any of x[k - 1], x[k], x[k + 1] is NaN or +-inf; its square counts as 0.  Counted with integers.
 *   W(i)      [max(1, i - h), min(n - 2, i + h)], cnt(i) = |W(i)|, which may be 0 (i = 0 or n - 1 with h = 0; every i when n < 3).
 *   E(i)      the sum of sq(k) over k in W(i), in float64, BY ADDITIONS ONLY (si_level_runs' rule and bound: within cnt * 2^-52 * E of
 *             the exact sum).  Exact for int16 (E < 2^46), and for fp32 samples on a 2^-20 grid with |x| <= 1.
 *   hot(i)    cnt(i) >= 1, no bad centre lies in W(i), and E(i) >= lim(i) = fl64(((double)T * (double)T) * cnt(i)).
 *   dead(j)   hot(i) for some i with |i - j| <= h and 0 <= i < n: the union of the hot windows.
 * channel >= 0 scans that channel: its neighbours are elements (k +- 1) * channels + channel, never the adjacent elements.  channel = -1
 * is JOINT: a sample time is dead when every channel's dead_c holds, against one T.
 * Consequences: with half = 0, hot(i) <=> |d(i)| >= T for 1 <= i <= n - 2; n < 3 gives zero runs; a window that holds a non-finite
 * sample is never hot (a float file whose damage IS non-finite samples is not this call's).  With threshold = 0 and rel_threshold = 0
 * every window with a centre is hot.
 * The result is si_quiet_runs': sorted int32 (start, len) rows, rows [0, min(total, max_runs)) written, the total in n_runs, T in
 * threshold_out when not NULL; the same input gives the same bytes (no atomics; plain stores).
 * SI_EINVAL before any launch, naming the argument, for everything si_level_runs refuses, except that rel_threshold must lie in
 * [0, 4] (|d| <= 4 * peak) and not be NaN. */
int si_burst_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int half, float threshold, float rel_threshold,
                  int min_len, int32_t* runs, int max_runs, int32_t* n_runs, float* threshold_out, si_stream_t stream);

/* ---- NaN, inf and out-of-range samples: found, and kept out of the interpolation -----------------------------------------
 * The reference has no detection (I_ea/predict.py:85-90) and its loads pass every sample value on (:79-80).  A float file whose damage is
 * the sample VALUES -- NaN, +-inf, 3e38 left by a division by zero, a decoder that ran off its buffer, a damaged sector -- is seen by
 * none of the detectors above (NaN is loud, never held, and a window that holds one is neither low nor hot), and one such sample inside
 * a hand-typed gap still poisons its whole context: the interpolating cutters run FIRs over the file, so NaN leaves the masked span.
 *
 * invalid(v, c), for a ceiling c > 0 (+inf allowed) -- ONE definition (csrc/common.h, si_invalid) shared by the four calls below:
 *   fp32            !(|v| <= min(c, FLT_MAX)): NaN of any payload and sign, +-inf, and |v| > c.  With c = +inf exactly "not finite".
 *                   -0.0 and subnormals are valid.
 *   int16           !((float)|v| <= c), the magnitude taken in int32 (|-32768| = 32768, exact); c counts the file's own steps.
 *   packed 24-bit   the same with 24-bit steps (|-2^23| exact).  A PCM sample is invalid only under a finite ceiling: c = 32766 marks
 *                   clipped int16 samples.
 *
 * si_invalid_runs: every maximal run of invalid samples of at least min_len samples.  Input layout, channels / channel (channels = 1 is
 * a mono file and gives the mono bytes; channel = -1 is JOINT: a time is dead when EVERY channel's element is invalid), output rows,
 * scratch, limits and refusals are si_dead_runs' for the arguments they share.  There is no pass 0: no peak, no threshold_out.  A sample
 * at or past n, or in front of the base, is never read as dead.  Plain stores, no atomics: the same input gives the same bytes.
 * SI_EINVAL before any launch, naming the argument, for everything si_dead_runs refuses for the shared arguments, and a ceiling that is
 * <= 0 or NaN.
 *
 * si_cut_rate_valid / si_cut_pair_valid / si_cut_clips_valid: the contract of si_cut_rate[_ch] / si_cut_pair[_ch] / si_cut_clips, with
 * one more sentence: A FILE SAMPLE THAT IS invalid(., ceiling) IS STAGED AS +0.0 (judged in the file's own units, before the conversion
 * to full scale).  Wings, tap counts, fma order, the single rounding and the unfiltered 16 kHz row of a 16 kHz file are untouched, so
 * the outputs equal, byte for byte, the plain call's on the file with its invalid samples replaced by +0.0 -- without that copy of the
 * file.  channels = 1 is the mono file; channels >= 2 reads channel `channel` of the interleaved file (si_dead_runs' convention: one
 * call, not two).  si_cut_clips_valid is fp32, the 22.05 kHz route.  SI_EINVAL before any launch for everything the mirrored call
 * refuses, channels outside 1 .. SI_MAX_CHANNELS, channel outside [0, channels), and a ceiling that is <= 0 or NaN. */
int si_invalid_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, float ceiling, int min_len, int32_t* runs,
                    int max_runs, int32_t* n_runs, si_stream_t stream);
int si_cut_rate_valid(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_start,
                      const int32_t* start, int C, int L, const si_sinc_filter* filt, float ceiling, float* out, si_stream_t stream);
int si_cut_pair_valid(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_frame,
                      const int32_t* frame, int C, int L22, int L16, const si_sinc_filter* filt22, const si_sinc_filter* filt16, float ceiling,
                      float* out22, float* out16, si_stream_t stream);
int si_cut_clips_valid(si_ctx* ctx, const float* src, int n_src, const int32_t* host_start, const int32_t* start, int C, int L, float ceiling,
                       float* out, si_stream_t stream);

/* ---- Clicks and pops by locally scaled AR prediction error -----------------------------------------------------------
 * The reference has no detection (I_ea/predict.py:85-90).  The five detectors above find damage that is quieter than the speech, blocks
 * that are louder, and bad values; a click of one to a few IN-RANGE samples -- a bit error in a high byte, a dropped or repeated sample
 * at a buffer seam, a contact click -- is seen by none of them.  si_impulse_runs whitens the signal with a short-time AR model (speech
 * onsets, sibilants and glottal pulses are largely predictable; a click is not) and compares each sample's squared prediction error
 * with the mean squared prediction error of its own neighbourhood (Vaseghi & Rayner; Godsill & Rayner ch. 5).  Input layout, sample
 * types, channels / channel, output rows, scratch and limits are si_level_runs'.  For one channel x[0 .. n) (elements k * channels + c),
 * values taken as the file's own numbers in float64 (the fp32 value, the PCM integer in its type's steps), with p = order, h = half,
 * g = guard, B = 512:
 *   peak, T   si_dead_runs': T = max(threshold, fl32(rel_threshold * peak)); with rel_threshold == 0 the peak is not computed.  T = 0
 *             is allowed: the ratio test remains.
 *   blocks    block b is [b B, min(n, (b + 1) B)); its fit window F_b = [max(0, b B - 256), min(n, (b + 1) B + 256)).
 *   model     r[k] = the sum of w[t] * w[t + k] over t, t + k in F_b, k = 0 .. p, IN THIS ORDER: eight partial sums, partial q over
 *             t = q, q + 8, q + 16, ... counted from F_b's first sample, each in index order starting from +0.0, then ((q0 + q1) + q2)
 *             + ... + q7.  r[0] <- r[0] * (1 + 1e-9).  Levinson-Durbin, i = 1 .. p: a_0 = 1, E = r[0], kappa = -(r[i] + sum_{j=1}^{i-1}
 *             a_j r[i - j]) / E (the sum in the order j = 1, 2, ...), a_j <- a_j + kappa * a_{i-j}, a_i = kappa, E <- E * (1 - kappa^2).
 *             The model is a = (1, 0, ..., 0) when |F_b| <= p, r[0] == 0, or E <= 0 or non-finite at any step.
 *   bad       badblk(b): a NaN or +-inf lies in F_b (counted with integers); then every t of the block is bad.
 *   e(t)      for p <= t < n: a_0 * x[t] + a_1 * x[t - 1] + ... + a_p * x[t - p] with block(t)'s model, added in this order, float64, every
 *             product and sum rounded on its own (no fused multiply-add).  x[t - j] in front of the block are the file's samples.
 *             sq(t) = fl64(e * e).  t < p has no residual: it is never hot and lies in no window.
 *   L(t), R(t)  [max(p, t - h), t - g - 1] and [t + g + 1, min(n - 1, t + h)], either may be empty; cnt(t) = |L| + |R|;
 *             S(t) = the sum of sq over both, in float64 BY ADDITIONS ONLY (si_level_runs' rule; within cnt * 2^-52 * S of the exact sum).
 *   hot(t)    t >= p; cnt(t) >= h - g; no bad sample is t or lies in L(t) or R(t); sq(t) > fl64((double)T * (double)T);
 *             fl64(sq(t) * cnt(t)) > fl64(fl64((double)ratio * (double)ratio) * S(t)).  There is no division: a non-zero residual over an
 *             all-zero neighbourhood (a click in digital silence) is hot, a zero residual never is.
 *   dead(j)   hot(t) for some t with |t - j| <= pad and 0 <= t < n.
 * channel >= 0 scans that channel (elements k * channels + channel, never the adjacent ones); channel = -1 is JOINT: a sample time is
 * dead when EVERY channel's dead_c holds, against one T from the peak over all elements.  n <= p gives zero runs.
 * The result is si_quiet_runs': sorted int32 (start, len) rows, rows [0, min(total, max_runs)) written, the total in n_runs, T in
 * threshold_out when not NULL; plain stores, no atomics: the same input gives the same bytes.  Scratch is si_dead_runs'.  One workgroup
 * holds its samples, residuals and window sums as float64 in LDS (135 168 bytes at half + pad = SI_IMPULSE_MAX_HALF).
 * SI_EINVAL before any launch, naming the argument, for: everything si_level_runs refuses for the arguments they share; order outside
 * 2 .. SI_IMPULSE_MAX_ORDER; guard outside 0 .. SI_IMPULSE_MAX_GUARD; half outside guard + 1 .. SI_IMPULSE_MAX_HALF; pad outside
 * 0 .. SI_IMPULSE_MAX_PAD; half + pad above SI_IMPULSE_MAX_HALF; ratio NaN or outside [1, 1e6]; rel_threshold NaN or outside [0, 4].
 *
 * si_impulse_residual: e(t) itself, the whitened signal of ONE channel (0 <= channel < channels; channels = 1 is a mono file), through
 * the same device functions as the detector: e[t] for t in [0, n) as device float64 -- 0.0 for t < p, NaN for a bad sample.  No
 * scratch.  SI_EINVAL for channels / channel out of range, NULL x or e, n outside 1 .. 2^31 - 2049, order outside 2 .. 32. */
#define SI_IMPULSE_MAX_ORDER 32
#define SI_IMPULSE_MAX_HALF 1024
#define SI_IMPULSE_MAX_GUARD 64
#define SI_IMPULSE_MAX_PAD 16
int si_impulse_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int order, int half, int guard, int pad,
                    float ratio, float threshold, float rel_threshold, int min_len, int32_t* runs, int max_runs, int32_t* n_runs,
                    float* threshold_out, si_stream_t stream);
int si_impulse_residual(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int order, double* e, si_stream_t stream);

/* ---- Short damaged runs mended in place by least-squares AR interpolation ------------------------------------------
 * The detectors find a single NaN or a 3-sample underrun exactly; regenerating a 20 ms frame for it replaces good speech.  si_mend_runs
 * fills the runs of at most max_len samples from their own neighbourhood instead (Janssen; Godsill & Rayner): an AR model of order p
 * fitted to K intact samples on either side, then the missing samples that minimise its prediction error.  Nothing the reference
 * computes: it has no detection and no repair but the model                                             I_ea/predict.py:85-90
 *
 * x: the caller's copy of the file on the device, repaired IN PLACE: n sample times of fp32, int16 or packed 24-bit PCM by is_pcm16
 * (SI_SAMPLE_*; an s24 view may start at any byte), one channel (channels = 1) or channel `channel` of `channels` interleaved (element
 * offsets are 64-bit).  runs: device int32 (n_runs, 2) rows (start, len), sorted and disjoint, as the five detectors emit them.
 * status: device int32 (n_runs), one word per row -- the first of these that applies, with p = order, K = context, s = start, m = len,
 * e = s + m:
 *   SI_MEND_BADROW 6     s < 0, m < 1 or e > n: no sample read, none written
 *   SI_MEND_LONG 0       m > max_len: left for the inpainter
 *   SI_MEND_EDGE 3       s - K < 0 or e + K > n
 *   SI_MEND_NEAR 4       another row meets [s - K, e + K): row i - 1 ends past s - K, or row i + 1 starts before e + K
 *   SI_MEND_NONFINITE 5  a non-finite sample among the 2 K context samples, or a non-finite result
 *   SI_MEND_AR 1         filled by the model
 *   SI_MEND_LINE 2       model degenerate: u_i = x[s - 1] + (i + 1) / (m + 1) * (x[e] - x[s - 1]) in float64
 * The model, in float64 on the file's own values (the fp32 value, the PCM integer), w = x[s - K .. e + K), W = 2 K + m:
 *   r[k] = sum w[t] w[t + k] over the pairs that lie on ONE side of the gap (k = 0 .. p), then r[0] *= 1 + 1e-9; r[0] == 0: LINE
 *   Levinson-Durbin for a_0 = 1, a_1 .. a_p with E <- E (1 - kappa^2); E <= 0 or not finite at any step: LINE
 *   b[k] = sum_j a_j a_{j + k};  B_ij = b[|i - j|] (0 past p);  d_i = -sum over the KNOWN t within p of K + i of b[|t - K - i|] w[t]
 *   B u = d by Cholesky; a pivot <= 0: LINE.  u minimises sum_{t = K}^{K + m - 1 + p} (sum_j a_j w[t - j])^2.
 * fp32 stores (float) u; int16 and s24 store rint(u), ties to even, clamped to the type's range, as the sample's own 2 or 3 bytes.
 * Only AR and LINE write, only [s, e) of that channel, and nothing before the whole solve has succeeded; NEAR keeps every row's reads
 * clear of every other row's writes, so a row alone gives the bytes of the same row inside a table.  No atomics, fixed summation
 * orders: the same input gives the same bits.  One workgroup per row, no scratch; profiled in the family "patch_rate".
 * SI_EINVAL before any launch, naming the argument: channels outside 1 .. SI_MAX_CHANNELS, channel outside [0, channels), NULL x, n
 * outside 1 .. 2^31 - 2049, n_runs outside 0 .. SI_MEND_MAX_RUNS, NULL runs or status with n_runs > 0, max_len outside
 * 1 .. SI_MEND_MAX_LEN, order outside 2 .. SI_MEND_MAX_ORDER, context outside 4 * order .. SI_MEND_MAX_CONTEXT.  n_runs = 0 launches
 * nothing. */
#define SI_MEND_MAX_LEN 64
#define SI_MEND_MAX_ORDER 32
#define SI_MEND_MAX_CONTEXT 1024
#define SI_MEND_MAX_RUNS 65536
#define SI_MEND_LONG 0
#define SI_MEND_AR 1
#define SI_MEND_LINE 2
#define SI_MEND_EDGE 3
#define SI_MEND_NEAR 4
#define SI_MEND_NONFINITE 5
#define SI_MEND_BADROW 6
int si_mend_runs(si_ctx* ctx, void* x, int is_pcm16, int n, int channels, int channel, const int32_t* runs, int n_runs, int max_len,
                 int order, int context, int32_t* status, si_stream_t stream);

/* Shape helpers (host arithmetic only). */
int si_num_frames(const si_ctx* ctx, int N);            /* encoder frames T for N samples, <0 on error */
int si_vocoder_samples(const si_ctx* ctx, int Tm, int stretch);   /* output samples per clip */

/* Per-kernel timing.  Between si_profile_start and si_profile_stop every kernel launch of this context is
 * bracketed by two HIP events recorded on the launch stream.  si_profile_stop waits for those events and returns
 * one entry per kernel family: launches, summed device milliseconds, summed ALGORITHMIC flops and bytes (layer
 * shapes only: no padding, halo or recompute).  max_launches bounds the event pool; launches beyond it are not
 * recorded.  This is what bench.py's `roofline` object is computed from.  si_profile_filter restricts the bracketing
 * to ONE family (its entry name; NULL or "" = all): an event pair costs ~4 us of stream time, 6 % of a step when every
 * launch carries one, so bench.py times its K steps with only the dominant family bracketed. */
typedef struct si_profile_entry {
    char name[48];
    int32_t launches;
    int32_t reserved;
    double ms;
    double flops;
    double bytes;
} si_profile_entry;
int si_profile_start(si_ctx* ctx, int max_launches);
int si_profile_filter(si_ctx* ctx, const char* family);
int si_profile_stop(si_ctx* ctx, si_profile_entry* out, int capacity, int* count);

/* Test hook.  Intermediates are named "features", "projected", "encoder_in", "last_hidden" (encoder) and
 * "ups<i>", "stage<i>" (vocoder with an fp32 residual stream; of the last chunk of clips).  si_debug_capture registers a device buffer that
 * the NEXT forwards copy the named tensor into at the moment it is produced (workspace buffers are recycled
 * within a forward); dst = NULL unregisters.  si_debug_size returns the tensor's element count in the last forward.
 * Per-op taps of the encoder, each the tensor exactly as stored (a name ending in ".bf16" holds raw bf16 values,
 * 2 bytes each, and its capacity counts bf16 elements; every other capacity counts floats):
 *   conv0 / conv0.bf16        conv0 (+ GroupNorm + GELU in the group flavour), (B, L1, C0)
 *   conv0.ln / conv0.ln.bf16  layer flavour: LayerNorm + GELU behind conv0
 *   conv<i> / conv<i>.bf16    strided conv i (+ GELU in the group flavour), (B, L_{i+1}, C_i); ragged: rows past a clip are stale
 *   conv<i>.ln[.bf16]         layer flavour: LayerNorm + GELU behind conv i
 *   features.ln[.bf16]        the feature projection's LayerNorm rows, (rows, C_last), directly behind it: fp32, or in bf16 mode with
 *                             operand-ready activations the bf16 operand only (the form the projection GEMM reads); absent
 *                             without feat_proj_layer_norm
 *   pos_conv                  h + GELU(pos_conv(h) + b), (rows, H) fp32, directly behind the positional conv (posconv.hip or the
 *                             tap-GEMM) and before the encoder LayerNorm; h is "projected" with the padded frames zeroed
 *   layer<l>.h                the fp32 hidden state entering layer l (out-proj's residual)
 *   layer<l>.h.bf16           the QKV GEMM's bf16 operand
 *   layer<l>.qkv[.bf16]       q | k | v, (rows, 3H)
 *   layer<l>.att[.bf16]       attention output, (rows, H)
 *   layer<l>.att_res          out-proj + residual
 *   layer<l>.ln1[.bf16]       LayerNorm rows / its bf16 operand (pre-LN, bf16 mode: the operand only)
 *   layer<l>.ffn[.bf16]       GELU(FFN1), (rows, I) (the bf16 form without its row padding)
 *   layer<l>.ffn_res          FFN2 + residual
 *   layer<l>.ln2[.bf16]       as ln1
 * These are produced only while some capture is registered (they then also appear in si_debug_size); registering any
 * capture runs the post-LN layers with every LayerNorm writing its rows (SI_ENC_LNFUSE's unfused path).
 * Taps of the vocoder's fp16 activation stream (fp16 mode with SI_VOC_RES16, where "ups<i>" / "stage<i>" do not exist), of
 * the last chunk of clips: names ending in ".f16" hold the raw fp16 tensor exactly as stored, 2 bytes per element, capacity
 * counted in fp16 elements.  Ragged batches: rows past a clip's own end are stale.
 *   pre.f16                      conv_pre's output, (B, Tout, C0)
 *   ups<i>.f16                   upsampler i's output, (B, Lo, C_i), from upsample.hip, gemmcu.hip's TC kernels or the tap-GEMM
 *   stage<i>.rb<j>.p<n>.f16      output of pair n of resblock j (ResBlock2: of conv n): the block's own stream for n < last, the
 *                                running MRF sum (blocks 0 .. j, each scaled by 1 / num_kernels) for the last n.  A resblock that
 *                                runs as one reschain.hip launch has only the last one.
 *   stage<i>.f16                 the completed MRF mean, as the next consumer reads it
 * Like the encoder's these are named and looked up only while some capture is registered; unlike the encoder's they are
 * copies behind the launch that produced the tensor and change neither which kernel runs nor any value.
 * Stored activated: the producer of an upsampler that runs in gemmcu.hip's TC kernels (profile family "gemmcu_f16_*":
 * N = u * Cout a multiple of 256, k = 2 u, unless SI_VOC_UPSGEMM=0) stores leaky_relu(x, 0.1) of its fp32 value instead of x.
 * That producer's tensor is "pre.f16" for upsampler 0 and "stage<i-1>.f16" (= the last "stage<i-1>.rb<j>.p<n>.f16") for upsampler i;
 * no other tap is activated, and with SI_VOC_UPSGEMM=0 none is.
 * Taps of the vocoder's fp32 residual stream (fp32, bf16x3, bf16, and fp16 with SI_VOC_RES16=0; of the last chunk of clips), next to
 * "ups<i>" / "stage<i>": fp32 tensors, capacities in floats, under the same rule -- copies behind the producing launch, named and
 * looked up only while some capture is registered, changing no launch and no value.  Ragged batches: rows past a clip's own end are stale.
 *   pre                          conv_pre's output, (B, Tout, C0)
 *   stage<i>.rb<j>.t<n>          the intermediate of pair n of resblock j: conv 1's output before conv 2's leaky-ReLU, (B, Lo, C_i).
 *   stage<i>.rb<j>.t<n>.bf16     The operand-ready modes store it only as conv 2's 16-bit operand, type16(leaky_relu(t, 0.1)): the raw
 *   stage<i>.rb<j>.t<n>.f16      tensor, 2 bytes per element (bf16 mode / fp16 mode with SI_VOC_RES16=0).  ResBlock2 has no intermediate.
 *   stage<i>.rb<j>.p<n>          as its ".f16" namesake: the block's own stream for n < last, the running MRF sum for the last n
 * Taps of the mel front-end (si_mel_frontend and its _varlen / _spans forms), under the same rule: fp32 copies behind the producing
 * launch, changing no launch and no value.  "mel_frames" is sized on every call; the other two only while some capture is registered.
 *   mel_peak                     max |x| of each clip with its spans zeroed, (B); only with normalize != 0
 *   mel_frames                   the windowed frames as the DFT GEMMs read them, folded: (B, Tm, 1040) =
 *                                [s_0 .. s_512 | 15 zeros | 0, d_1 .. d_511], s_k = w[k] + w[1024 - k], d_k = w[k] - w[1024 - k]
 *                                (s_0 = w[0], s_512 = w[512]).  Ragged batches: frames past a clip's own are not written (stale).
 *   mel_spec                     the DFT, (B, Tm, 1032) = [re(0..512) | 3 pad | im(0..512) | 3 pad]; the pad columns (513..515,
 *                                1029..1031) hold whatever the workspace held, and so do the rows of frames past a ragged clip's own */
int si_debug_capture(si_ctx* ctx, const char* name, float* dst, long capacity);
long si_debug_size(si_ctx* ctx, const char* name);

/* Test hook: where a pass writes.  The encoder, the generator and the mel front-end carve their caller-owned workspace into named
 * regions, in order, at 256-aligned offsets.  si_debug_ws_regions returns the regions of that pass's most recent call on this context
 * (`which`: SI_WS_ENCODER, SI_WS_VOCODER, SI_WS_MEL): name, offset from the workspace pointer of that call, and the bytes the pass
 * asked for -- the only bytes of the workspace it may write.  *count receives the number of regions (at most SI_WS_MAX_REGIONS; 0
 * before the first call), of which the first min(count, capacity) are stored.  Host bookkeeping only: no allocation, no device work.
 * SI_WS_REDZONE=<bytes> in the environment of si_create (a test switch; rounded down to a multiple of 256, at most 1 MiB, default 0)
 * makes the carve leave that many bytes in front of the first region and behind every region, the last included; the library never
 * writes them, and si_workspace_bytes / si_mel_workspace_bytes grow by that size times a fixed count per pass.  Unset, every offset
 * and every size is what it is without the switch.  A test fills the workspace, runs the pass and finds every byte outside
 * [offset, offset + bytes) of the regions as it left it. */
#define SI_WS_ENCODER 0
#define SI_WS_VOCODER 1
#define SI_WS_MEL 2
#define SI_WS_MAX_REGIONS 32
typedef struct si_ws_region {
    char name[24];
    uint64_t offset;
    uint64_t bytes;
} si_ws_region;
int si_debug_ws_regions(si_ctx* ctx, int which, si_ws_region* out, int capacity, int* count);

#ifdef __cplusplus
}
#endif
#endif /* SI_HIP_H */
