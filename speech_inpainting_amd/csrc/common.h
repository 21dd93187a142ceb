// Internal declarations shared by the HIP translation units of libsi_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/si_hip.h"
#include "weights_host.h"

#define SI_HIP_CHECK(expr)                                                                      \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) return si_fail_hip(ctx, _e, #expr, __FILE__, __LINE__);           \
    } while (0)

int si_fail_hip(si_ctx* ctx, hipError_t e, const char* what, const char* file, int line);
int si_fail(si_ctx* ctx, int code, const char* fmt, ...);
// HIP-event bracket around one kernel launch (no-op unless si_profile_start armed the context)
void si_prof_begin(si_ctx* ctx, const char* name, double flops, double bytes, hipStream_t st);
void si_prof_end(si_ctx* ctx, hipStream_t st);
// Diagnostic (SI_PROF_SHAPES=1 in the environment): the family name with the GEMM shape appended, so that a per-kernel table
// separates the launches of one instantiation; otherwise `name` itself.  The returned pointer is valid until the next call.
const char* si_prof_shape_name(const char* name, long M, int N, int K);
// Raise a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) when a launch needs more than the
// 64 KB default.  The high-water mark is kept per context (= per device): a process-wide cache would skip the call
// for a second context on another GPU.
int si_ensure_dyn_lds(si_ctx* ctx, const void* kern, size_t bytes);
int si_num_cus(si_ctx* ctx);   // compute units of the context's device (persistent-kernel grids)

typedef unsigned short bf16_t;   // raw bf16 bits

// ------------------------------------------------------------------------------------------------
// The sample types of the file-typed calls.  SiS24 is one packed little-endian signed 24-bit PCM sample as a WAV
// data chunk holds it: three bytes of alignment 1, so `const SiS24* x` indexes samples, x[i] touches exactly bytes [3 i, 3 i + 3) and a
// view may start at any byte.  value() is exact in fp32, and so is value() * 2^-23.
// ------------------------------------------------------------------------------------------------
struct SiS24 {
    uint8_t b[3];
    SiS24() = default;
    __host__ __device__ explicit SiS24(int v) : b{(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16)} {}
    __host__ __device__ int value() const { return (int)((unsigned)b[0] << 8 | (unsigned)b[1] << 16 | (unsigned)b[2] << 24) >> 8; }
};
static_assert(sizeof(SiS24) == 3 && alignof(SiS24) == 1, "SiS24 is three packed bytes");

// The C ABI's is_pcm16 argument as one of SI_SAMPLE_F32 / _S16 / _S24: 2 is s24, every other non-zero value int16 as it always was.
inline int si_sample_format(int is_pcm16) { return is_pcm16 == SI_SAMPLE_S24 ? SI_SAMPLE_S24 : is_pcm16 != 0 ? SI_SAMPLE_S16 : SI_SAMPLE_F32; }
inline double si_sample_bytes(int fmt) { return fmt == SI_SAMPLE_S24 ? 3.0 : fmt == SI_SAMPLE_S16 ? 2.0 : 4.0; }
// f(null pointer of the sample type fmt names): the launchers pick their instantiation through its type.
template <class F>
inline void si_with_sample(int fmt, F&& f) {
    if (fmt == SI_SAMPLE_S24) f(static_cast<const SiS24*>(nullptr));
    else if (fmt == SI_SAMPLE_S16) f(static_cast<const int16_t*>(nullptr));
    else f(static_cast<const float*>(nullptr));
}
// f(std::true_type or std::false_type): the same for a kernel's compile-time switch, read as decltype(flag)::value.
template <class F>
inline void si_with_flag(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// invalid(v, c) for a ceiling c > 0 (+inf allowed): the ONE definition that si_invalid_runs and the three _valid feeds
// share.  fp32: NaN of any payload and sign, +-inf and |v| > c; with c = +inf exactly "not finite"; -0.0 and subnormals are valid.
// PCM: |v| > c with the magnitude taken in int32 (32768 / 2^23 exact in fp32) and c counting the file's own steps, so a PCM sample is
// invalid only under a finite ceiling.
__device__ __forceinline__ bool si_invalid(float v, float c) { return !(__builtin_fabsf(v) <= __builtin_fminf(c, __FLT_MAX__)); }
__device__ __forceinline__ bool si_invalid(int16_t v, float c) { const int a = v; return !((float)(a < 0 ? -a : a) <= c); }
__device__ __forceinline__ bool si_invalid(SiS24 v, float c) { const int a = v.value(); return !((float)(a < 0 ? -a : a) <= c); }

// ------------------------------------------------------------------------------------------------
// Ragged batches (BASELINE configs[4]: clips of different lengths in ONE launch, each clip's result equal to that clip run
// alone -- the reference's one-file-per-run script, I_ea/predict.py:76-207).  Storage keeps a fixed stride per clip (the
// longest clip's); a device int32 array holds every clip's own row count, and the persistent kernels number their tiles clip
// by clip WITHOUT gaps: tile t -> (clip, first row, the clip's rows).  `t` is wave-uniform; every lane gets the result.
// One vector load, a 6-step wave scan and a ballot per call (per tile of tens of microseconds).
// ------------------------------------------------------------------------------------------------
struct SiVlTile { int b, row0, L; };
#ifdef __HIPCC__
__device__ __forceinline__ SiVlTile si_vl_tile(const int32_t* __restrict__ lens, int B, int step, int t) {
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    int base = 0;
    for (int s0 = 0; s0 < B; s0 += 64) {
        const int s = s0 + lane;
        const int Lb = s < B ? lens[s] : 0;
        const int nb = Lb > 0 ? (Lb + step - 1) / step : 0;
        int incl = nb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const int tot = __shfl(incl, 63, 64);
        if (t < base + tot) {                                          // wave-uniform
            const unsigned long long m = __ballot(base + incl > t);
            const int l = (int)__builtin_ctzll(m);
            SiVlTile r;
            r.b = s0 + l;
            r.row0 = (t - base - __shfl(incl - nb, l, 64)) * step;
            r.L = __shfl(Lb, l, 64);
            return r;
        }
        base += tot;
    }
    return SiVlTile{B, 0, 0};                                          // t past the last tile
}
#endif
// the same count on the host: tiles of `step` rows over clips of lens[b] rows
static inline long si_vl_tiles(const int32_t* lens, int B, int step) {
    long n = 0;
    for (int b = 0; b < B; ++b) if (lens[b] > 0) n += (lens[b] + step - 1) / step;
    return n;
}

// ------------------------------------------------------------------------------------------------
// "Tap GEMM": every contraction of the path (Conv1d with stride/dilation/groups, ConvTranspose1d split
// into stride phases, Linear) is
//     out[seg][m][n] = epi( sum_tap sum_ci  pro(x[seg][m*stride + tap*dil - pad][g*Cin + ci]) * W[g][tap][n][ci] )
// on channels-last activations, i.e. a GEMM whose A operand is a shifted view of the activation matrix.
// ------------------------------------------------------------------------------------------------
enum { SI_ACT_NONE = 0, SI_ACT_GELU = 1 };

struct TapGemmParams {
    const float* x;        // [nseg][Lin][ldx] fp32, channels-last (NULL when x16 is given)
    const unsigned short* x16;  // same geometry, 16-bit in the math mode's operand type; pro_slope (if != 1) is applied to it while staging
    const void* w;         // [groups][ntaps][Npad][Cin]  (fp32, or bf16 hi plane)
    const void* w_lo;      // bf16x3: lo plane, same layout
    const float* bias;     // [groups*N] or nullptr
    const float* res;      // residual, indexed like out, or nullptr
    // res_stats != NULL: the residual is LayerNorm(res) -- res holds the rows BEFORE the normalisation, res_stats (mean, rstd) per row,
    // res_gamma / res_beta its affine pair (the normalised rows were written as a bf16 GEMM operand only); bf16 GEMM kernels only
    const float* res_stats; const float* res_gamma; const float* res_beta;
    const unsigned short* res16;  // residual as raw 16-bit values of the math mode's type (instead of res)
    int acc16;             // accumulate reads the previous value from out16 (raw 16-bit) instead of out
    float* out;            // fp32 output (may be NULL when only out16 is wanted)
    unsigned short* out16; // optional operand-ready copy for the consumer: type16(leaky_relu(v, out16_slope)), indexed like out
    float out16_slope;     // the consumer's prologue slope (1 = identity)
    int nseg, Lin, M;      // segments (clips), input rows and output rows per segment
    int ldx;               // input row stride (floats)
    long x_seg_stride;     // floats between segments
    int Cin;               // input channels per group (multiple of BK)
    int N, Npad;           // output columns per group, padded row count of W
    int ntaps, stride, dil, pad;
    int groups;
    int ldo;               // output row stride (floats)
    long o_seg_stride;
    long ooff;             // flat offset added to m*ldo + n (ConvTranspose phase layout: -pad*Cout)
    long olimit;           // stores outside [0, olimit) of a segment are dropped
    float pro_slope;       // leaky-relu slope applied to x while staging (1 = identity)
    int act;               // SI_ACT_*
    float alpha;           // v = (acc + bias -> act -> + res) * alpha
    int accumulate;        // out = v + out
    double algo_macs;      // algorithmic multiply-accumulates of the layer (0: derive from the GEMM shape)
    int wide_epilogue;     // set by the launcher: row-contiguous 16-byte epilogue through an LDS transpose
    int lingemm;           // caller allows the dedicated bf16 GEMM kernel (lingemm.hip) when the shape fits it
    // ragged batches (all device int32 (nseg), all NULL for uniform segments): segment s reads seg_lin[s] input rows (instead
    // of Lin: rows outside read as zero -- the convolution's padding at the clip's OWN end), computes seg_m[s] output rows
    // (instead of M: tiles past them exit at once) and stores inside [0, seg_orows[s] * olim_mul) (instead of olimit).
    // seg_row_off: PACKED rows -- segment s starts at row seg_row_off[s] of x (row stride ldx) and of out / res / out16
    // (row stride ldo) instead of at s * x_seg_stride / s * o_seg_stride.
    const int32_t* seg_lin;
    const int32_t* seg_m;
    const int32_t* seg_orows;
    int olim_mul;
    const int32_t* seg_row_off;
    const int32_t* seg_m_host;   // host copy of seg_m (grid sizing of the kernels that walk tiles without gaps)
};

// N-tile width the launcher uses for a given N; the packer pads W rows to a multiple of it.
// si_pick_bn / si_round_up: weights_host.h (the layout plan pads N with them on the host)

int si_launch_tapgemm(si_ctx* ctx, int math, const TapGemmParams& p, hipStream_t st);

// The encoder's bf16 GEMM (lingemm.hip): out[seg][m][n] = epi(sum_k A[seg][m][k] W[n][k] + bias[n]); A row m = K
// consecutive bf16 at x16 + seg * x_seg_stride + m * lda (lda < K: overlapping rows = a strided convolution on
// channels-last activations); W = ntaps blocks [N][Cin] (k = tap * Cin + ci).  Returns 1 when the shape is not covered.
struct LinGemmParams {
    const unsigned short* x16; int x_bytes;     // activations (bf16) and the size of their buffer in bytes
    int lda; long x_seg_stride;                 // elements between consecutive A rows / segments
    int nseg, M, K;
    const unsigned short* w; int w_bytes;
    int N, Cin, ntaps; long w_tap_stride;       // elements between tap blocks of W
    const float* bias; const float* res;        // res: fp32, indexed like out
    const float* res_stats; const float* res_gamma; const float* res_beta;   // see TapGemmParams
    float* out; unsigned short* out16;          // fp32 and / or bf16 output
    int ldo; long o_seg_stride;
    int act;
    int xcd_rows;                               // set by the launcher: > 0 = XCD-aware tile order over this many row blocks
    // ragged batches: segment s holds seg_m[s] output rows (device int32 (nseg); NULL: M for all); seg_m_host = the same on the host
    const int32_t* seg_m;
    const int32_t* seg_m_host;
    // gemmcu.hip's transposed-convolution mode (si_launch_gemmcu_tc; fp16 operands and output): tap t of row m reads input row
    // m + t * tc_dil of a segment of tc_rows_in rows (zeros outside), leaky-ReLU(tc_slope) on the input, output element (m, n) at
    // m * ldo + n + tc_ooff of its segment, dropped outside [0, tc_olimit)
    int tc_dil, tc_rows_in; float tc_slope; long tc_ooff, tc_olimit;
    const int32_t* tc_seg_lin; const int32_t* tc_seg_orows; int tc_olim_mul;   // ragged batches: segment s reads tc_seg_lin[s] rows, keeps [0, tc_seg_orows[s] * tc_olim_mul)
};
int si_launch_lingemm(si_ctx* ctx, const LinGemmParams& p, hipStream_t st);
// The same contract as ONE tile per CU and round (gemmcu.hip: 8 or 16 waves, tile shape per instantiation), for the shapes whose
// tiles fill whole rounds of the CUs; returns 1 otherwise.  Bit-identical to lingemm.hip.
int si_launch_gemmcu(si_ctx* ctx, const LinGemmParams& p, hipStream_t st);
// The generator's early upsamplers on the fp16 stream as the same kernel (TapGemmParams of a ConvTranspose1d in its two-tap form);
// SI_OK when launched, negative on error, 1 when the shape is not covered (the caller uses the tap-GEMM).
int si_launch_gemmcu_tc(si_ctx* ctx, const TapGemmParams& p, hipStream_t st, bool always = false);   // always: also where tiles are mostly padding
bool si_gemmcu_tc_covers(si_ctx* ctx, const TapGemmParams& p, bool always = false);                   // would the call above launch?
int si_opt_gemmcu(const si_ctx* ctx);       // SI_ENC_GEMMCU: 0 never, 1 by the shape rule (default), 2 whenever the shape allows, 10 + c: instantiation c

// ------------------------------------------------------------------------------------------------
// encoder kernels (encoder_kernels.hip)
// ------------------------------------------------------------------------------------------------
struct WaveNormParams {           // A0 + A1 (group-norm flavour)
    const float* wav;             // (B, N) raw
    const int32_t* mask_start;    // (B) or null
    const int32_t* mask_len;      // (B) or null
    int B, N, L1;                 // L1 = conv0 output length
    int C, K, S;                  // conv0 channels / kernel / stride
    int normalize;                // 0: wav is already zero-mean/unit-variance
    const int32_t* valid_len;     // (B) or null: samples of each right-padded clip that are real; the rest is padding
                                  // (statistics over the real samples only, padding reads as 0 AFTER the normalisation:
                                  // transformers/models/wav2vec2/feature_extraction_wav2vec2.py:88-91)
    float norm_eps;               // variance epsilon of the normalisation: 1e-7 (HF processor) / 1e-5 (F.layer_norm(x, x.shape),
                                  // I_da/src/hubert_feature_reader.py:53-54)
    const double* pre_add;        // (B) or null: value added to every sample BEFORE the zero mask, in fp64, rounded to fp32
                                  // once -- `(y + 1e-6) * mask` on the float64 clip (I_da/scripts/inpainting.py:187-192)
    const int32_t* seg_L1;        // (B) or null: ragged batches -- conv0 output rows of each clip's OWN length (with valid_len =
                                  // its samples): GroupNorm statistics over those rows only, rows past them are not written
};

// Multi-gap masks: a clip carries 0 .. SI_MAX_SPANS zeroed sample spans instead of the one of mask_start / mask_len.  CSR table in device
// memory: clip b owns entries [off[b], off[b + 1]) of start / len (samples), sorted by start and disjoint (si_span_table, checked on the
// host by the C ABI).  A launcher given a table runs the `_spans` sibling of its kernel (mask_start / mask_len of the params are then
// NULL); without one, today's kernel with today's arguments.
struct SiSpans { const int32_t* off; const int32_t* start; const int32_t* len; };

// The masked-or-not test of a thread whose sample index NEVER DECREASES between calls (the whole-clip passes wave_stats and wave_peak).
// The thread keeps the first span that does not end at or before its index in registers: a sample that stays inside or in front of
// that span costs the two compares of the single-span test; the table is read (two global loads) once per span the thread passes, and
// lanes that pass a span at different samples diverge for that step.  The streaming loops ask `clear` once per 16-byte load first, so
// outside the gaps -- nearly all of a clip -- a vector costs one compare and no walk.
struct SiSpanWalk {
    const int32_t* s; const int32_t* l;
    int k, n, cs, ce;
    __device__ __forceinline__ void load() {
        if (k < n) { cs = s[k]; ce = cs + l[k]; } else { cs = 0x7fffffff; ce = 0x7fffffff; }
    }
    __device__ __forceinline__ SiSpanWalk(const SiSpans& sp, int b) : s(sp.start), l(sp.len), k(sp.off[b]), n(sp.off[b + 1]) { load(); }
    __device__ __forceinline__ bool hit(int i) {
        while (i >= ce) { ++k; load(); }
        return i >= cs;
    }
    // true: none of the samples [i, i + cnt) is masked and the cursor needs no step (spans behind the cursor end at or before an earlier
    // index, the cursor's span and all later ones start at cs or after) -- the one compare a 16-byte load pays outside the gaps
    __device__ __forceinline__ bool clear(int i, int cnt) const { return i + cnt <= cs; }
};

int si_launch_wave_stats(si_ctx* ctx, const WaveNormParams& p, double* stats /*B*2: mean, rstd*/, hipStream_t st, const SiSpans* sp = nullptr);
// conv0 -> GroupNorm(C groups) -> GELU, channels-last out (B, L1, C)
int si_launch_conv0_groupnorm(si_ctx* ctx, const WaveNormParams& p, const double* stats, const float* w /*[C][K]*/,
                              const float* gamma, const float* beta, double* partials, float* affine, float* out,
                              hipStream_t st, unsigned short* out16 = nullptr /* write bf16 there INSTEAD of fp32 into out */,
                              const SiSpans* sp = nullptr);
// conv0 (+bias) only, channels-last out, for the layer-norm flavour (LN+GELU applied by si_launch_layernorm)
int si_launch_conv0_affine(si_ctx* ctx, const WaveNormParams& p, const double* stats, const float* w, const float* bias,
                           float* affine, float* out, hipStream_t st, const SiSpans* sp = nullptr);
size_t si_conv0_partials_bytes(int B, int N);

// y = LN(x [+ add]) * gamma + beta over the last dim C (rows x C), optional GELU afterwards
// y16 (optional): bf16 copy of y for a bf16 GEMM consumer; y may then be NULL (bf16 output only)
int si_launch_layernorm(si_ctx* ctx, const float* x, const float* add, const float* gamma, const float* beta, float* y,
                        long rows, int C, float eps, int gelu, hipStream_t st, unsigned short* y16 = nullptr, float* stats = nullptr);

// softmax(q k^T / sqrt(64)) v for head_dim 64; qkv (B, T, 3H) packed [q | k | v]; out (B, T, H)
// out16 (optional): write the result as bf16 there INSTEAD of fp32 into out
// bf16_products: with out16 given, run both products on bf16 MFMA (fp32 softmax); false keeps the exact-fp32 kernel
// valid_frames (B) or null: keys >= valid_frames[b] are padding and excluded for every query (modeling_hubert.py:250-251)
// row_off (B + 1, device) or null: ragged batches on PACKED rows -- clip b = rows [row_off[b], row_off[b + 1]); T is then the
// longest clip's frame count (grid sizing) and real_t2 = sum of T_b^2 (the algorithmic flop count)
int si_launch_attention(si_ctx* ctx, const float* qkv, float* out, int B, int T, int H, int heads, hipStream_t st,
                        unsigned short* out16 = nullptr, bool bf16_products = true, const int32_t* valid_frames = nullptr,
                        const int32_t* row_off = nullptr, double real_t2 = 0.0);
// bf16 encoder mode: q | k | v arrive as bf16 (B, T, 3H) from the QKV GEMM's epilogue; both products on bf16 MFMA
int si_launch_attention_bf16in(si_ctx* ctx, const unsigned short* qkv16, int B, int T, int H, int heads, hipStream_t st,
                               unsigned short* out16, const int32_t* valid_frames = nullptr, const int32_t* row_off = nullptr,
                               double real_t2 = 0.0);
// HuBERT's positional conv in the bf16 encoder mode (posconv.hip): out = x + gelu(conv(x) + b) on (rows, H) fp32, the group's weights
// streamed once per workgroup; returns 1 when the shape is not covered (the caller runs the tap-GEMM)
int si_launch_posconv(si_ctx* ctx, const float* x, float* out, const void* w, const float* bias, int B, int T, int Tmax, int H, int groups,
                      int ntaps, int Npad, int pad, const int32_t* row_off, const int32_t* lens, double rows_total, hipStream_t st);
// ragged batches: (B, Tmax, C) padded rows <-> packed rows [row_off[b], row_off[b + 1]); unpack zeroes the padded rows
int si_launch_repack_rows(si_ctx* ctx, const float* src, float* dst, int B, int Tmax, int C, const int32_t* row_off, bool unpack, hipStream_t st);
// valid_frames[b] = conv-stack length of valid_len[b] samples (modeling_hubert.py:664-677), clamped to [1, T]
int si_launch_frame_lengths(si_ctx* ctx, const int32_t* valid_len, int B, int nconv, const int32_t* kernels, const int32_t* strides,
                            int T, int32_t* valid_frames, hipStream_t st);
// x[b][t][:] = 0 for t >= valid_frames[b] (padded frames of the projected states, modeling_hubert.py:428-431)
int si_launch_zero_padded_rows(si_ctx* ctx, float* x, int B, int T, int H, const int32_t* valid_frames, hipStream_t st);

// Which frames a codebook call works on.  GRID form: frames frame_pos[b] + [0, n) of every clip, outputs (B, n); frame_cnt (B) or null:
// frames replaced per clip (ragged batches), <= n.  TABLE form (multi-gap masks): n entries, entry f = frame frame_pos[f] of clip
// frame_clip[f]; labels / target / terms / pred / cos_pt are flat (n), in table order.  All arrays are device int32.
struct si_cb_frames {
    bool table;
    const int32_t* frame_clip;
    const int32_t* frame_pos;
    const int32_t* frame_cnt;
    int n;
    static si_cb_frames grid(const int32_t* frame_pos, int Lm, const int32_t* frame_cnt = nullptr) { return {false, nullptr, frame_pos, frame_cnt, Lm}; }
    static si_cb_frames of_table(const int32_t* frame_clip, const int32_t* frame_pos, int F) { return {true, frame_clip, frame_pos, nullptr, F}; }
    long frames(int B) const { return table ? (long)n : (long)B * n; }
};

// cosine arg-max against centred centroids + splice of the raw centroid into mel (A10..A13)
int si_launch_codebook_splice(si_ctx* ctx, const float* feats, int B, int T, int D, const si_cb_frames& fr, const float* cb_centered /*K x D*/,
                              const float* cb_raw /*K x D*/, const float* cb_rnorm /*K*/, int K, float* mel, int Tm, int64_t* labels,
                              hipStream_t st);

// out[b][t] = (t < first[b] || t >= last[b]) ? clean[b][t] : masked[b][t]  (I_da/scripts/inpainting.py:209-214)
int si_launch_code_splice(si_ctx* ctx, const int64_t* clean, const int64_t* masked, const int32_t* first, const int32_t* last, int B, int T,
                          int64_t* out, hipStream_t st);

// mel[b, :, pos] = cb_raw[label] for every frame of `fr` (the expected_inpaint splice, I_ea/predict.py:177-189)
int si_launch_codebook_gather(si_ctx* ctx, const int64_t* labels, int B, int D, const si_cb_frames& fr, const float* cb_raw, int K, float* mel,
                              int Tm, hipStream_t st);

// k-means unit assignment: labels[row] = argmin_k ||x_row - c_k||^2 (first minimum); dist (optional) = that squared distance
// cnorm_scratch (K floats, device) or null: with it (and D % 32 == 0) the distance GEMM runs on the matrix pipe (exact-fp32 MFMA)
int si_launch_kmeans_assign(si_ctx* ctx, const float* x, long rows, int D, const float* cent, int K, int64_t* labels, float* dist,
                            hipStream_t st, float* cnorm_scratch = nullptr);

// loss half of LossFunction.cos_sim + cos_sim_target_labels (f-4): per-frame terms 1 - cos(v, c_target), their
// fixed-order sum, arg-max labels and cos(c_pred, c_target)
int si_launch_codebook_metrics(si_ctx* ctx, const float* feats, int B, int T, int D, const si_cb_frames& fr, const float* cb_centered,
                               const float* cb_rnorm, int K, const int64_t* target, float* terms, float* loss, int64_t* pred, float* cos_pt,
                               hipStream_t st);

// mel-domain and waveform metrics (metrics_kernels.hip; I_ea/metrics.py:38-62,127-142)
int si_launch_mel_metrics(si_ctx* ctx, const float* a, const float* b, int B, int D, int L, const float* center, float* out, hipStream_t st);
int si_launch_sisdr(si_ctx* ctx, const float* est, const float* ref, int B, int n, float* out, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// mel front-end kernels (frontend_kernels.hip)
// ------------------------------------------------------------------------------------------------
// n_len / tm_len (B, device) or null: ragged batches -- clip b holds n_len[b] samples (row stride N) and tm_len[b] frames (stride Tm)
int si_launch_wave_peak(si_ctx* ctx, const float* wav, const int32_t* ms, const int32_t* me, int B, int N, float* peak,
                        hipStream_t st, const int32_t* n_len = nullptr, const SiSpans* sp = nullptr /* multi-gap masks: instead of ms / me */);
// mask -> normalise*0.95 -> reflect-pad -> Hann window, as the (B*Tm, kc + nfft / 2) matrix of FOLDED frames
// [w[0], w[k] + w[nfft - k] (k = 1 .. nfft/2 - 1), w[nfft/2], zeros up to kc | 0, w[k] - w[nfft - k]]: the operands of the two
// half-size DFT GEMMs (cosine / sine part)
int si_launch_mel_frames(si_ctx* ctx, const float* wav, const int32_t* ms, const int32_t* me, const float* peak,
                         const float* hann, int B, int N, int Tm, int hop, int pad, int nfft, int kc, int normalize, float* frames,
                         hipStream_t st, const int32_t* n_len = nullptr, const int32_t* tm_len = nullptr, const SiSpans* sp = nullptr);
// spec rows [re | pad | im at im_off] -> sqrt(re^2+im^2+1e-9) -> banded mel basis -> log(clamp 1e-5) -> mel (B, nmel, Tm)
int si_launch_mel_project(si_ctx* ctx, const float* spec, int ld_spec, int nbin, int im_off, const float* basis_t, const int32_t* lo,
                          const int32_t* hi, int nmel, int B, int Tm, float* mel, hipStream_t st, const int32_t* tm_len = nullptr);

// polyphase FIR resampler (upfirdn with resample_poly's centring); taps are device fp32, already pre-padded
int si_launch_resample_poly(si_ctx* ctx, const float* x, int B, int n_in, const float* taps, int ntaps, int up, int down,
                            int pre_remove, int n_out, float* y, hipStream_t st);

// resampy / librosa 0.9.1 `kaiser_best` band-limited interpolation (frontend_kernels.hip); tables are device float64
int si_launch_resample_sinc(si_ctx* ctx, const float* x, const int32_t* n_len, int B, int n_in, const double* win, const double* dwin, int nwin,
                            int num_table, int step, double scale, double ratio, const double* time_reg, int n_out, float* y, hipStream_t st);
// `audio * 32768` + truncating int16 cast (I_ea/predict.py:204-206)
int si_launch_pcm16(si_ctx* ctx, const float* wav, long n, int16_t* out, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// patch mode (patch_kernels.hip)
// ------------------------------------------------------------------------------------------------
// The device half of si_patch_table: per window the first 22.05 kHz sample of its generator row and the row's length, per span the
// window that holds it, per clip lim = min(its samples, its generated samples), and the rising cross-fade ramp (fade floats).
struct SiPatch { const int32_t* win_start; const int32_t* win_len; const int32_t* span_win; const int32_t* lim; const float* ramp; int fade; };
// ext (B, D, Tout) -> out (W, D, Wmax): row (w, d) = ext[clip_w, d, w0_w : w1_w], zero past it; win (device) = [clip (W) | w0 (W) | w1 (W)]
int si_launch_gather_windows(si_ctx* ctx, const float* ext, const int32_t* win, int W, int D, int Tout, int Wmax, float* out, hipStream_t st);
// out / pcm (B, N22; either may be null) = orig outside the blend regions of `sp`, (1 - w) orig + w gain[b] gen inside; gain null = 1
int si_launch_patch_compose(si_ctx* ctx, const float* orig, const SiSpans& sp, const SiPatch& pt, const float* gen, int Lrow, const float* gain,
                            int B, int N22, float* out, int16_t* pcm, hipStream_t st);
// long recordings.  out (C, L) row c = src[start[c] : start[c] + L]; start device int32 (C), validated by the caller.
// ceiling != nullptr: a sample that is si_invalid(., *ceiling) is copied as +0.0
int si_launch_cut_clips(si_ctx* ctx, const float* src, const int32_t* start, int C, int L, const float* ceiling, float* out, hipStream_t st);
// the device half of si_region_table: per span, per window and per chunk arrays on the recording's own sample axis
struct SiRegions {
    const int32_t* start; const int32_t* len; const int32_t* span_win; const int32_t* span_lim;
    const int32_t* win_ctx; const int32_t* win_start; const int32_t* chunk; const int32_t* k0; const int32_t* k1;
    const float* ramp; int fade;
};
// one workgroup per listed chunk: the blended samples of its spans written into out / pcm (N22; either may be null), the rest untouched
int si_launch_patch_regions(si_ctx* ctx, const float* orig, const SiRegions& rt, int Q, const float* gen, int Lrow, const float* gain,
                            int N22, float* out, int16_t* pcm, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// dropout detection (detect_kernels.hip)
// ------------------------------------------------------------------------------------------------
// bytes of scratch the passes need for n samples: one bit per sample, six words per chunk of 2048 samples and two more
size_t si_detect_scratch_bytes(int n);
// One detection call: x device fp32, int16 or packed 24-bit -> runs (max_runs, 2) = the maximal runs of DEAD samples of
// at least min_len samples, sorted by start, and *n_runs = how many there are (all of them, whether or not they fit).  What "dead" means
// is the route's, and SiDetect carries its parameters; a field a route does not name is not read.  Arguments validated by the caller,
// scratch 16-byte aligned.
enum SiDetRoute {
    SI_DET_QUIET,       // |x| <= thr (interleaved 4.18)
    SI_DET_DEAD,        // quiet against T = max(thr, rel * peak) (kind & 1), held = within tol of a neighbour of the same channel (kind & 2) (4.20)
    SI_DET_LEVEL,       // under a window of 2 half + 1 samples whose energy is at most T^2 times their count, dilated by half (4.25)
    SI_DET_BURST,       // under a window of 2 half + 1 centres, cut to [1, n - 2], whose summed squares of x[k - 1] - 2 x[k] + x[k + 1] are at
                        // least T^2 times their count, dilated by half (4.28)
    SI_DET_INVALID,     // si_invalid(x, ceiling): NaN, +-inf, |x| > ceiling; no pass 0, no threshold out, thr not read (4.30)
    SI_DET_IMPULSE,     // within `pad` of a sample whose squared AR(order) prediction error is above T^2 and above ratio^2 times the mean
                        // squared prediction error of the samples within `half` of it, `guard` on either side left out (4.33)
};
struct SiDetect {
    int route;          // SiDetRoute
    float rel;          // dead, level, burst, impulse: T = max(thr, rel * peak), the peak taken by a pass 0 when rel > 0; 0 in the other routes
    float* thr_out;     // the same four: device, may be null; receives T
    int half;           // level, burst, impulse
    int kind;           // dead
    float tol;          // dead
    float ceiling;      // invalid
    int order, guard, pad;      // impulse
    float ratio;        // impulse
};
// channels = 0: x is one channel of n samples.  channels >= 1: x is interleaved (n sample times of `channels` channels),
// channel c >= 0 alone or all jointly (c < 0).  Every route but SI_DET_QUIET takes channels = 1 as the one-channel file.
int si_launch_detect(si_ctx* ctx, const void* x, int fmt, int n, int channels, int channel, float thr, int min_len, int32_t* runs, int max_runs,
                     int32_t* n_runs, char* scratch, hipStream_t st, SiDetect d);
// that prediction error itself, one channel of the file -> e (n) device float64: 0.0 below `order`, NaN at a sample of a bad block
int si_launch_impulse_residual(si_ctx* ctx, const void* x, int fmt, int n, int channels, int channel, int order, double* e, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// band-limited interpolation between two sample rates at the exact rational time: the one set of tables
// and the one per-output sum of rate_kernels.hip and rate_feed_kernels.hip
// ------------------------------------------------------------------------------------------------
// The kaiser_best tables of source rate -> target rate: P / Q = (target, source) / gcd, so output j of the target axis sits at source
// position j Q / P; H = ceil(nwin / step) taps per wing.
struct SiTaps {
    const double* win; const double* dwin; int nwin, num_table, step; double scale;
    int P, Q, H;
};
// Output j from `row`, which holds the source samples from `base` on as fp32 (zero where the source has none).  n, r = divmod(j Q, P)
// in int64; frac = scale (r / P); left wing off, eta = split(frac num_table), taps k < min(n + 1, (nwin - off) / step) on x[n - k];
// right wing the same from scale - frac, taps k < min(cap - n - 1, (nwin - off') / step) on x[n + 1 + k] -- cap: the source's length,
// or a value no n reaches where the row's zeros already end it; weights fma(eta, dwin, win), sum by fma in float64, left ascending
// then right ascending, rounded once to fp32: resample_sinc_kernel's arithmetic at the exact time.  Nothing in it depends on where the
// row starts.  The statements keep this order: a * b - c contracts across them, and the bits depend on it.
template <typename Cap>
__device__ __forceinline__ float si_wings(const float* __restrict__ row, long base, long j, Cap cap, const SiTaps& r) {
    const long P = r.P, Q = r.Q;
    const int nwin = r.nwin, step = r.step;
    const double scale = r.scale, ntab = (double)r.num_table;
    const long t = j * Q;
    const long nl = t / P;
    const int n = (int)nl;
    const double frac = scale * ((double)(t - nl * P) / (double)P);
    double acc = 0.0;
    {
        const double idx = frac * ntab;
        const int off = (int)idx;
        const double eta = idx - (double)off;
        const int taps = min(n + 1, (nwin - off) / step);
        const float* xs = row + (nl - base);
        for (int k = 0; k < taps; ++k) {
            const int i = off + k * step;
            acc = fma(fma(eta, r.dwin[i], r.win[i]), (double)xs[-k], acc);
        }
    }
    {
        const double idx = (scale - frac) * ntab;
        const int off = (int)idx;
        const double eta = idx - (double)off;
        const int taps = (int)min(cap - n - 1, (Cap)((nwin - off) / step));
        const float* xs = row + (nl + 1 - base);
        for (int k = 0; k < taps; ++k) {
            const int i = off + k * step;
            acc = fma(fma(eta, r.dwin[i], r.win[i]), (double)xs[k], acc);
        }
    }
    return (float)acc;
}

// ------------------------------------------------------------------------------------------------
// repair at the file's own sample rate (rate_kernels.hip)
// ------------------------------------------------------------------------------------------------
// si_rate_table's device arrays (spans, span_lim, chunks, fade and ramp in FILE samples; windows in 22.05 kHz samples), the tables of
// 22 050 -> sr, and row_cap = floor(2047 Q / P) + 2 + 2 H: the 22.05 kHz samples one chunk's share of one span can read, the floats of
// dynamic LDS the launch asks for.
struct SiRate {
    const int32_t* start; const int32_t* len; const int32_t* span_win; const int32_t* span_lim;
    const int32_t* win_ctx; const int32_t* win_start; const int32_t* win_len; const int32_t* win_lim;
    const int32_t* chunk; const int32_t* k0; const int32_t* k1;
    const float* ramp; int fade;
    SiTaps r;           // 22 050 -> sr: P / Q = (sr, 22050) / gcd, file sample i sits at 22.05 kHz position i Q / P
    int row_cap;
};
// one workgroup per listed chunk of 2048 file samples: the blended samples of its spans written into out (n_file, orig's type: fp32 or
// int16 / packed 24-bit by fmt), the rest untouched.  ch = 0: a mono file (the mono kernel, profiled as patch_rate); else channel
// `channel` of ch interleaved (patch_rate_ch).  Arguments validated by the caller.
int si_launch_patch_rate(si_ctx* ctx, const void* orig, int fmt, int n_file, int ch, int channel, const SiRate& rt, int num_chunks,
                         const float* gen, int Lrow, const float* gain, void* out, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// context clips cut at the file's own rate (rate_feed_kernels.hip)
// ------------------------------------------------------------------------------------------------
constexpr int RF_TILE = SI_CUT_RATE_TILE;               // consecutive outputs of one clip per workgroup of cut_rate (si_hip.h; native.CUT_RATE_TILE)
constexpr int RF_PAIR_FRAMES = SI_CUT_PAIR_FRAMES;      // consecutive 20 ms frames of one clip per workgroup of cut_pair (si_hip.h; native.CUT_PAIR_FRAMES)
// si_cut_rate: the tables of sr -> 22 050; cap = floor((RF_TILE - 1) Q / P) + 2 + 2 H: the file samples one tile can read, the floats of
// dynamic LDS the launch asks for, and N22 = ceil(n_file P / Q)
struct SiFeed {
    SiTaps r;
    int cap, N22;
};
// si_cut_pair: the tables of sr -> 22 050 and sr -> 16 000; cap = ceil(RF_PAIR_FRAMES sr / 50) + 2 + 2 max(H22, H16): the floats of
// dynamic LDS; N22 = ceil(n_file P22 / Q22), N16 = ceil(n_file P16 / Q16), lim16 = ceil(N22 320 / 441): where a clip's 16 kHz row may
// end; direct16: sr = 16000, r16 holds no tables (H = 0, P = Q = 1)
struct SiPair {
    SiTaps r22, r16;
    int cap, N22, N16, lim16, direct16;
};
// One launcher per kernel family.  The file x (n_file sample times; fp32, int16 or packed 24-bit by fmt): ch = 0 a mono file (the mono
// kernel, profiled as cut_rate), else channel `channel` of ch interleaved (cut_rate_ch).  ceiling = nullptr: the file
// as it is; else a file sample that is si_invalid(., *ceiling), judged in the file's own units before any conversion,
// enters the interpolation (the copy) as +0.0 -- the same grid, LDS and profile family.  Arguments validated by the caller.
// out (C, L) row c = 22.05 kHz samples [start[c], start[c] + L) of x, interpolated at the exact time j Q / P; start device int32 (C)
int si_launch_cut_rate(si_ctx* ctx, const void* x, int fmt, int n_file, int ch, int channel, const int32_t* start, int C, int L, const SiFeed& fd,
                       const float* ceiling, float* out, hipStream_t st);
// out22 (C, L22) row c = 22.05 kHz samples 441 frame[c] + [0, L22), out16 (C, L16) row c = 16 kHz samples 320 frame[c] + [0, L16) of x
int si_launch_cut_pair(si_ctx* ctx, const void* x, int fmt, int n_file, int ch, int channel, const int32_t* frame, int C, int L22, int L16,
                       const SiPair& pr, const float* ceiling, float* out22, float* out16, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// short runs mended in place by least-squares AR interpolation (mend_kernels.hip)
// ------------------------------------------------------------------------------------------------
// one workgroup per row of runs (n_runs, 2): status[row] = SI_MEND_*, and for AR / LINE the samples [start, start + len) of channel
// `channel` of x (n sample times of ch >= 1 interleaved channels, the type fmt names) rewritten; arguments validated by the caller
int si_launch_mend_runs(si_ctx* ctx, void* x, int fmt, int n, int ch, int channel, const int32_t* runs, int n_runs, int max_len, int order,
                        int context, int32_t* status, hipStream_t st);

// erf-GELU of the bf16 encoder's GEMM epilogues (lingemm.hip, gemmcu.hip: the SAME function, their results are bit-identical).
// erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 -- below one fp32 ulp of the result for |x| >= 1 and far below the bf16
// rounding every consumer of these outputs applies; 15 VALU operations instead of libm erff's ~31 with two divergent branches.
__device__ __forceinline__ float si_gelu_fast(float x) {
    const float z = x * 0.70710678118654752440f;
    const float az = __builtin_fabsf(z);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    poly *= t;
    const float e = __builtin_amdgcn_exp2f(-az * az * 1.4426950408889634f);
    const float erf = __builtin_copysignf(fmaf(-poly, e, 1.0f), z);
    return 0.5f * x * (1.0f + erf);
}

// LayerNorm applied to one element: the ONE expression of it on the path.  layernorm_kernel writes y with it; a GEMM epilogue whose
// residual is a LayerNorm output that was never stored (LinGemmParams::res_stats) recomputes the same value from the same floats.
__device__ __forceinline__ float si_ln_apply(float x, float mean, float rstd, float g, float b) { return fmaf((x - mean) * rstd, g, b); }

// leaky-ReLU(0.1) of an accumulator as max(v, 0.1 v) in two VALU ops: fmaxf() would first canonicalise both operands
// (a v_max_f32 v, v, v each), which nothing downstream of an MFMA accumulator needs
__device__ __forceinline__ float si_lrelu01(float v) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(0.1f * v));
    return r;
}

// lrelu(0.1) -> ConvTranspose1d(Cin -> Cin / 2, k = 4, stride 2) of the generator's late stages on the fp16 stream, as a streaming
// GEMM over overlapping input rows (upsample.hip): GEMM row m = input row m, columns n = phase * Cout + co, taps read rows m, m - 1.
struct UpsampleParams {
    const unsigned short* x16;        // (B, Lin, Cin) raw fp16
    const unsigned short* w;          // [taps][N][Cin] fp16 (the tap-GEMM's packing)
    const float* bias;                // [N]: the layer's bias repeated per phase
    unsigned short* out16;            // (B, Lout, Cout) raw fp16
    int B, Lin, M;                    // M GEMM rows per clip (Lin + 1 for k = 4, stride 2, padding 1)
    int Cin, N, taps;
    long ooff;                        // GEMM element (m, n) is element m * N + n - ooff of its clip's output (ooff = padding * Cout)
    long o_clip_stride, o_clip_elems; // elements between clips / per clip of the output
    // ragged batches (NULL: uniform): clip b holds lens_lin[b] input rows, lens_m[b] GEMM rows and lens_lin[b] * N output elements
    // (k = 2 * stride: N output elements per input row); *_host: the same on the host; Lin / M / o_clip_elems = the longest clip's
    const int32_t* lens_lin; const int32_t* lens_m; const int32_t* lens_m_host;
    int total_tiles;                  // set by the launcher
};
// SI_OK when launched, negative on error, 1 when the shape is not covered (the caller runs the tap-GEMM)
int si_launch_upsample_stream(si_ctx* ctx, const UpsampleParams& p, hipStream_t st);

// One ResBlock1 step y' = (y + conv2(lrelu(conv1(lrelu(y)) + b1)) + b2) * alpha [+ previous y'] as one kernel on the raw
// fp16 activation stream (respair.hip: C = 32 / 64; respair_wide.hip: C = 128 / 256).  Returns 1 when the shape is not covered.
struct ResPairParams {
    const unsigned short* y16;   // [B][L][C] raw fp16 activation stream (input and residual)
    unsigned short* out16;       // [B][L][C] raw fp16
    const unsigned short* w1;    // [k][C][C] fp16 (tap, n, ci)
    const unsigned short* w2;
    const float* b1;
    const float* b2;
    int B, L, k, dil;
    float alpha;                 // out = (conv2 + b2 + y) * alpha
    int accumulate;              // out += previous out16
    // ragged batches (NULL: every clip holds L rows): clip b holds lens[b] rows at stride L; lens_host = the same on the host
    const int32_t* lens; const int32_t* lens_host;
    int total_tiles;             // set by the launcher
    float out_slope;             // 0 or 1: none; otherwise out = leaky_relu(out, out_slope) before the fp16 rounding -- the activation of the
                                 // only consumer (the next stage's upsampler on gemmcu.hip), applied by the producer (respair_wide.hip only)
};
int si_launch_respair_wide(si_ctx* ctx, int C, const ResPairParams& p, hipStream_t st);
// A whole ResBlock1 -- three (c1, c2) pairs chained, the residual stream kept in LDS -- as one kernel (reschain.hip: C = 32).
// out = x_3 * alpha [+ previous out]; returns 1 when the shape is not covered.
struct ResChainParams {
    const unsigned short* y16;   // [B][L][C] raw fp16 activation stream
    unsigned short* out16;       // [B][L][C] raw fp16
    const unsigned short* w1[3]; // per pair: [k][C][C] fp16 (tap, n, ci)
    const unsigned short* w2[3];
    const float* b1[3];
    const float* b2[3];
    int B, L, k;
    int dil[3];                  // dilation of c1 per pair (c2 has dilation 1)
    float alpha;
    int accumulate;
    const int32_t* lens; const int32_t* lens_host;   // ragged batches: as ResPairParams
    int total_tiles;
};
int si_launch_reschain(si_ctx* ctx, int C, const ResChainParams& p, hipStream_t st);
int si_launch_respair(si_ctx* ctx, int C, const unsigned short* y16, unsigned short* out16, const void* w1, const void* w2,
                      const float* b1, const float* b2, int B, int L, int k, int dil, float alpha, int accumulate, hipStream_t st,
                      const int32_t* lens = nullptr, const int32_t* lens_host = nullptr, float out_slope = 1.f);

// ------------------------------------------------------------------------------------------------
// vocoder kernels (vocoder_kernels.hip)
// ------------------------------------------------------------------------------------------------
// mel (B, D, Tm) channels-first -> (B, Tout, ldo) channels-last, time-stretched (stretch=1) or copied;
// channels D..ldo-1 are written as zero.
// tm_len / tout_len (B, device) or null: ragged batches -- clip b holds tm_len[b] mel frames (stride Tm) and tout_len[b] output rows (stride Tout)
int si_launch_extend_mel(si_ctx* ctx, const float* mel, int B, int D, int Tm, int Tout, int stretch, float* out, int ldo,
                         hipStream_t st, const int32_t* tm_len = nullptr, const int32_t* tout_len = nullptr);
int si_launch_extend_mel_cf(si_ctx* ctx, const float* mel, int B, int D, int Tm, int Tout, float* out, hipStream_t st);   // (B, D, Tm) -> (B, D, Tout), channels-first
// I_da CodeGenerator front (f-2): embedding look-ups + frame repeat + channel concat -> (B, nparts * E, F) channels-first
int si_launch_small_conv1d(si_ctx* ctx, const float* x, const float* w, const float* bias, const float* res, float* y, int B, int Cin,
                           int Tin, int Cout, int Tout, int K, int stride, int dil, int pad, int relu_in, int channels_last, hipStream_t st);
// the whole F0 encoder in one launch, activations in LDS (vocoder_kernels.hip); 1 = does not fit, launch layer by layer
int si_launch_f0enc_fused(si_ctx* ctx, const float* weights, const float* f0, int B, int T, float* h_out, int in_width, int out_width, int width,
                          int n_state, int depth, int down_t, int stride_t, int growth, int dk, int dpad, double macs, hipStream_t st);
int si_launch_unit_frontend(si_ctx* ctx, const int64_t* code, int Fc, const int64_t* f0_code, int Fp, const float* spk_emb,
                            const float* emb_c, int Kc, const float* emb_p, int Kp, int E, int B, float* out, hipStream_t st);
// leaky_relu(0.01) -> Conv1d(C -> 1, k, pad k/2) -> tanh ; x (B, L, C) channels-last -> wav (B, L)
// lens / lens_host (B) or null: ragged batches -- clip b holds lens[b] rows (stride L) and as many output samples (stride L)
int si_launch_conv_post(si_ctx* ctx, const float* x, const float* w /*[k][C]*/, const float* bias, int B, int L, int C, int k,
                        float* wav, hipStream_t st, const unsigned short* x16 = nullptr /* raw fp16 input instead of x */,
                        const int32_t* lens = nullptr, const int32_t* lens_host = nullptr);
