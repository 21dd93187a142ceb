// api.hip -- C ABI of libsi_hip.so (include/si_hip.h): context, checkpoint packing, forward orchestration.
//
// The checkpoint packing itself (weight-norm folding, re-layout into the tap-GEMM form, the casts, the codebook tables), the
// descriptor check and the layout plan are plain host code in weights_host.cpp; this file keeps the context and the device.
// The result is ONE packed device blob whose layout depends only on the model desc and two environment options, so ranks that
// did not read the checkpoint can receive it by a single RCCL broadcast (si_alloc_weights + si_weights_device_ptr).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "common.h"

using namespace siw;   // GemmW / Layout, the plan and the packer: weights_host.h

struct si_ctx {
    int device = 0;
    si_model_desc d{};
    char err[512] = {0};
    Layout lay;
    char* wdev = nullptr;
    bool weights_ready = false;
    bool weights_verified = false;           // the blob's layout fingerprint has been compared with this context's (si_weights_check)
    std::map<std::string, long> dbg_size;                        // floats of each intermediate of the last forward
    std::map<std::string, std::pair<float*, long>> dbg_capture;  // name -> (device dst, capacity in floats)
    // per-launch HIP-event timing (si_profile_start / si_profile_stop)
    struct ProfRec { int name; hipEvent_t a, b; double flops, bytes; };
    bool prof_on = false;
    std::string prof_filter;             // non-empty: only launches of this kernel family are bracketed
    std::vector<std::string> prof_names;
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    size_t prof_used = 0;
    int prof_open = -1;
    int num_cus = 0;
    std::map<const void*, size_t> dyn_lds;   // per kernel: dynamic-LDS limit already raised on this context's device
    // arithmetic-path options, read from the environment when the context is created (all default to 1)
    PackOpts popt;                           // SI_VOC_OPREADY / SI_VOC_RES16: the two options that move bytes of the packed image
    bool opt_enc_opready = true, opt_att_bf16 = true, opt_enc_lingemm = true;
    bool opt_enc_posconv = true;             // the positional conv on posconv.hip in the bf16 encoder mode (SI_ENC_POSCONV=0: the generic tap-GEMM)
    int opt_ln_fuse = 1;                     // post-LN layers, bf16 mode: LayerNorm outputs read as residuals are recomputed in the GEMM epilogues (SI_ENC_LNFUSE=0: written)
    int opt_voc_upsgemm = 1;                 // the generator's early upsamplers on gemmcu.hip's TC instantiations (SI_VOC_UPSGEMM=0: the tap-GEMM)
    int opt_ffn_pad = 64;                    // elements of padding behind each row of the bf16 FFN intermediate (SI_ENC_FFNPAD; multiple of 8, <= 128):
                                             // rows 6144 bytes apart are 6272 apart instead -- FFN2 -1.5 % (profiles/r04_ffnpad_ab.txt), same values
    int opt_gemmcu = 1;                      // encoder GEMMs as one tile per CU (gemmcu.hip): 0 never, 1 by the shape rule, 2 whenever the shape allows, 10 + c (A/B)
    int opt_voc_chain = 1;                   // whole-resblock kernel on the C = 32 stage (SI_VOC_CHAIN=0: one launch per conv pair)
    int opt_voc_fuse = 1;                    // 0: never, 1: every covered width, otherwise a mask of the channel counts to fuse (32 | 64 | 128 | 256)
    // constant tables of the mel front-end (built on first use): DFT matrix [Npad][n_fft] = rows cos | -sin, periodic
    // Hann window, transposed Slaney mel basis with the non-zero bin span of every band
    char* fe_dev = nullptr;
    size_t fe_dft = 0, fe_hann = 0, fe_basis = 0, fe_lo = 0, fe_hi = 0;
    // ragged batches: per-clip length tables are built on the host (launch grids depend on them) and reach the device through a
    // small ring of pinned staging slots (an async copy from pageable memory may still be reading its source after the call returns)
    std::vector<int32_t> vl_host;            // the table of the call in progress (launchers read it during the call only)
    static constexpr int VL_SLOTS = 4;
    int32_t* vl_pin[VL_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t vl_pin_ints[VL_SLOTS] = {0, 0, 0, 0};
    hipEvent_t vl_ev[VL_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int vl_next = 0;
    float* km_cnorm = nullptr;               // |c_k|^2 scratch of si_kmeans_assign (K floats; library-owned, stream-ordered reuse)
    int km_cnorm_cap = 0;
    char* det_scratch = nullptr;             // bitmap + per-chunk words of si_quiet_runs (library-owned, stream-ordered reuse, grown on demand)
    size_t det_scratch_cap = 0;
    // test switch SI_WS_REDZONE: bytes the carve leaves untouched around every region, and the regions of each
    // pass's most recent carve (si_debug_ws_regions); fixed arrays, written on the host at carve time
    size_t ws_zone = 0;
    struct WsRegion { const char* name; size_t offset, bytes; };      // (the name is the carve call's literal)
    struct WsLog { int n = 0; WsRegion r[SI_WS_MAX_REGIONS]; };
    WsLog ws_log[3];                         // SI_WS_ENCODER, SI_WS_VOCODER, SI_WS_MEL
};

int si_fail(si_ctx* ctx, int code, const char* fmt, ...) {
    char* dst = ctx ? ctx->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}
int si_fail_hip(si_ctx* ctx, hipError_t e, const char* what, const char* file, int line) {
    return si_fail(ctx, SI_EHIP, "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
}

// Test hook: remember the size of a named intermediate and, when a capture is registered for it, copy it out
// the moment it is produced (workspace buffers are recycled later in the same forward).  n elements of esize bytes
// (2: raw bf16 / fp16, copied bit for bit; such names end in ".bf16" / ".f16"); ld > 0: n / cols rows of `cols` elements stored
// ld elements apart (the padded FFN intermediate), captured dense.  A capacity smaller than n keeps the leading whole rows.
// A name with a conversion in it ("layer%d.h": the per-conv / per-layer / per-pair taps, numbered by a, b, c) is formatted and
// looked up only while some capture is registered, so the forward without captures formats no name and touches no map.
struct TapSrc { const void* p; long n; int esize = 4; long cols = 0, ld = 0; };
static int si_tap(si_ctx* ctx, hipStream_t st, TapSrc s, const char* fmt, int a = 0, int b = 0, int c = 0) {
    if (ctx->dbg_capture.empty() && strchr(fmt, '%')) return SI_OK;
    char name[48];
    snprintf(name, sizeof(name), fmt, a, b, c);
    ctx->dbg_size[name] = s.n;
    auto it = ctx->dbg_capture.find(name);
    if (it == ctx->dbg_capture.end()) return SI_OK;
    const long m = s.n < it->second.second ? s.n : it->second.second;
    if (m <= 0) return SI_OK;
    if (s.ld > s.cols && s.cols > 0) {
        if (m / s.cols > 0)
            SI_HIP_CHECK(hipMemcpy2DAsync(it->second.first, (size_t)s.cols * s.esize, s.p, (size_t)s.ld * s.esize, (size_t)s.cols * s.esize,
                                          (size_t)(m / s.cols), hipMemcpyDeviceToDevice, st));
    } else {
        SI_HIP_CHECK(hipMemcpyAsync(it->second.first, s.p, (size_t)m * s.esize, hipMemcpyDeviceToDevice, st));
    }
    return SI_OK;
}

// Per-launch timing with HIP events recorded on the launch stream (the same stream the kernel runs on).
// Called by every si_launch_* around its kernel; a no-op unless si_profile_start armed it.
void si_prof_begin(si_ctx* ctx, const char* name, double flops, double bytes, hipStream_t st) {
    if (!ctx->prof_on || ctx->prof_used + 2 > ctx->prof_pool.size()) { ctx->prof_open = -1; return; }
    if (!ctx->prof_filter.empty() && ctx->prof_filter != name) { ctx->prof_open = -1; return; }
    int id = -1;
    for (size_t i = 0; i < ctx->prof_names.size(); ++i) if (ctx->prof_names[i] == name) { id = (int)i; break; }
    if (id < 0) { id = (int)ctx->prof_names.size(); ctx->prof_names.push_back(name); }
    si_ctx::ProfRec r{id, ctx->prof_pool[ctx->prof_used], ctx->prof_pool[ctx->prof_used + 1], flops, bytes};
    ctx->prof_used += 2;
    (void)hipEventRecord(r.a, st);
    ctx->prof_open = (int)ctx->prof_recs.size();
    ctx->prof_recs.push_back(r);
}
const char* si_prof_shape_name(const char* name, long M, int N, int K) {
    static const bool on = getenv("SI_PROF_SHAPES") && atoi(getenv("SI_PROF_SHAPES")) != 0;
    if (!on) return name;
    static thread_local char buf[48];
    snprintf(buf, sizeof(buf), "%s_%ldx%dx%d", name, M, N, K);
    return buf;
}
int si_ensure_dyn_lds(si_ctx* ctx, const void* kern, size_t bytes) {
    if (bytes <= 64 * 1024) return SI_OK;
    size_t& have = ctx->dyn_lds[kern];
    if (bytes > have) {
        SI_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = bytes;
    }
    return SI_OK;
}
int si_opt_gemmcu(const si_ctx* ctx) { return ctx->opt_gemmcu; }
int si_num_cus(si_ctx* ctx) {
    if (ctx->num_cus <= 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->num_cus = n;
    }
    return ctx->num_cus;
}
// host table (ctx->vl_host) -> device `dst`, stream-ordered, through the next pinned slot
static int vl_upload(si_ctx* ctx, int32_t* dst, hipStream_t st) {
    const size_t n = ctx->vl_host.size();
    const int slot = ctx->vl_next;
    ctx->vl_next = (slot + 1) % si_ctx::VL_SLOTS;
    if (!ctx->vl_ev[slot]) SI_HIP_CHECK(hipEventCreateWithFlags(&ctx->vl_ev[slot], hipEventDisableTiming));
    else SI_HIP_CHECK(hipEventSynchronize(ctx->vl_ev[slot]));                  // the copy that last used this slot has finished
    if (ctx->vl_pin_ints[slot] < n) {
        if (ctx->vl_pin[slot]) SI_HIP_CHECK(hipHostFree(ctx->vl_pin[slot]));
        ctx->vl_pin[slot] = nullptr; ctx->vl_pin_ints[slot] = 0;
        SI_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ctx->vl_pin[slot]), std::max<size_t>(n, 4096) * sizeof(int32_t), hipHostMallocDefault));
        ctx->vl_pin_ints[slot] = std::max<size_t>(n, 4096);
    }
    memcpy(ctx->vl_pin[slot], ctx->vl_host.data(), n * sizeof(int32_t));
    SI_HIP_CHECK(hipMemcpyAsync(dst, ctx->vl_pin[slot], n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SI_HIP_CHECK(hipEventRecord(ctx->vl_ev[slot], st));
    return SI_OK;
}
void si_prof_end(si_ctx* ctx, hipStream_t st) {
    if (ctx->prof_open < 0) return;
    (void)hipEventRecord(ctx->prof_recs[ctx->prof_open].b, st);
    ctx->prof_open = -1;
}

namespace {

int stage_channels(const si_ctx* ctx, int i) { return siw::stage_channels(ctx->d, ctx->popt, i); }
BlobHeader blob_header(const si_ctx* ctx) { return siw::blob_header(ctx->d, ctx->popt, ctx->lay); }
Err ctx_err(si_ctx* ctx) { return ctx ? Err{ctx->err, sizeof(ctx->err)} : Err{g_create_err, sizeof(g_create_err)}; }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The regions of one pass, carved in order from the caller's workspace at 256-aligned offsets.  zone > 0 (SI_WS_REDZONE): `zone` bytes
// that nothing is handed out of lie in front of the first region and behind every region, the last one included.  Every region is
// recorded by name in the pass's log; one more than the log holds fails the carve like one past the estimate.
struct Carver {
    char* base; size_t cap; size_t zone; si_ctx::WsLog* log; size_t cur; bool ok = true;
    const char* failed = "";                 // the first region that did not fit (for the refusal's message)
    float* floats(size_t n, const char* name) { return reinterpret_cast<float*>(bytes(n * 4, name)); }
    char* bytes(size_t n, const char* name) {
        size_t o = cur; cur = align_up(cur + n, 256) + zone;
        if (cur > cap || log->n >= SI_WS_MAX_REGIONS) { if (ok) failed = name; ok = false; return base; }
        log->r[log->n++] = {name, o, n};
        return base + o;
    }
};
Carver carver(si_ctx* ctx, int which, void* workspace, size_t workspace_bytes) {
    ctx->ws_log[which].n = 0;
    return Carver{static_cast<char*>(workspace), workspace_bytes, ctx->ws_zone, &ctx->ws_log[which], ctx->ws_zone};
}
// zones the estimates pay for: one in front, one behind each region a pass can carve (encoder: the length table or the frame
// counts, never both; generator: table, mel, 6 + 6 buffers; mel: 3 + table)
constexpr int ENC_WS_ZONES = 18, VOC_WS_ZONES = 15, MEL_WS_ZONES = 5;

// Ragged batches: the per-clip length table of the call in progress.  `fill` writes its `ints` zeroed entries on the host and returns
// an error code for a length it refuses; the table is then carved from the `what` workspace and uploaded in stream order.
struct VlTable { const int32_t* host = nullptr; int32_t* dev = nullptr; };
template <class Fill>
int vl_table(si_ctx* ctx, Carver& W, size_t ints, hipStream_t st, const char* what, VlTable& t, Fill fill) {
    ctx->vl_host.assign(ints, 0);
    if (int rc = fill(ctx->vl_host.data())) return rc;
    t.dev = reinterpret_cast<int32_t*>(W.bytes(ints * 4, "lengths"));
    if (!W.ok) return si_fail(ctx, SI_ENOMEM, "internal: %s workspace carve exceeded its own estimate at region '%s'", what, W.failed);
    if (int rc = vl_upload(ctx, t.dev, st)) return rc;
    t.host = ctx->vl_host.data();
    return SI_OK;
}

struct EncDims { int T; std::vector<int> L; };
EncDims enc_dims(const si_model_desc& d, int N) {
    EncDims e; e.L.push_back(N);
    int n = N;
    for (int i = 0; i < d.num_conv; ++i) { n = n >= d.conv_kernel[i] ? (n - d.conv_kernel[i]) / d.conv_stride[i] + 1 : 0; e.L.push_back(n); }
    e.T = n;
    return e;
}

size_t encoder_ws_bytes(const si_ctx* ctx, int B, int N) {
    const si_model_desc& d = ctx->d;
    EncDims e = enc_dims(d, N);
    size_t cmax = 0;
    for (int i = 0; i < d.num_conv; ++i) cmax = std::max(cmax, (size_t)e.L[i + 1] * d.conv_dim[i]);
    const size_t BT = (size_t)B * std::max(e.T, 1);
    size_t f = 2 * (size_t)B * cmax + BT * d.conv_dim[d.num_conv - 1] + BT * d.hidden_size * 3 + BT * 3 * d.hidden_size + BT * d.intermediate_size +
               (size_t)B * d.conv_dim[0] * 2 + BT * 2;                    // (+ the LayerNorm (mean, rstd) rows of the fused post-LN layers)
    // bf16 operand-ready copies (encoder in bf16 mode): LN(features), hidden, attention output, FFN intermediate
    const size_t h16 = (BT * d.conv_dim[d.num_conv - 1] + 2 * BT * d.hidden_size + BT * (d.intermediate_size + 128)) * 2;   // (+ the row padding of the FFN intermediate)
    return f * 4 + h16 + (size_t)B * 16 + (size_t)B * 4 + si_conv0_partials_bytes(B, N) + 41 * 256 +
           align_up((size_t)(SI_MAX_CONV + 3) * (B + 1) * 4, 256) +   // ragged batches: per-layer length table + row offsets
           ENC_WS_ZONES * ctx->ws_zone;
}

// Clips per vocoder pass.  Measured on MI355X (B = 32, fp32): 4 -> 109 ms/step, 8 -> 93, 16 -> 89, 32 -> 88: small
// chunks leave the early stages (L = 2752 rows per clip) with fewer workgroups than CUs, and the fp32 MFMA path
// is compute-bound, so cache residency of a small chunk buys nothing.
int vocoder_chunk(const si_model_desc& d, int B) { int c = d.vocoder_chunk > 0 ? d.vocoder_chunk : 32; return std::min(c, std::max(B, 1)); }

long voc_tout(int Tm, int stretch) { return stretch ? (long)std::floor((double)Tm * (441.0 / 256.0)) : Tm; }

size_t vocoder_ws_bytes(const si_ctx* ctx, int B, int Tm, int stretch) {
    const si_model_desc& d = ctx->d;
    const int Bc = vocoder_chunk(d, B);
    const long Tout = voc_tout(Tm, stretch);
    size_t lc_max = (size_t)Tout * d.up_initial_channel;
    long L = Tout; int c = d.up_initial_channel;
    for (int i = 0; i < d.num_ups; ++i) { L *= d.up_rates[i]; c = stage_channels(ctx, i); lc_max = std::max(lc_max, (size_t)L * c); }
    // 6 fp32 activation buffers + 6 half-size buffers for the operand-ready 16-bit copies (bf16 / fp16 modes)
    const size_t f = (size_t)Bc * Tout * ctx->lay.mel_ld + 9 * (size_t)Bc * lc_max;
    return f * 4 + 32 * 256 + align_up((size_t)(2 * SI_MAX_UPS + 3) * B * 4, 256) +   // ragged batches: per-stage length table
           VOC_WS_ZONES * ctx->ws_zone;
}

TapGemmParams gemm_params(const si_ctx* ctx, const GemmW& G) {
    TapGemmParams p{};
    p.w = ctx->wdev + G.w;
    p.w_lo = G.math == SI_MATH_BF16X3 ? ctx->wdev + G.w_lo : nullptr;
    p.bias = G.has_bias ? reinterpret_cast<const float*>(ctx->wdev + G.bias) : nullptr;
    p.Cin = G.Cin; p.N = G.N; p.Npad = G.Npad; p.ntaps = G.ntaps; p.groups = G.groups;
    p.stride = 1; p.dil = 1; p.pad = 0; p.pro_slope = 1.f; p.act = SI_ACT_NONE; p.alpha = 1.f; p.accumulate = 0;
    p.out16_slope = 1.f;
    p.nseg = 1;
    return p;
}

// ConvTranspose1d(k, stride u, padding (k - u) / 2) of upsampler i over Lin rows as a GEMM: row m holds the u output rows
// m * u - pad .. m * u - pad + u - 1 (the phases), so Lout = u * Lin output rows take M GEMM rows
struct UpsGeom { int u, pad; long Lout; int M; };
UpsGeom ups_geom(const si_model_desc& d, int i, long Lin) {
    const int u = d.up_rates[i], pad = (d.up_kernels[i] - u) / 2;
    const long Lout = Lin * u;
    return UpsGeom{u, pad, Lout, (int)((pad + Lout - 1) / u + 1)};
}

// y(rows x N) = x(rows x K) W^T + b [+act] [+res], with the optional operands of LinearIo:
// x16 / y16: operand-ready bf16 input (instead of x) / additional-or-only bf16 output, see TapGemmParams
// ld_in / ld_out (elements; 0 = dense): row strides of the 16-bit input / of the output when they are padded (the FFN intermediate)
// res_ln (stats, gamma, beta): the residual is LayerNorm(res), recomputed in the GEMM's epilogue (TapGemmParams::res_stats)
struct ResLn { const float* stats = nullptr; const float* gamma = nullptr; const float* beta = nullptr; };
struct LinearIo { const unsigned short* x16 = nullptr; unsigned short* y16 = nullptr; int ld_in = 0, ld_out = 0; ResLn res_ln; };
int linear(si_ctx* ctx, const GemmW& G, const float* x, float* y, long rows, int act, const float* res, hipStream_t st, const LinearIo& io = LinearIo()) {
    TapGemmParams p = gemm_params(ctx, G);
    p.x = io.x16 ? nullptr : x; p.x16 = io.x16; p.out = y; p.out16 = io.y16; p.res = res; p.act = act;
    p.res_stats = io.res_ln.stats; p.res_gamma = io.res_ln.gamma; p.res_beta = io.res_ln.beta;
    p.nseg = 1; p.Lin = (int)rows; p.M = (int)rows; p.ldx = io.ld_in ? io.ld_in : G.Cin; p.x_seg_stride = 0;
    p.ldo = io.ld_out ? io.ld_out : G.N; p.o_seg_stride = 0; p.ooff = 0; p.olimit = rows * p.ldo;
    p.lingemm = ctx->opt_enc_lingemm;
    return si_launch_tapgemm(ctx, G.math, p, st);
}

const float* wf(const si_ctx* ctx, size_t off) { return reinterpret_cast<const float*>(ctx->wdev + off); }

}  // namespace

static int hubert_run(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len, const int32_t* valid_len,
                      int normalize, float norm_eps, const double* pre_add, int output_layer, int B, int N, float* out_feats, float* out_hidden,
                      void* workspace, size_t workspace_bytes, si_stream_t stream, const int32_t* host_len = nullptr, const SiSpans* spans = nullptr);

// A span table as the C ABI takes it: everything the kernels assume is checked here, on the host copy, before anything is launched.
static int check_span_table(si_ctx* ctx, const char* who, const si_span_table* t, int B, SiSpans& out) {
    if (!t || t->struct_size != (int32_t)sizeof(si_span_table)) return si_fail(ctx, SI_EINVAL, "%s: si_span_table size mismatch", who);
    if (!t->host_off || !t->span_off) return si_fail(ctx, SI_EINVAL, "%s: span table with NULL offsets", who);
    if (t->num_clips != B) return si_fail(ctx, SI_EINVAL, "%s: span table for %d clips, batch of %d", who, t->num_clips, B);
    if (t->host_off[0] != 0 || t->host_off[B] != t->num_spans || t->num_spans < 0)
        return si_fail(ctx, SI_EINVAL, "%s: span offsets run 0 .. %d but the table holds %d spans", who, t->host_off[B], t->num_spans);
    if (t->num_spans > 0 && (!t->host_start || !t->host_len || !t->span_start || !t->span_len))
        return si_fail(ctx, SI_EINVAL, "%s: span table with NULL start / len", who);
    for (int b = 0; b < B; ++b) {
        const int k0 = t->host_off[b], k1 = t->host_off[b + 1];
        if (k1 < k0 || k1 > t->num_spans) return si_fail(ctx, SI_EINVAL, "%s: span offsets of clip %d decrease or leave the table", who, b);
        if (k1 - k0 > SI_MAX_SPANS) return si_fail(ctx, SI_EINVAL, "%s: clip %d has %d spans, more than SI_MAX_SPANS = %d", who, b, k1 - k0, SI_MAX_SPANS);
        for (int k = k0; k < k1; ++k) {
            const long s = t->host_start[k], l = t->host_len[k];
            if (s < 0 || l < 0 || s + l > 0x7fffffffL) return si_fail(ctx, SI_EINVAL, "%s: clip %d span %d = [%ld, +%ld) is not a sample range", who, b, k - k0, s, l);
            if (k > k0 && s < (long)t->host_start[k - 1] + t->host_len[k - 1])
                return si_fail(ctx, SI_EINVAL, "%s: clip %d span %d overlaps or precedes span %d (spans must be sorted and disjoint)", who, b, k - k0, k - k0 - 1);
        }
    }
    out = SiSpans{t->span_off, t->span_start, t->span_len};
    return SI_OK;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int si_version(void) { return SI_ABI_VERSION; }

const char* si_last_error(const si_ctx* ctx) { return ctx ? ctx->err : g_create_err; }

int si_create(si_ctx** out, int device_id, const si_model_desc* desc) {
    if (!out) return si_fail(nullptr, SI_EINVAL, "si_create: out is NULL");
    *out = nullptr;
    int rc = check_desc(desc, ctx_err(nullptr));
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev)
        return si_fail(nullptr, SI_EHIP, "si_create: device %d not available (%d HIP devices visible)", device_id, ndev);
    si_ctx* ctx = new si_ctx();
    ctx->device = device_id;
    ctx->d = *desc;
    ctx->popt = pack_opts_from_env();        // the same reading as si_plan_weights / si_pack_weights_host
    ctx->opt_voc_fuse = getenv("SI_VOC_FUSE") ? atoi(getenv("SI_VOC_FUSE")) : 1;
    ctx->opt_voc_chain = getenv("SI_VOC_CHAIN") ? atoi(getenv("SI_VOC_CHAIN")) : 1;
    ctx->opt_enc_opready = env_flag("SI_ENC_OPREADY");
    ctx->opt_att_bf16 = env_flag("SI_ATT_BF16");
    ctx->opt_enc_lingemm = env_flag("SI_ENC_LINGEMM");
    ctx->opt_enc_posconv = env_flag("SI_ENC_POSCONV");
    ctx->opt_gemmcu = getenv("SI_ENC_GEMMCU") ? atoi(getenv("SI_ENC_GEMMCU")) : 1;
    ctx->opt_ln_fuse = getenv("SI_ENC_LNFUSE") ? atoi(getenv("SI_ENC_LNFUSE")) : 1;
    ctx->opt_voc_upsgemm = getenv("SI_VOC_UPSGEMM") ? atoi(getenv("SI_VOC_UPSGEMM")) : 1;
    ctx->opt_ffn_pad = getenv("SI_ENC_FFNPAD") ? std::min(128, std::max(0, atoi(getenv("SI_ENC_FFNPAD")) / 8 * 8)) : 64;
    ctx->ws_zone = getenv("SI_WS_REDZONE") ? (size_t)std::min(1L << 20, std::max(0L, atol(getenv("SI_WS_REDZONE")))) / 256 * 256 : 0;
    plan_layout(ctx->d, ctx->popt, ctx->lay);
    *out = ctx;
    return SI_OK;
}

void si_destroy(si_ctx* ctx) {
    if (!ctx) return;
    if (ctx->wdev) { (void)hipSetDevice(ctx->device); (void)hipFree(ctx->wdev); }
    if (ctx->fe_dev) { (void)hipSetDevice(ctx->device); (void)hipFree(ctx->fe_dev); }
    if (ctx->km_cnorm) { (void)hipSetDevice(ctx->device); (void)hipFree(ctx->km_cnorm); }
    if (ctx->det_scratch) { (void)hipSetDevice(ctx->device); (void)hipFree(ctx->det_scratch); }
    for (hipEvent_t e : ctx->prof_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < si_ctx::VL_SLOTS; ++i) {
        if (ctx->vl_ev[i]) { (void)hipEventSynchronize(ctx->vl_ev[i]); (void)hipEventDestroy(ctx->vl_ev[i]); }
        if (ctx->vl_pin[i]) (void)hipHostFree(ctx->vl_pin[i]);
    }
    delete ctx;
}

int si_alloc_weights(si_ctx* ctx) {
    if (!ctx) return SI_EINVAL;
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->wdev) SI_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx->wdev), ctx->lay.total));
    ctx->weights_ready = true;          // bytes arrive by broadcast before the first forward
    ctx->weights_verified = false;      // ... and are checked against this context's layout then (si_weights_check)
    return SI_OK;
}

int si_load_weights(si_ctx* ctx, const void* host_blob, size_t nbytes, const char* index) {
    if (!ctx || !host_blob || !index) return si_fail(ctx, SI_EINVAL, "si_load_weights: NULL argument");
    std::vector<char> image;                 // the same bytes si_pack_weights_host returns, header included
    int rc = pack_image(ctx->d, ctx->popt, ctx->lay, host_blob, nbytes, index, image, ctx_err(ctx));
    if (rc) return rc;                       // a refused checkpoint leaves the device blob and the context's state as they were
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->wdev) SI_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx->wdev), ctx->lay.total));
    SI_HIP_CHECK(hipMemcpy(ctx->wdev, image.data(), ctx->lay.total, hipMemcpyHostToDevice));
    ctx->weights_ready = true;
    ctx->weights_verified = true;
    return SI_OK;
}

int si_weights_check(si_ctx* ctx) {
    if (!ctx) return SI_EINVAL;
    if (!ctx->wdev) return si_fail(ctx, SI_ESTATE, "weights are not allocated: call si_load_weights or si_alloc_weights first");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    BlobHeader got{};
    SI_HIP_CHECK(hipMemcpy(&got, ctx->wdev, sizeof(got), hipMemcpyDeviceToHost));
    const BlobHeader want = blob_header(ctx);
    if (got.magic != want.magic || got.version != want.version || got.fingerprint != want.fingerprint || got.total != want.total)
        return si_fail(ctx, SI_EWEIGHTS, "the weight blob in this context was packed for a different layout (fingerprint %016llx / %llu bytes, this "
                       "context plans %016llx / %llu): the source rank's model desc or SI_VOC_* environment differs, or the broadcast has not arrived",
                       (unsigned long long)got.fingerprint, (unsigned long long)got.total, (unsigned long long)want.fingerprint, (unsigned long long)want.total);
    ctx->weights_verified = true;
    return SI_OK;
}

int si_weights_device_ptr(si_ctx* ctx, void** ptr, size_t* nbytes) {
    if (!ctx || !ptr || !nbytes) return si_fail(ctx, SI_EINVAL, "si_weights_device_ptr: NULL argument");
    if (!ctx->wdev) return si_fail(ctx, SI_ESTATE, "weights are not allocated: call si_load_weights or si_alloc_weights first");
    *ptr = ctx->wdev;
    *nbytes = ctx->lay.total;
    return SI_OK;
}

int si_num_frames(const si_ctx* ctx, int N) { return ctx ? enc_dims(ctx->d, N).T : SI_EINVAL; }

int si_vocoder_samples(const si_ctx* ctx, int Tm, int stretch) {
    if (!ctx) return SI_EINVAL;
    long L = voc_tout(Tm, stretch);
    for (int i = 0; i < ctx->d.num_ups; ++i) L *= ctx->d.up_rates[i];
    return (int)L;
}

int si_workspace_bytes(si_ctx* ctx, int B, int N, int Tm, size_t* out) {
    if (!ctx || !out || B <= 0) return si_fail(ctx, SI_EINVAL, "si_workspace_bytes: bad argument");
    size_t a = N > 0 ? encoder_ws_bytes(ctx, B, N) : 0;
    size_t b = Tm > 0 ? vocoder_ws_bytes(ctx, B, Tm, 1) : 0;
    *out = std::max(a, b);
    return SI_OK;
}

int si_hubert_forward(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len, int normalize, int B, int N,
                      float* out_feats, void* workspace, size_t workspace_bytes, si_stream_t stream) {
    return si_hubert_forward_padded(ctx, wav, mask_start, mask_len, nullptr, normalize, B, N, out_feats, workspace, workspace_bytes, stream);
}

int si_hubert_forward_padded(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len, const int32_t* valid_len,
                             int normalize, int B, int N, float* out_feats, void* workspace, size_t workspace_bytes, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!out_feats) return si_fail(ctx, SI_EINVAL, "si_hubert_forward: NULL / empty argument");
    return hubert_run(ctx, wav, mask_start, mask_len, valid_len, normalize, 1e-7f, nullptr, 0, B, N, out_feats, nullptr, workspace,
                      workspace_bytes, stream);
}

int si_hubert_forward_varlen(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len, const int32_t* sample_len,
                             int normalize, int B, int N, float* out_feats, void* workspace, size_t workspace_bytes, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!out_feats || !sample_len) return si_fail(ctx, SI_EINVAL, "si_hubert_forward_varlen: NULL argument");
    return hubert_run(ctx, wav, mask_start, mask_len, nullptr, normalize, 1e-7f, nullptr, 0, B, N, out_feats, nullptr, workspace, workspace_bytes,
                      stream, sample_len);
}

int si_hubert_extract_features(si_ctx* ctx, const si_extract_desc* x, const float* wav, const int32_t* mask_start, const int32_t* mask_len,
                               const double* pre_mask_add, int B, int N, float* out_hidden, void* workspace, size_t workspace_bytes,
                               si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!x || x->struct_size != (int32_t)sizeof(si_extract_desc)) return si_fail(ctx, SI_EINVAL, "si_hubert_extract_features: si_extract_desc size mismatch");
    if (!out_hidden) return si_fail(ctx, SI_EINVAL, "si_hubert_extract_features: NULL output");
    if (x->output_layer < 1 || x->output_layer > ctx->d.num_layers)
        return si_fail(ctx, SI_EINVAL, "output_layer %d outside 1..%d", x->output_layer, ctx->d.num_layers);
    if (x->normalize < 0 || x->normalize > 2) return si_fail(ctx, SI_EINVAL, "normalize mode %d unknown (0 none, 1 processor, 2 layer_norm)", x->normalize);
    return hubert_run(ctx, wav, mask_start, mask_len, nullptr, x->normalize != 0, x->normalize == 2 ? 1e-5f : 1e-7f, pre_mask_add,
                      x->output_layer, B, N, nullptr, out_hidden, workspace, workspace_bytes, stream);
}

int si_hubert_forward_spans(si_ctx* ctx, const float* wav, const si_span_table* spans, const int32_t* sample_len, int normalize,
                            int B, int N, float* out_feats, void* workspace, size_t workspace_bytes, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!out_feats || B <= 0) return si_fail(ctx, SI_EINVAL, "si_hubert_forward_spans: NULL / empty argument");
    SiSpans sp;
    if (int rc = check_span_table(ctx, "si_hubert_forward_spans", spans, B, sp)) return rc;
    return hubert_run(ctx, wav, nullptr, nullptr, nullptr, normalize, 1e-7f, nullptr, 0, B, N, out_feats, nullptr, workspace, workspace_bytes,
                      stream, sample_len, &sp);
}

int si_code_splice(si_ctx* ctx, const int64_t* code_clean, const int64_t* code_masked, const int32_t* first, const int32_t* last, int B, int T,
                   int64_t* out, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!code_clean || !code_masked || !first || !last || !out || B <= 0 || T <= 0) return si_fail(ctx, SI_EINVAL, "si_code_splice: NULL / empty argument");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_code_splice(ctx, code_clean, code_masked, first, last, B, T, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// The encoder.  output_layer = 0: all layers [+ the stable flavour's final LayerNorm] + final_layers -> out_feats (B, T, codebook_dim).
// output_layer = L >= 1: stop after L transformer layers and copy the hidden state (the residual stream in the pre-LN flavour, the
// layer's output LayerNorm in the post-LN one) to out_hidden (B, T, H) -- fairseq's extract_features(output_layer = L).
// host_len (B, HOST) or null: ragged batch -- clip b holds host_len[b] samples of its row of N; each clip's result equals that clip
// run alone (conv0 statistics over its own rows, convolutions stop at its own lengths, the transformer runs on PACKED rows).
static int hubert_run(si_ctx* ctx, const float* wav, const int32_t* mask_start, const int32_t* mask_len, const int32_t* valid_len,
                      int normalize, float norm_eps, const double* pre_add, int output_layer, int B, int N, float* out_feats, float* out_hidden,
                      void* workspace, size_t workspace_bytes, si_stream_t stream, const int32_t* host_len, const SiSpans* spans) {
    if (!ctx->weights_ready) return si_fail(ctx, SI_ESTATE, "si_hubert_forward before weights were loaded");
    if (!ctx->weights_verified) if (int rcw = si_weights_check(ctx)) return rcw;      // a received blob: once, before its first use
    if (!wav || !workspace || B <= 0) return si_fail(ctx, SI_EINVAL, "si_hubert_forward: NULL / empty argument");
    const si_model_desc& d = ctx->d;
    const Layout& L = ctx->lay;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const EncDims e = enc_dims(d, N);
    if (e.T < 1) return si_fail(ctx, SI_EINVAL, "clip of %d samples is shorter than the conv stack's receptive field", N);
    if (workspace_bytes < encoder_ws_bytes(ctx, B, N))
        return si_fail(ctx, SI_ENOMEM, "workspace of %zu bytes < %zu needed for B=%d N=%d", workspace_bytes, encoder_ws_bytes(ctx, B, N), B, N);
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    const int T = e.T, H = d.hidden_size, I = d.intermediate_size, CF = d.conv_dim[d.num_conv - 1];
    size_t cmax = 0;
    for (int i = 0; i < d.num_conv; ++i) cmax = std::max(cmax, (size_t)e.L[i + 1] * d.conv_dim[i]);

    Carver W = carver(ctx, SI_WS_ENCODER, workspace, workspace_bytes);
    // ---- ragged batch: the table [samples | L_1 .. L_nconv | row offsets (B + 1)] on the host and on the device
    const bool vl = host_len != nullptr;
    VlTable tab;
    long rows_packed = 0;
    double sum_t2 = 0.0;
    if (vl) {
        if (valid_len || output_layer) return si_fail(ctx, SI_EINVAL, "ragged batches: not combined with padded batches or output_layer");
        if (d.codebook_dim % 4) return si_fail(ctx, SI_EINVAL, "ragged batches need codebook_dim %% 4 == 0");
        const size_t off = (size_t)(d.num_conv + 1) * B;               // the row offsets
        if (int trc = vl_table(ctx, W, off + B + 1, st, "encoder", tab, [&](int32_t* t) -> int {
            for (int b = 0; b < B; ++b) {
                if (host_len[b] < 1 || host_len[b] > N) return si_fail(ctx, SI_EINVAL, "ragged batch: clip %d holds %d samples, outside 1..%d", b, host_len[b], N);
                const EncDims eb = enc_dims(d, host_len[b]);
                if (eb.T < 1) return si_fail(ctx, SI_EINVAL, "ragged batch: clip %d (%d samples) is shorter than the conv stack's receptive field", b, host_len[b]);
                for (int i = 0; i <= d.num_conv; ++i) t[(size_t)i * B + b] = eb.L[i];
                t[off + b] = (int32_t)rows_packed;
                rows_packed += eb.T;
                sum_t2 += (double)eb.T * eb.T;
            }
            t[off + B] = (int32_t)rows_packed;
            return SI_OK;
        })) return trc;
        valid_len = tab.dev;                                 // the statistics and loaders of conv0 stop at each clip's own samples
    }
    auto dL = [&](int i) { return tab.dev + (size_t)i * B; };          // device / host rows of conv layer i's output (0: samples)
    auto hL = [&](int i) { return tab.host + (size_t)i * B; };
    const int32_t* d_rowoff = vl ? dL(d.num_conv + 1) : nullptr;
    const long BT = vl ? rows_packed : (long)B * T;          // transformer rows
    double* stats = reinterpret_cast<double*>(W.bytes((size_t)B * 16, "stats"));
    int32_t* vframes = (valid_len && !vl) ? reinterpret_cast<int32_t*>(W.bytes((size_t)B * 4, "vframes")) : nullptr;
    double* partials = reinterpret_cast<double*>(W.bytes(si_conv0_partials_bytes(B, N), "partials"));
    float* affine = W.floats((size_t)B * d.conv_dim[0] * 2, "affine");
    float* cbuf[2] = {W.floats((size_t)B * cmax, "cbuf0"), W.floats((size_t)B * cmax, "cbuf1")};
    const bool c16 = ctx->opt_enc_opready && d.encoder_math == SI_MATH_BF16 && !d.feat_norm_layer && d.num_conv >= 2;
    unsigned short* cb16[2] = {reinterpret_cast<unsigned short*>(cbuf[0]), reinterpret_cast<unsigned short*>(cbuf[1])};   // same storage, bf16 view
    float* lnf = W.floats(BT * CF, "lnf");
    float* h = W.floats(BT * H, "h");
    float* h2 = W.floats(BT * H, "h2");
    float* att = W.floats(BT * H, "att");
    float* qkv = W.floats(BT * 3 * H, "qkv");
    float* ffn = W.floats(BT * I, "ffn");
    // Operand-ready bf16 activations for the encoder GEMMs (bf16 mode): LayerNorm, attention and the FFN's first GEMM
    // also / only write bf16(x) -- the rounding the consuming GEMM would apply while staging -- so the four GEMMs of a
    // layer load 2-byte operands (their dominant traffic: M = B*T rows re-read by every N-tile) and skip the
    // conversion.  Bit-identical to converting in the consumer.  SI_ENC_OPREADY=0 restores fp32 inputs.
    const bool e16 = ctx->opt_enc_opready && d.encoder_math == SI_MATH_BF16;
    unsigned short* lnf16 = e16 ? reinterpret_cast<unsigned short*>(W.bytes((size_t)BT * CF * 2, "lnf16")) : nullptr;
    unsigned short* h16 = e16 ? reinterpret_cast<unsigned short*>(W.bytes((size_t)BT * H * 2, "h16")) : nullptr;
    unsigned short* att16 = e16 ? reinterpret_cast<unsigned short*>(W.bytes((size_t)BT * H * 2, "att16")) : nullptr;
    // Post-LN layers in bf16 mode: a LayerNorm's output is read as a bf16 GEMM operand and as the fp32 residual of the second GEMM
    // behind it.  The fp32 copy (19.5 MB per launch at the bench shape, 4.7 of the LayerNorm's 14.4 us) is not written: the
    // LayerNorm stores (mean, rstd) per row and the residual-adding epilogue recomputes the element from the row it was
    // normalised from -- the SAME expression on the same floats (si_ln_apply), so the values do not change.  The pre-LN sums then
    // live in ONE buffer that out-proj / FFN2 update in place (each element is read and written by the same lane).
    // SI_ENC_LNFUSE=0, debug captures, fp32 mode or a width the bf16 GEMM kernels do not cover: every LayerNorm writes its rows.
    const bool ln_fuse = e16 && ctx->opt_ln_fuse && ctx->opt_enc_lingemm && !d.stable_layer_norm && ctx->dbg_capture.empty() && H % 128 == 0 && I % 64 == 0 &&
                         (double)(BT + 128) * (I + 128) * 2.0 < 2.0e9;
    float* ln_stats = ln_fuse ? W.floats(BT * 2, "ln_stats") : nullptr;
    const int ffn_ld = e16 ? I + ctx->opt_ffn_pad : I;                 // row stride of the bf16 FFN intermediate (SI_ENC_FFNPAD)
    unsigned short* ffn16 = e16 ? reinterpret_cast<unsigned short*>(W.bytes((size_t)BT * ffn_ld * 2, "ffn16")) : nullptr;
    if (!W.ok) return si_fail(ctx, SI_ENOMEM, "internal: encoder workspace carve exceeded its own estimate at region '%s'", W.failed);
    // bf16 mode with the bf16-MFMA attention: the QKV GEMM writes q | k | v as bf16 only (the rounding the attention
    // kernel's staging would apply), into the storage of the fp32 matrix
    const bool qkv_bf16 = e16 && ctx->opt_att_bf16;
    unsigned short* qkv16 = reinterpret_cast<unsigned short*>(qkv);

    int rc;
    // A convolution of the encoder on (B, Lin, groups * Cin) -> (B, M, groups * N); ragged: clip b reads row li of the length table
    // and writes row lo (modeling_hubert.py:664-677).  Operands, stride / padding and the epilogue are the caller's.
    auto enc_conv = [&](const GemmW& G, int Lin, int M, int li, int lo) {
        TapGemmParams p = gemm_params(ctx, G);
        p.nseg = B; p.Lin = Lin; p.M = M; p.ldx = G.groups * G.Cin; p.x_seg_stride = (long)Lin * p.ldx;
        p.ldo = G.groups * G.N; p.o_seg_stride = (long)M * p.ldo; p.olimit = p.o_seg_stride;
        if (vl) {
            p.seg_lin = dL(li); p.seg_m = dL(lo); p.seg_orows = dL(lo); p.olim_mul = p.ldo; p.seg_m_host = hL(lo);
            double rows = 0; for (int b = 0; b < B; ++b) rows += hL(lo)[b];
            p.algo_macs = rows * p.ldo * (double)G.Cin * G.ntaps;
        }
        return p;
    };
    // A0 + A1: normalise fused into conv0
    WaveNormParams wp{wav, mask_start, mask_len, B, N, e.L[1], d.conv_dim[0], d.conv_kernel[0], d.conv_stride[0], normalize, valid_len, norm_eps, pre_add,
                      vl ? dL(1) : nullptr};
    if ((rc = si_launch_wave_stats(ctx, wp, stats, st, spans))) return rc;
    if (vframes && (rc = si_launch_frame_lengths(ctx, valid_len, B, d.num_conv, d.conv_kernel, d.conv_stride, e.T, vframes, st))) return rc;
    // layer-norm flavour (HuBERT-large) in bf16 mode: every conv is followed by LayerNorm + GELU over its 512 channels; the
    // LayerNorm writes ONLY the bf16 operand of the next conv (the rounding that conv would apply while staging), into the
    // other buffer (its bf16 rows would overlap unread fp32 rows of its own input), so that the convolutions run on the
    // dedicated bf16 GEMM kernels (gemmcu / lingemm) like the group-norm flavour's; the last one writes the fp32 features.
    const bool l16 = ctx->opt_enc_opready && d.encoder_math == SI_MATH_BF16 && d.feat_norm_layer && d.num_conv >= 2;
    const long n0 = (long)B * e.L[1] * d.conv_dim[0];
    if (!d.feat_norm_layer) {
        // group-norm flavour in bf16 mode: the conv chain runs on operand-ready bf16 activations (conv0 and convs 1..n-2
        // write ONLY the bf16 operand of their single consumer; the last conv writes fp32 for the LayerNorm that follows)
        rc = si_launch_conv0_groupnorm(ctx, wp, stats, wf(ctx, L.conv0_w), wf(ctx, L.conv0_g), wf(ctx, L.conv0_b), partials, affine, cbuf[0], st,
                                       c16 ? cb16[0] : nullptr, spans);
        if (!rc) rc = c16 ? si_tap(ctx, st, {cb16[0], n0, 2}, "conv%d.bf16", 0) : si_tap(ctx, st, {cbuf[0], n0}, "conv%d", 0);
    } else {
        rc = si_launch_conv0_affine(ctx, wp, stats, wf(ctx, L.conv0_w), d.conv_bias ? wf(ctx, L.conv0_bias) : nullptr, affine, cbuf[0], st, spans);
        if (!rc) rc = si_tap(ctx, st, {cbuf[0], n0}, "conv%d", 0);
        if (!rc) rc = si_launch_layernorm(ctx, cbuf[0], nullptr, wf(ctx, L.conv0_g), wf(ctx, L.conv0_b), l16 ? nullptr : cbuf[0], (long)B * e.L[1], d.conv_dim[0],
                                          1e-5f, 1, st, l16 ? cb16[1] : nullptr);
        if (!rc) rc = l16 ? si_tap(ctx, st, {cb16[1], n0, 2}, "conv%d.ln.bf16", 0) : si_tap(ctx, st, {cbuf[0], n0}, "conv%d.ln", 0);
    }
    if (rc) return rc;
    // A2: strided convs as tap-GEMMs
    int cur = 0;
    for (int i = 1; i < d.num_conv; ++i) {
        const ConvW& c = L.convs[i - 1];
        TapGemmParams p = enc_conv(c.g, e.L[i], e.L[i + 1], i, i + 1);
        p.x = cbuf[cur]; p.out = cbuf[cur ^ 1];
        if (c16) {
            p.x = nullptr; p.x16 = cb16[cur];
            if (i + 1 < d.num_conv) { p.out = nullptr; p.out16 = cb16[cur ^ 1]; p.out16_slope = 1.f; }
        }
        if (l16) { p.x = nullptr; p.x16 = cb16[1]; p.out = cbuf[0]; }          // bf16 in from buffer 1, fp32 out to buffer 0
        p.stride = d.conv_stride[i];
        p.act = d.feat_norm_layer ? SI_ACT_NONE : SI_ACT_GELU;
        p.lingemm = ctx->opt_enc_lingemm;
        if ((rc = si_launch_tapgemm(ctx, c.g.math, p, st))) return rc;
        const long ni = (long)B * e.L[i + 1] * d.conv_dim[i];            // (B, L_{i+1}, C_i); ragged: rows past a clip's own L are stale
        if ((rc = p.out ? si_tap(ctx, st, {p.out, ni}, "conv%d", i) : si_tap(ctx, st, {p.out16, ni, 2}, "conv%d.bf16", i))) return rc;
        if (l16) {
            const bool last = i + 1 == d.num_conv;
            if ((rc = si_launch_layernorm(ctx, cbuf[0], nullptr, wf(ctx, c.ln_g), wf(ctx, c.ln_b), last ? cbuf[1] : nullptr, (long)B * e.L[i + 1], d.conv_dim[i],
                                          1e-5f, 1, st, last ? nullptr : cb16[1])))
                return rc;
            if ((rc = last ? si_tap(ctx, st, {cbuf[1], ni}, "conv%d.ln", i) : si_tap(ctx, st, {cb16[1], ni, 2}, "conv%d.ln.bf16", i))) return rc;
            cur = 1;
            continue;
        }
        cur ^= 1;
        if (d.feat_norm_layer) {
            if ((rc = si_launch_layernorm(ctx, cbuf[cur], nullptr, wf(ctx, c.ln_g), wf(ctx, c.ln_b), cbuf[cur], (long)B * e.L[i + 1], d.conv_dim[i], 1e-5f, 1, st)))
                return rc;
            if ((rc = si_tap(ctx, st, {cbuf[cur], ni}, "conv%d.ln", i))) return rc;
        }
    }
    const float* feat = cbuf[cur];                                   // (B, T, CF)
    if (vl) {                                                        // -> packed rows (sum of T_b, CF): everything behind is row-wise
        if ((rc = si_launch_repack_rows(ctx, cbuf[cur], cbuf[cur ^ 1], B, T, CF, d_rowoff, false, st))) return rc;
        feat = cbuf[cur ^ 1];
    }
    if ((rc = si_tap(ctx, st, {feat, BT * CF}, "features"))) return rc;
    // A3: LN + projection
    LinearIo proj_io;
    if (d.feat_proj_layer_norm) {
        // (bf16 mode: the projection reads the bf16 operand only)
        if ((rc = si_launch_layernorm(ctx, feat, nullptr, wf(ctx, L.fp_ln_g), wf(ctx, L.fp_ln_b), lnf16 ? nullptr : lnf, BT, CF, d.layer_norm_eps, 0, st, lnf16))) return rc;
        proj_io.x16 = lnf16;
        // (per-op tap: named and looked up only while some capture is registered)
        if (!ctx->dbg_capture.empty() &&
            (rc = lnf16 ? si_tap(ctx, st, {lnf16, BT * CF, 2}, "features.ln.bf16") : si_tap(ctx, st, {lnf, BT * CF}, "features.ln"))) return rc;
    }
    if ((rc = linear(ctx, L.proj, d.feat_proj_layer_norm ? lnf : feat, h, BT, SI_ACT_NONE, nullptr, st, proj_io))) return rc;
    if ((rc = si_tap(ctx, st, {h, BT * H}, "projected"))) return rc;
    // right-padded batches: padded frames of the projected states are zeroed before the positional conv and excluded
    // as attention keys (modeling_hubert.py:428-437 / 573-582)
    if (vframes && (rc = si_launch_zero_padded_rows(ctx, h, B, T, H, vframes, st))) return rc;
    // A4: h2 = h + gelu(pos_conv(h) + b)
    bool pos_done = false;
    if (d.encoder_math == SI_MATH_BF16 && ctx->opt_enc_posconv && L.pos.has_bias) {
        // the dedicated kernel (posconv.hip): N = the group's own width, the group's weights once per workgroup
        const int prc = si_launch_posconv(ctx, h, h2, ctx->wdev + L.pos.w, wf(ctx, L.pos.bias), B, T, T, H, d.pos_conv_groups, d.pos_conv_kernel,
                                          L.pos.Npad, d.pos_conv_kernel / 2, d_rowoff, vl ? dL(d.num_conv) : nullptr, (double)BT, st);
        if (prc < 0) return prc;
        pos_done = prc == 0;
    }
    if (!pos_done) {
        TapGemmParams p = enc_conv(L.pos, T, T, d.num_conv, d.num_conv);
        p.x = h; p.out = h2; p.res = h;
        p.pad = d.pos_conv_kernel / 2;
        p.act = SI_ACT_GELU;
        if (vl) p.seg_row_off = d_rowoff;                    // packed rows: the conv's zero padding begins at each clip's own last frame
        if ((rc = si_launch_tapgemm(ctx, L.pos.math, p, st))) return rc;
    }
    if (!ctx->dbg_capture.empty() && (rc = si_tap(ctx, st, {h2, BT * H}, "pos_conv"))) return rc;   // (per-op tap, before the encoder LayerNorm)
    const float eps = d.layer_norm_eps;
    ResLn cur_ln;                                                      // ln_fuse: the LayerNorm whose (unwritten) output is the current hidden state
    // LayerNorm of the transformer rows: fp32 rows to y and / or their bf16 operand to y16; ln_fuse: (mean, rstd) per row for cur_ln
    auto norm = [&](const float* x, size_t gamma, size_t beta, float* y, unsigned short* y16 = nullptr) {
        if (ln_fuse) cur_ln = ResLn{ln_stats, wf(ctx, gamma), wf(ctx, beta)};
        return si_launch_layernorm(ctx, x, nullptr, wf(ctx, gamma), wf(ctx, beta), y, BT, H, eps, 0, st, y16, ln_stats);
    };
    if (!d.stable_layer_norm) {
        if ((rc = norm(h2, L.enc_ln_g, L.enc_ln_b, ln_fuse ? nullptr : h, h16))) return rc;
    } else {
        std::swap(h, h2);
    }
    if ((rc = si_tap(ctx, st, {h, BT * H}, "encoder_in"))) return rc;
    // A5..A8.  The optional operands of a layer's four GEMMs (bf16 mode: each reads the operand-ready copy its producer wrote; the
    // rows of the FFN intermediate are ffn_ld apart); ln_fuse adds the LayerNorm residual of the moment to out-proj's and FFN2's.
    const long nh = BT * H;
    LinearIo qkv_io, out_io, ffn1_io, ffn2_io;
    qkv_io.x16 = h16; qkv_io.y16 = qkv_bf16 ? qkv16 : nullptr;
    out_io.x16 = att16;
    ffn1_io.x16 = h16; ffn1_io.y16 = ffn16; ffn1_io.ld_out = ffn_ld;
    ffn2_io.x16 = ffn16; ffn2_io.ld_in = ffn_ld;
    // (taps of a layer: no-ops unless a capture is registered; captures also turn ln_fuse off)
    // q | k | v of layer l from x (bf16 mode: from h16 = bf16(x)), then the attention into att / att16
    auto attention = [&](int l, const float* x) -> int {
        int r;
        if (e16 && (r = si_tap(ctx, st, {h16, nh, 2}, "layer%d.h.bf16", l))) return r;
        if ((r = linear(ctx, L.layers[l].qkv, x, qkv_bf16 ? nullptr : qkv, BT, SI_ACT_NONE, nullptr, st, qkv_io))) return r;
        if (qkv_bf16) r = si_launch_attention_bf16in(ctx, qkv16, B, T, H, d.num_heads, st, att16, vframes, d_rowoff, sum_t2);
        else r = si_launch_attention(ctx, qkv, att, B, T, H, d.num_heads, st, att16, ctx->opt_att_bf16, vframes, d_rowoff, sum_t2);
        if (!r) r = qkv_bf16 ? si_tap(ctx, st, {qkv16, 3 * nh, 2}, "layer%d.qkv.bf16", l) : si_tap(ctx, st, {qkv, 3 * nh}, "layer%d.qkv", l);
        if (!r) r = att16 ? si_tap(ctx, st, {att16, nh, 2}, "layer%d.att.bf16", l) : si_tap(ctx, st, {att, nh}, "layer%d.att", l);
        return r;
    };
    // the FFN's first GEMM of layer l on x (bf16 mode: on h16, writing the bf16 intermediate only)
    auto ffn1 = [&](int l, const float* x) -> int {
        if (int r = linear(ctx, L.layers[l].ffn1, x, e16 ? nullptr : ffn, BT, SI_ACT_GELU, nullptr, st, ffn1_io)) return r;
        return e16 ? si_tap(ctx, st, {ffn16, BT * I, 2, I, ffn_ld}, "layer%d.ffn.bf16", l) : si_tap(ctx, st, {ffn, BT * I}, "layer%d.ffn", l);
    };
    for (int l = 0; l < d.num_layers; ++l) {
        const LayerW& Wl = L.layers[l];
        if ((rc = si_tap(ctx, st, {h, nh}, "layer%d.h", l))) return rc;
        if (!d.stable_layer_norm && ln_fuse) {   // post-LN (modeling_hubert.py:371-404) with recomputed LayerNorm residuals
            // h2 holds the rows the current hidden state was normalised FROM; out-proj / FFN2 add their residual LayerNorm(h2)
            // from it and write the next pre-LN sum over it.  The last layer's (or the asked-for layer's) output is written.
            const bool want_rows = l + 1 == d.num_layers || output_layer == l + 1;
            if ((rc = attention(l, h))) return rc;
            out_io.res_ln = cur_ln;
            if ((rc = linear(ctx, Wl.out, att, h2, BT, SI_ACT_NONE, h2, st, out_io))) return rc;
            if ((rc = norm(h2, Wl.ln1_g, Wl.ln1_b, nullptr, h16))) return rc;
            if ((rc = ffn1(l, h))) return rc;
            ffn2_io.res_ln = cur_ln;
            if ((rc = linear(ctx, Wl.ffn2, ffn, h2, BT, SI_ACT_NONE, h2, st, ffn2_io))) return rc;
            if ((rc = norm(h2, Wl.ln2_g, Wl.ln2_b, want_rows ? h : nullptr, h16))) return rc;
        } else if (!d.stable_layer_norm) {       // post-LN, every LayerNorm written; h16 = bf16(h) when e16
            if ((rc = attention(l, h))) return rc;
            if ((rc = linear(ctx, Wl.out, att, h2, BT, SI_ACT_NONE, h, st, out_io))) return rc;
            if ((rc = si_tap(ctx, st, {h2, nh}, "layer%d.att_res", l))) return rc;
            if ((rc = norm(h2, Wl.ln1_g, Wl.ln1_b, h, h16))) return rc;
            if ((rc = si_tap(ctx, st, {h, nh}, "layer%d.ln1", l)) || (e16 && (rc = si_tap(ctx, st, {h16, nh, 2}, "layer%d.ln1.bf16", l)))) return rc;
            if ((rc = ffn1(l, h))) return rc;
            if ((rc = linear(ctx, Wl.ffn2, ffn, h2, BT, SI_ACT_NONE, h, st, ffn2_io))) return rc;
            if ((rc = si_tap(ctx, st, {h2, nh}, "layer%d.ffn_res", l))) return rc;
            if ((rc = norm(h2, Wl.ln2_g, Wl.ln2_b, h, h16))) return rc;
            if ((rc = si_tap(ctx, st, {h, nh}, "layer%d.ln2", l)) || (e16 && (rc = si_tap(ctx, st, {h16, nh, 2}, "layer%d.ln2.bf16", l)))) return rc;
        } else {                                 // pre-LN "stable" (modeling_hubert.py:504-547); residual adds are in place
            // (bf16 mode: the normalised rows feed GEMMs only -- their bf16 operand is all that is written)
            if ((rc = norm(h, Wl.ln1_g, Wl.ln1_b, e16 ? nullptr : h2, h16))) return rc;
            if ((rc = e16 ? si_tap(ctx, st, {h16, nh, 2}, "layer%d.ln1.bf16", l) : si_tap(ctx, st, {h2, nh}, "layer%d.ln1", l))) return rc;
            if ((rc = attention(l, h2))) return rc;
            if ((rc = linear(ctx, Wl.out, att, h, BT, SI_ACT_NONE, h, st, out_io))) return rc;
            if ((rc = si_tap(ctx, st, {h, nh}, "layer%d.att_res", l))) return rc;
            if ((rc = norm(h, Wl.ln2_g, Wl.ln2_b, e16 ? nullptr : h2, h16))) return rc;
            if ((rc = e16 ? si_tap(ctx, st, {h16, nh, 2}, "layer%d.ln2.bf16", l) : si_tap(ctx, st, {h2, nh}, "layer%d.ln2", l))) return rc;
            if ((rc = ffn1(l, h2))) return rc;
            if ((rc = linear(ctx, Wl.ffn2, ffn, h, BT, SI_ACT_NONE, h, st, ffn2_io))) return rc;
            if ((rc = si_tap(ctx, st, {h, nh}, "layer%d.ffn_res", l))) return rc;
        }
        if (output_layer == l + 1) {
            // fairseq `extract_features(output_layer = L)` (I_da/src/hubert_feature_reader.py:60-65): the loop stops after layer
            // L - 1 and returns its output; the pre-LN flavour's final LayerNorm is applied only when no layer was asked for
            SI_HIP_CHECK(hipMemcpyAsync(out_hidden, h, (size_t)BT * H * sizeof(float), hipMemcpyDeviceToDevice, st));
            return SI_OK;
        }
    }
    if (d.stable_layer_norm) {
        if ((rc = norm(h, L.enc_ln_g, L.enc_ln_b, h2))) return rc;
        std::swap(h, h2);
    }
    if ((rc = si_tap(ctx, st, {h, BT * H}, "last_hidden"))) return rc;
    // A9: final_layers = LN -> Linear(H, codebook_dim), always fp32
    if ((rc = si_launch_layernorm(ctx, h, nullptr, wf(ctx, L.head_ln_g), wf(ctx, L.head_ln_b), h2, BT, H, 1e-5f, 0, st))) return rc;
    if (!vl) return linear(ctx, L.head, h2, out_feats, BT, SI_ACT_NONE, nullptr, st);
    // ragged batch: the head on the packed rows (into the dead q|k|v storage), then out to (B, T, D) with zero rows past each clip
    if ((rc = linear(ctx, L.head, h2, qkv, BT, SI_ACT_NONE, nullptr, st))) return rc;
    return si_launch_repack_rows(ctx, qkv, out_feats, B, T, d.codebook_dim, d_rowoff, true, st);
}

// What the seven si_codebook_* entry points require before they launch: a context whose weights are loaded and -- for a blob that was
// received, not read -- verified; `args_ok`, the call's own NULL / empty check; for a call that writes a mel, centroids as wide as the
// generator's input.  Selects the context's device.
static int codebook_enter(si_ctx* ctx, const char* call, bool args_ok, bool writes_mel) {
    if (!ctx) return SI_EINVAL;
    if (!ctx->weights_ready) return si_fail(ctx, SI_ESTATE, "%s before weights were loaded", call);
    if (!ctx->weights_verified) if (int rcw = si_weights_check(ctx)) return rcw;
    if (!args_ok) return si_fail(ctx, SI_EINVAL, "%s: NULL / empty argument", call);
    if (writes_mel && ctx->d.codebook_dim != ctx->d.num_mels)
        return si_fail(ctx, SI_EINVAL, "codebook_dim %d != generator input width %d: centroids are not frames of this generator's input",
                       ctx->d.codebook_dim, ctx->d.num_mels);
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return SI_OK;
}

static int codebook_splice(si_ctx* ctx, const float* feats, int B, int T, const si_cb_frames& fr, float* mel, int Tm, int64_t* labels,
                           si_stream_t stream) {
    const Layout& L = ctx->lay;
    return si_launch_codebook_splice(ctx, feats, B, T, ctx->d.codebook_dim, fr, wf(ctx, L.cb_centered), wf(ctx, L.cb_raw), wf(ctx, L.cb_rnorm),
                                     ctx->d.num_clusters, mel, Tm, labels, static_cast<hipStream_t>(stream));
}

static int codebook_gather(si_ctx* ctx, const int64_t* labels, int B, const si_cb_frames& fr, float* mel, int Tm, si_stream_t stream) {
    return si_launch_codebook_gather(ctx, labels, B, ctx->d.codebook_dim, fr, wf(ctx, ctx->lay.cb_raw), ctx->d.num_clusters, mel, Tm,
                                     static_cast<hipStream_t>(stream));
}

static int codebook_metrics(si_ctx* ctx, const float* feats, int B, int T, const si_cb_frames& fr, const int64_t* target_labels,
                            float* loss_terms, float* loss, int64_t* pred_labels, float* cos_pred_target, si_stream_t stream) {
    const Layout& L = ctx->lay;
    return si_launch_codebook_metrics(ctx, feats, B, T, ctx->d.codebook_dim, fr, wf(ctx, L.cb_centered), wf(ctx, L.cb_rnorm), ctx->d.num_clusters,
                                      target_labels, loss_terms, loss, pred_labels, cos_pred_target, static_cast<hipStream_t>(stream));
}

extern "C" {

int si_codebook_splice(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_pos, int Lm, float* mel, int Tm,
                       int64_t* labels, si_stream_t stream) {
    if (int rc = codebook_enter(ctx, "si_codebook_splice", feats && frame_pos && mel && B > 0 && Lm >= 0, true)) return rc;
    return codebook_splice(ctx, feats, B, T, si_cb_frames::grid(frame_pos, Lm), mel, Tm, labels, stream);
}

int si_codebook_splice_varlen(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_pos, const int32_t* frame_cnt, int Lm,
                              float* mel, int Tm, int64_t* labels, si_stream_t stream) {
    if (int rc = codebook_enter(ctx, "si_codebook_splice_varlen", feats && frame_pos && frame_cnt && mel && B > 0 && Lm >= 0, true)) return rc;
    return codebook_splice(ctx, feats, B, T, si_cb_frames::grid(frame_pos, Lm, frame_cnt), mel, Tm, labels, stream);
}

int si_codebook_splice_spans(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_clip, const int32_t* frame_pos, int F,
                             float* mel, int Tm, int64_t* labels, si_stream_t stream) {
    const bool args_ok = feats && mel && B > 0 && T > 0 && Tm > 0 && F >= 0 && (F == 0 || (frame_clip && frame_pos));
    if (int rc = codebook_enter(ctx, "si_codebook_splice_spans", args_ok, true)) return rc;
    return codebook_splice(ctx, feats, B, T, si_cb_frames::of_table(frame_clip, frame_pos, F), mel, Tm, labels, stream);
}

int si_codebook_splice_labels(si_ctx* ctx, const int64_t* labels, int B, const int32_t* frame_pos, int Lm, float* mel, int Tm,
                              si_stream_t stream) {
    if (int rc = codebook_enter(ctx, "si_codebook_splice_labels", labels && frame_pos && mel && B > 0 && Lm >= 0, true)) return rc;
    return codebook_gather(ctx, labels, B, si_cb_frames::grid(frame_pos, Lm), mel, Tm, stream);
}

int si_codebook_splice_labels_spans(si_ctx* ctx, const int64_t* labels, int B, const int32_t* frame_clip, const int32_t* frame_pos, int F,
                                    float* mel, int Tm, si_stream_t stream) {
    const bool args_ok = mel && B > 0 && Tm > 0 && F >= 0 && (F == 0 || (labels && frame_clip && frame_pos));
    if (int rc = codebook_enter(ctx, "si_codebook_splice_labels_spans", args_ok, true)) return rc;
    return codebook_gather(ctx, labels, B, si_cb_frames::of_table(frame_clip, frame_pos, F), mel, Tm, stream);
}

int si_codebook_metrics(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_pos, int Lm,
                        const int64_t* target_labels, float* loss_terms, float* loss, int64_t* pred_labels, float* cos_pred_target,
                        si_stream_t stream) {
    const bool args_ok = feats && frame_pos && target_labels && loss_terms && loss && cos_pred_target && B > 0 && Lm > 0;
    if (int rc = codebook_enter(ctx, "si_codebook_metrics", args_ok, false)) return rc;
    return codebook_metrics(ctx, feats, B, T, si_cb_frames::grid(frame_pos, Lm), target_labels, loss_terms, loss, pred_labels, cos_pred_target,
                            stream);
}

int si_codebook_metrics_spans(si_ctx* ctx, const float* feats, int B, int T, const int32_t* frame_clip, const int32_t* frame_pos, int F,
                              const int64_t* target_labels, float* loss_terms, float* loss, int64_t* pred_labels, float* cos_pred_target,
                              si_stream_t stream) {
    const bool args_ok = feats && frame_clip && frame_pos && target_labels && loss_terms && loss && cos_pred_target && B > 0 && T > 0 && F > 0;
    if (int rc = codebook_enter(ctx, "si_codebook_metrics_spans", args_ok, false)) return rc;
    return codebook_metrics(ctx, feats, B, T, si_cb_frames::of_table(frame_clip, frame_pos, F), target_labels, loss_terms, loss, pred_labels,
                            cos_pred_target, stream);
}

int si_kmeans_assign(si_ctx* ctx, const float* feats, int64_t rows, int D, const float* centroids, int K, int64_t* labels,
                     float* sq_dist, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!feats || !centroids || !labels || rows < 0) return si_fail(ctx, SI_EINVAL, "si_kmeans_assign: NULL / bad argument");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    if (K > ctx->km_cnorm_cap) {                                       // (a context is single-threaded and its calls stream-ordered by contract)
        if (ctx->km_cnorm) { SI_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream))); SI_HIP_CHECK(hipFree(ctx->km_cnorm)); ctx->km_cnorm = nullptr; ctx->km_cnorm_cap = 0; }
        const int cap = std::max(K, 1024);
        SI_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx->km_cnorm), (size_t)cap * sizeof(float)));
        ctx->km_cnorm_cap = cap;
    }
    const bool mfma = !(getenv("SI_KMEANS_MFMA") && atoi(getenv("SI_KMEANS_MFMA")) == 0);   // (read per call: the test compares both kernels)
    return si_launch_kmeans_assign(ctx, feats, (long)rows, D, centroids, K, labels, sq_dist, static_cast<hipStream_t>(stream),
                                   mfma ? ctx->km_cnorm : nullptr);
}

int si_mel_metrics(si_ctx* ctx, const float* mel_a, const float* mel_b, int B, int D, int L, const float* center, float* out3,
                   si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!mel_a || !mel_b || !out3) return si_fail(ctx, SI_EINVAL, "si_mel_metrics: NULL argument");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_mel_metrics(ctx, mel_a, mel_b, B, D, L, center, out3, static_cast<hipStream_t>(stream));
}

int si_sisdr(si_ctx* ctx, const float* est, const float* ref, int B, int n, float* out, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!est || !ref || !out) return si_fail(ctx, SI_EINVAL, "si_sisdr: NULL argument");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_sisdr(ctx, est, ref, B, n, out, static_cast<hipStream_t>(stream));
}

// ---- F0 VQ-VAE encoder (row f-2): I_da/src/model.py:160-163 runs `self.fo_vqvae.encoder(fo)` -- jukebox.py `Encoder` with one
//      level = `EncoderConvBlock` (:11-116): down_t x [Conv1d(k = 2 s, stride s, pad s / 2) + Resnet1D(depth blocks of
//      x + Conv1(ReLU(Conv3_dil(ReLU(x)))), dilation growth^j, resnet.py:29-97)] + Conv1d(width -> out, 3, 1, 1).
namespace {
struct F0Shape { int k, pad; };
F0Shape f0_down_shape(int s) { return (s % 2 == 0) ? F0Shape{2 * s, s / 2} : F0Shape{2 * s + 1, s / 2 + 1}; }   // jukebox.py:54-57
bool f0_desc_ok(const si_f0enc_desc* d) {
    return d && d->in_width >= 1 && d->out_width >= 1 && d->width >= 1 && d->n_state >= 1 && d->depth >= 0 && d->down_t >= 1 && d->stride_t >= 1 &&
           d->dilation_growth >= 1 && d->down_t <= 16 && d->depth <= 32;
}
}  // namespace

size_t si_f0_encoder_weight_floats(const si_f0enc_desc* d) {
    if (!f0_desc_ok(d)) return 0;
    const F0Shape ds = f0_down_shape(d->stride_t);
    size_t n = 0;
    for (int i = 0; i < d->down_t; ++i) {
        n += (size_t)d->width * (i == 0 ? d->in_width : d->width) * ds.k + d->width;
        n += (size_t)d->depth * ((size_t)d->n_state * d->width * 3 + d->n_state + (size_t)d->width * d->n_state + d->width);
    }
    return n + (size_t)d->out_width * d->width * 3 + d->out_width;
}

int si_f0_encoder_frames(const si_f0enc_desc* d, int T) {
    if (!f0_desc_ok(d) || T <= 0) return 0;
    const F0Shape ds = f0_down_shape(d->stride_t);
    for (int i = 0; i < d->down_t; ++i) {
        if (T + 2 * ds.pad < ds.k) return 0;                           // (torch's Conv1d raises: the padded input is shorter than the kernel)
        T = (T + 2 * ds.pad - ds.k) / d->stride_t + 1;
    }
    return T;
}

size_t si_f0_encoder_workspace_bytes(const si_f0enc_desc* d, int B, int T) {
    if (!f0_desc_ok(d) || B <= 0 || T <= 0) return 0;
    const F0Shape ds = f0_down_shape(d->stride_t);
    const int T1 = (T + 2 * ds.pad - ds.k) / d->stride_t + 1;          // the longest intermediate
    const size_t c = (size_t)std::max(d->width, d->n_state);
    return 3 * ((size_t)B * c * std::max(T1, 1) * sizeof(float) + 256);
}

int si_f0_encoder_forward(si_ctx* ctx, const si_f0enc_desc* d, const float* weights, const float* f0, int B, int T, float* h_out,
                          void* workspace, size_t workspace_bytes, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!f0_desc_ok(d)) return si_fail(ctx, SI_EINVAL, "si_f0_encoder_forward: bad descriptor");
    if (!weights || !f0 || !h_out || !workspace || B <= 0 || T <= 0) return si_fail(ctx, SI_EINVAL, "si_f0_encoder_forward: NULL / empty argument");
    if (si_f0_encoder_frames(d, T) <= 0) return si_fail(ctx, SI_EINVAL, "si_f0_encoder_forward: %d frames are too few for %d stride-%d convolutions", T, d->down_t, d->stride_t);
    const size_t need = si_f0_encoder_workspace_bytes(d, B, T);
    if (workspace_bytes < need) return si_fail(ctx, SI_ENOMEM, "workspace of %zu bytes < %zu needed", workspace_bytes, need);
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const F0Shape ds = f0_down_shape(d->stride_t);
    {
        // one persistent launch with the track's activations in LDS (bit-identical to the layer-by-layer form below, which
        // remains for tracks too long for LDS); SI_F0_FUSED=0 forces the latter (the test compares the two)
        const bool fused_on = !(getenv("SI_F0_FUSED") && atoi(getenv("SI_F0_FUSED")) == 0);   // (read per call: the test flips it in-process)
        if (fused_on) {
            double macs = 0;
            int Tc = T, cin = d->in_width;
            for (int i = 0; i < d->down_t; ++i) {
                const int To = (Tc + 2 * ds.pad - ds.k) / d->stride_t + 1;
                macs += (double)B * To * d->width * (double)cin * ds.k + (double)d->depth * B * To * ((double)d->n_state * d->width * 3 + (double)d->width * d->n_state);
                Tc = To; cin = d->width;
            }
            macs += (double)B * Tc * d->out_width * (double)d->width * 3;
            const int frc = si_launch_f0enc_fused(ctx, weights, f0, B, T, h_out, d->in_width, d->out_width, d->width, d->n_state, d->depth, d->down_t,
                                                  d->stride_t, d->dilation_growth, ds.k, ds.pad, macs, st);
            if (frc <= 0) return frc;
        }
    }
    const size_t slot = need / 3 / sizeof(float);
    float* buf[3] = {static_cast<float*>(workspace), static_cast<float*>(workspace) + slot, static_cast<float*>(workspace) + 2 * slot};
    const float* w = weights;
    const float* x = f0;                                               // (B, in_width, T)
    int cin = d->in_width, Tc = T, cur = -1;
    int rc;
    for (int i = 0; i < d->down_t; ++i) {
        const int To = (Tc + 2 * ds.pad - ds.k) / d->stride_t + 1;
        const float* cw = w; w += (size_t)d->width * cin * ds.k;
        const float* cb = w; w += d->width;
        const int o = (cur + 1) % 3;
        if ((rc = si_launch_small_conv1d(ctx, x, cw, cb, nullptr, buf[o], B, cin, Tc, d->width, To, ds.k, d->stride_t, 1, ds.pad, 0, 0, st))) return rc;
        cur = o; x = buf[cur]; cin = d->width; Tc = To;
        long dil = 1;
        for (int j = 0; j < d->depth; ++j) {
            const float* w3 = w; w += (size_t)d->n_state * d->width * 3;
            const float* b3 = w; w += d->n_state;
            const float* w1 = w; w += (size_t)d->width * d->n_state;
            const float* b1 = w; w += d->width;
            const int t1 = (cur + 1) % 3, t2 = (cur + 2) % 3;
            if ((rc = si_launch_small_conv1d(ctx, x, w3, b3, nullptr, buf[t1], B, d->width, Tc, d->n_state, Tc, 3, 1, (int)dil, (int)dil, 1, 0, st))) return rc;
            if ((rc = si_launch_small_conv1d(ctx, buf[t1], w1, b1, x, buf[t2], B, d->n_state, Tc, d->width, Tc, 1, 1, 1, 0, 1, 0, st))) return rc;
            cur = t2; x = buf[cur];
            dil *= d->dilation_growth;
            if (dil > (1 << 20)) return si_fail(ctx, SI_EINVAL, "si_f0_encoder_forward: dilation overflow");
        }
    }
    const float* fw = w; w += (size_t)d->out_width * d->width * 3;
    return si_launch_small_conv1d(ctx, x, fw, w, nullptr, h_out, B, d->width, Tc, d->out_width, Tc, 3, 1, 1, 1, 0, 1, st);
}

int si_unit_frontend(si_ctx* ctx, const int64_t* code, int Fc, const int64_t* f0_code, int Fp, const float* spk_emb, const float* emb_c,
                     int Kc, const float* emb_p, int Kp, int E, int B, float* out, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!code || !emb_c || !out || B <= 0 || Fc <= 0 || E <= 0 || Kc <= 0) return si_fail(ctx, SI_EINVAL, "si_unit_frontend: NULL / empty argument");
    if (f0_code && (!emb_p || Fp <= 0 || Kp <= 0)) return si_fail(ctx, SI_EINVAL, "si_unit_frontend: f0_code needs its embedding table");
    if (f0_code) {
        const int F = Fp > Fc ? Fp : Fc, s = Fp > Fc ? Fc : Fp;
        // `_upsample` repeats each frame F // len times and refuses anything that does not fill F (I_da/src/model.py:104-112)
        if (F % s) return si_fail(ctx, SI_EINVAL, "si_unit_frontend: %d and %d frames: misalignment between condition features", Fc, Fp);
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_unit_frontend(ctx, code, Fc, f0_code, Fp, spk_emb, emb_c, Kc, emb_p, Kp, E, B, out, static_cast<hipStream_t>(stream));
}

int si_resample_poly(si_ctx* ctx, const float* x, int B, int n_in, const float* taps, int ntaps, int up, int down,
                     int pre_remove, int n_out, float* y, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!x || !taps || !y || B <= 0 || n_in <= 0) return si_fail(ctx, SI_EINVAL, "si_resample_poly: NULL / empty argument");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_resample_poly(ctx, x, B, n_in, taps, ntaps, up, down, pre_remove, n_out, y, static_cast<hipStream_t>(stream));
}

static int hifigan_run(si_ctx* ctx, const float* mel, int B, int Tm, int stretch, float* wav_out, void* workspace,
                       size_t workspace_bytes, si_stream_t stream, const int32_t* host_len);

int si_resample_sinc(si_ctx* ctx, const float* x, const int32_t* n_len, int B, int n_in, const si_sinc_filter* f, int n_out, float* y,
                     si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!x || !y || !f || !f->win || !f->dwin || !f->time_reg || B <= 0 || n_in <= 0) return si_fail(ctx, SI_EINVAL, "si_resample_sinc: NULL / empty argument");
    if (f->struct_size != (int32_t)sizeof(si_sinc_filter)) return si_fail(ctx, SI_EINVAL, "si_resample_sinc: si_sinc_filter size mismatch");
    if (n_out > f->n_time) return si_fail(ctx, SI_EINVAL, "si_resample_sinc: %d outputs but the time-register table holds %d", n_out, f->n_time);
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_resample_sinc(ctx, x, n_len, B, n_in, f->win, f->dwin, f->nwin, f->num_table, f->step, f->scale, f->ratio, f->time_reg, n_out, y,
                                   static_cast<hipStream_t>(stream));
}

int si_extend_mel(si_ctx* ctx, const float* mel, int B, int Tm, float* out, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!mel || !out || B <= 0 || Tm <= 0) return si_fail(ctx, SI_EINVAL, "si_extend_mel: NULL / empty argument");
    const long Tout = voc_tout(Tm, 1);
    if (Tout < 1) return si_fail(ctx, SI_EINVAL, "mel of %d frames stretches to nothing", Tm);
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_extend_mel_cf(ctx, mel, B, ctx->d.num_mels, Tm, (int)Tout, out, static_cast<hipStream_t>(stream));
}

int si_pcm16(si_ctx* ctx, const float* wav, int64_t n, int16_t* out, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!wav || !out || n < 0) return si_fail(ctx, SI_EINVAL, "si_pcm16: NULL / bad argument");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_pcm16(ctx, wav, (long)n, out, static_cast<hipStream_t>(stream));
}

int si_hifigan_forward(si_ctx* ctx, const float* mel, int B, int Tm, int stretch, float* wav_out, void* workspace,
                       size_t workspace_bytes, si_stream_t stream) {
    return hifigan_run(ctx, mel, B, Tm, stretch, wav_out, workspace, workspace_bytes, stream, nullptr);
}

int si_hifigan_forward_varlen(si_ctx* ctx, const float* mel, const int32_t* mel_len, int B, int Tm, int stretch, float* wav_out, void* workspace,
                              size_t workspace_bytes, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!mel_len) return si_fail(ctx, SI_EINVAL, "si_hifigan_forward_varlen: NULL lengths");
    return hifigan_run(ctx, mel, B, Tm, stretch, wav_out, workspace, workspace_bytes, stream, mel_len);
}

// host_len (B, HOST) or null: ragged batch -- clip b holds host_len[b] mel frames of its Tm; every convolution's zero padding
// begins at the clip's OWN end, so its waveform equals that clip's alone; wav_out rows are the longest clip's, zero past each clip.
static int hifigan_run(si_ctx* ctx, const float* mel, int B, int Tm, int stretch, float* wav_out, void* workspace,
                       size_t workspace_bytes, si_stream_t stream, const int32_t* host_len) {
    if (!ctx) return SI_EINVAL;
    if (!ctx->weights_ready) return si_fail(ctx, SI_ESTATE, "si_hifigan_forward before weights were loaded");
    if (!ctx->weights_verified) if (int rcw = si_weights_check(ctx)) return rcw;
    if (!mel || !wav_out || !workspace || B <= 0 || Tm <= 0) return si_fail(ctx, SI_EINVAL, "si_hifigan_forward: NULL / empty argument");
    const si_model_desc& d = ctx->d;
    const Layout& Ly = ctx->lay;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t need = vocoder_ws_bytes(ctx, B, Tm, stretch);
    if (workspace_bytes < need) return si_fail(ctx, SI_ENOMEM, "workspace of %zu bytes < %zu needed for B=%d Tm=%d", workspace_bytes, need, B, Tm);
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    const int Bc_max = vocoder_chunk(d, B);
    const long Tout = voc_tout(Tm, stretch);
    if (Tout < 1) return si_fail(ctx, SI_EINVAL, "mel of %d frames stretches to nothing", Tm);
    size_t lc_max = (size_t)Tout * d.up_initial_channel;
    {
        long L = Tout; int c = d.up_initial_channel;
        for (int i = 0; i < d.num_ups; ++i) { L *= d.up_rates[i]; c = stage_channels(ctx, i); lc_max = std::max(lc_max, (size_t)L * c); }
    }
    const long Lwav = si_vocoder_samples(ctx, Tm, stretch);
    Carver W = carver(ctx, SI_WS_VOCODER, workspace, workspace_bytes);
    // ---- ragged batch: the table [mel frames | rows of stage 0 (stretched frames) .. stage num_ups | GEMM rows of upsampler 1 .. num_ups]
    const bool vl = host_len != nullptr;
    VlTable tab;
    if (vl) {
        if (int trc = vl_table(ctx, W, (size_t)(2 * d.num_ups + 2) * B, st, "vocoder", tab, [&](int32_t* t) -> int {
            for (int b = 0; b < B; ++b) {
                if (host_len[b] < 1 || host_len[b] > Tm) return si_fail(ctx, SI_EINVAL, "ragged batch: clip %d holds %d mel frames, outside 1..%d", b, host_len[b], Tm);
                long Lb = voc_tout(host_len[b], stretch);
                if (Lb < 1) return si_fail(ctx, SI_EINVAL, "ragged batch: clip %d (%d mel frames) stretches to nothing", b, host_len[b]);
                t[b] = host_len[b];
                t[(size_t)B + b] = (int32_t)Lb;
                for (int i = 0; i < d.num_ups; ++i) {
                    const UpsGeom g = ups_geom(d, i, Lb);
                    t[(size_t)(2 + i) * B + b] = (int32_t)g.Lout;
                    t[(size_t)(2 + d.num_ups + i) * B + b] = g.M;
                    Lb = g.Lout;
                }
            }
            return SI_OK;
        })) return trc;
        SI_HIP_CHECK(hipMemsetAsync(wav_out, 0, (size_t)B * Lwav * sizeof(float), st));   // samples past a clip's own end read as silence
    }
    float* ext_ws = W.floats((size_t)Bc_max * Tout * Ly.mel_ld, "ext");
    const size_t nbuf = (size_t)Bc_max * lc_max;
    float* buf_ws[6] = {W.floats(nbuf, "buf0"), W.floats(nbuf, "buf1"), W.floats(nbuf, "buf2"), W.floats(nbuf, "buf3"), W.floats(nbuf, "buf4"), W.floats(nbuf, "buf5")};
    char* const h16_raw[6] = {W.bytes(nbuf * 2, "h16_0"), W.bytes(nbuf * 2, "h16_1"), W.bytes(nbuf * 2, "h16_2"),
                              W.bytes(nbuf * 2, "h16_3"), W.bytes(nbuf * 2, "h16_4"), W.bytes(nbuf * 2, "h16_5")};
    unsigned short* h16_ws[6];
    for (int i = 0; i < 6; ++i) h16_ws[i] = reinterpret_cast<unsigned short*>(h16_raw[i]);
    // Operand-ready activations (bf16 / fp16 vocoder): every producer also writes type16(leaky_relu(x, 0.1)) -- exactly
    // what the next convolution would compute while staging -- so consumers copy 2-byte operands instead of loading
    // fp32 and converting; the ResBlock intermediate exists only in that form.  Same arithmetic, bit-identical output;
    // 20-40 % less HBM / L2 traffic on the convolution inputs.  SI_VOC_OPREADY=0 restores the fp32-input path.
    const bool opr = ctx->popt.voc_opready && (d.vocoder_math == SI_MATH_BF16 || d.vocoder_math == SI_MATH_F16);
    // fp16 activation stream (fp16 mode): activations live ONLY as raw fp16 -- the residual stream too -- and the
    // consumer applies its leaky-ReLU to the packed halves while staging: 10 instead of 16 bytes of HBM traffic per
    // element and conv pair (these stages run on the memory side in fp16).  The rounding it adds (fp16 after every
    // residual add) is small next to the operand rounding the mode already has: waveform RMS error 1.35e-4 vs 1.10e-4
    // (gate 1e-3).  SI_VOC_RES16=0 keeps the fp32 residual stream.
    const bool r16 = opr && ctx->popt.voc_res16 && d.vocoder_math == SI_MATH_F16;
    const int fuse_mask = ctx->opt_voc_fuse == 1 ? ~0 : ctx->opt_voc_fuse;
    if (!W.ok) return si_fail(ctx, SI_ENOMEM, "internal: vocoder workspace carve exceeded its own estimate at region '%s'", W.failed);
    const int nk = d.num_rb;
    static const char* upn[] = {"ups0", "ups1", "ups2", "ups3", "ups4", "ups5", "ups6", "ups7"};
    static const char* stn[] = {"stage0", "stage1", "stage2", "stage3", "stage4", "stage5", "stage6", "stage7"};

    // the generator on clips [b0, b0 + Bc) with its own scratch, enqueued on stream `st`
    auto run = [&](int b0, int Bc, float* ext, float* const* buf, unsigned short* const* h16, hipStream_t st) -> int {
        int rc;
        // Taps of the fp16 activation stream (names ending in ".f16": the raw fp16 tensor as stored, n elements).  Copies only, behind
        // the launch that produced the tensor: a registered capture changes neither which kernel runs nor any value; without one, none is named.
        auto tap16 = [&](const void* src, long n, const char* fmt, int a = 0, int b = 0, int c = 0) -> int {
            return (r16 && !ctx->dbg_capture.empty()) ? si_tap(ctx, st, {src, n, 2}, fmt, a, b, c) : SI_OK;
        };
        // Their namesakes of the fp32 residual stream ("pre", "stage<i>.rb<j>.p<n>": n floats) and the pairs' intermediate
        // ("stage<i>.rb<j>.t<n>", or the raw 16-bit tensor where only that exists): copies under the same rule.
        auto tap32 = [&](TapSrc s, const char* fmt, int a = 0, int b = 0, int c = 0) -> int {
            return (!r16 && !ctx->dbg_capture.empty()) ? si_tap(ctx, st, s, fmt, a, b, c) : SI_OK;
        };
        // ragged batch: device / host rows of the chunk's clips -- dTm mel frames, dLs(s) rows at stage s (0 = stretched frames)
        const int32_t* dTm = vl ? tab.dev + b0 : nullptr;
        auto dLs = [&](int sidx) -> const int32_t* { return vl ? tab.dev + (size_t)(1 + sidx) * B + b0 : nullptr; };
        auto hLs = [&](int sidx) -> const int32_t* { return vl ? tab.host + (size_t)(1 + sidx) * B + b0 : nullptr; };
        auto rows_of = [&](const int32_t* h, long uniform) { if (!h) return (double)Bc * uniform; double r = 0; for (int b = 0; b < Bc; ++b) r += h[b]; return r; };
        // A same-length convolution on the L rows of stage sidx (0: the stretched frames), `cin` real input channels stored ld_in apart:
        // every clip reads and writes its own rows.  Operands, prologue slope and epilogue are the caller's.
        auto stage_conv = [&](const GemmW& G, int sidx, long L, int ld_in, int cin, int dil) {
            TapGemmParams p = gemm_params(ctx, G);
            p.nseg = Bc; p.Lin = (int)L; p.M = (int)L; p.ldx = ld_in; p.x_seg_stride = L * ld_in;
            p.dil = dil; p.pad = dil * (G.ntaps - 1) / 2; p.ldo = G.N; p.o_seg_stride = L * G.N; p.olimit = p.o_seg_stride;
            p.algo_macs = rows_of(hLs(sidx), L) * G.N * (double)cin * G.ntaps;
            if (vl) { p.seg_lin = p.seg_m = p.seg_orows = dLs(sidx); p.olim_mul = p.ldo; p.seg_m_host = hLs(sidx); }
            return p;
        };
        // Upsampler i on Lc input rows of c channels: leaky_relu -> ConvTranspose1d as `u` phases of a (k + u - 1) / u-tap conv (row u'
        // reads input rows u', u'-1, ...), reading x / x16 and writing U / U16 as the arithmetic mode stores them; pro_slope is the caller's.
        auto ups_desc = [&](int i, long Lc, int c, const float* x, const unsigned short* x16, float* U, unsigned short* U16) {
            const UpsGeom g = ups_geom(d, i, Lc);
            const int cout = stage_channels(ctx, i);
            TapGemmParams p = gemm_params(ctx, Ly.ups[i]);
            p.x = x; p.out = U;
            if (opr) { p.x = nullptr; p.x16 = x16; p.out16 = U16; p.out16_slope = r16 ? 1.f : 0.1f; }
            if (r16) p.out = nullptr;
            p.nseg = Bc; p.Lin = (int)Lc; p.M = g.M; p.ldx = c; p.x_seg_stride = Lc * c;
            p.dil = -1; p.ldo = g.u * cout; p.o_seg_stride = g.Lout * cout; p.ooff = -(long)g.pad * cout; p.olimit = g.Lout * cout;
            p.algo_macs = rows_of(hLs(i), Lc) * (double)(d.up_initial_channel >> i) * (double)(d.up_initial_channel >> (i + 1)) * d.up_kernels[i];   // Cin*Cout*k*Lin (real widths)
            const size_t mrow = (size_t)(2 + d.num_ups + i) * B + b0;   // the chunk's clips in the table's GEMM-row column of upsampler i
            if (vl) { p.seg_lin = dLs(i); p.seg_m = tab.dev + mrow; p.seg_orows = dLs(i + 1); p.olim_mul = cout; p.seg_m_host = tab.host + mrow; }
            return p;
        };
        // Does upsampler i take ACTIVATED input?  The early upsamplers (N = 2048 / 1024) on the fp16 stream are real GEMMs: the
        // one-tile-per-CU kernel (gemmcu.hip, TC mode) runs them wherever it covers the layer's geometry (always = true: whatever the
        // batch -- the two forms round differently, and a clip's samples must not depend on its batch); SI_VOC_UPSGEMM=0: the tap-GEMM.
        // The producer of its input (conv_pre / the launch that completes the previous stage's MRF sum) then stores leaky_relu(x, 0.1)
        // -- the upsampler's own first statement (models.py:110) applied once to the fp32 value instead of to every fragment it is read
        // into -- and the upsampler takes its input as it is.  Asked ONCE per upsampler, the answer goes to both sides.  (The streaming
        // kernel, which applies its own leaky-ReLU, never meets an activated input only because si_launch_upsample_stream takes
        // N = Cin in {64, 128} and gemmcu_tc_pick N % 256 == 0: facts of upsample.hip and gemmcu.hip.)
        auto ups_takes_activated = [&](int i, long Lc, int c) -> bool {
            if (!r16 || !ctx->opt_voc_upsgemm || i >= d.num_ups || Ly.ups[i].math != SI_MATH_F16 || !Ly.ups[i].has_bias) return false;
            return si_gemmcu_tc_covers(ctx, ups_desc(i, Lc, c, nullptr, h16[0], nullptr, h16[2]), true);
        };
        // A14: stretch + transpose to channels-last
        if ((rc = si_launch_extend_mel(ctx, mel + (size_t)b0 * d.num_mels * Tm, Bc, d.num_mels, Tm, (int)Tout, stretch, ext, Ly.mel_ld, st, dTm, dLs(0)))) return rc;
        // B1: conv_pre
        float *x = buf[0], *xs = buf[1];
        unsigned short *x16 = h16[0], *xs16 = h16[1], *U16 = h16[2], *t16 = h16[3];
        const float in_slope = (opr && !r16) ? 1.f : 0.1f;   // what a conv applies to a stage's tensor: operand-ready inputs are already activated
        bool act_in = ups_takes_activated(0, Tout, d.up_initial_channel);   // of the upsampler that reads x16
        TapGemmParams pre = stage_conv(Ly.pre, 0, Tout, Ly.mel_ld, d.num_mels, 1);
        pre.x = ext; pre.out = x;
        if (opr) { pre.out16 = x16; pre.out16_slope = (r16 && !act_in) ? 1.f : 0.1f; }
        if (r16) pre.out = nullptr;
        if ((rc = si_launch_tapgemm(ctx, Ly.pre.math, pre, st))) return rc;
        if ((rc = tap16(x16, (long)Bc * Tout * d.up_initial_channel, "pre.f16"))) return rc;
        if ((rc = tap32({x, (long)Bc * Tout * d.up_initial_channel}, "pre"))) return rc;
        long Lc = Tout; int c = d.up_initial_channel;
        for (int i = 0; i < d.num_ups; ++i) {
            const GemmW& G = Ly.ups[i];
            const int cout = stage_channels(ctx, i);
            const long Lo = Lc * d.up_rates[i];
            float* U = buf[2];
            // B2: the upsampler
            TapGemmParams p = ups_desc(i, Lc, c, x, x16, U, U16);
            bool ups_done = false;
            if (r16 && (fuse_mask & 2) && d.up_rates[i] == 2 && d.up_kernels[i] == 4 &&   // (SI_VOC_FUSE: bit 1 = this kernel, the width bits = the ResBlock kernels)
                G.has_bias && G.Npad == G.N && G.math == SI_MATH_F16) {
                // the late upsamplers (128 / 64 input channels) are HBM-bound: a persistent streaming kernel (upsample.hip)
                UpsampleParams q{};
                q.x16 = p.x16; q.w = static_cast<const unsigned short*>(p.w); q.bias = p.bias; q.out16 = p.out16;
                q.B = p.nseg; q.Lin = p.Lin; q.M = p.M; q.Cin = p.ldx; q.N = p.ldo; q.taps = p.ntaps;
                q.ooff = -p.ooff; q.o_clip_stride = p.o_seg_stride; q.o_clip_elems = p.olimit;
                q.lens_lin = p.seg_lin; q.lens_m = p.seg_m; q.lens_m_host = p.seg_m_host;
                rc = si_launch_upsample_stream(ctx, q, st);
                if (rc < 0) return rc;
                ups_done = rc == 0;
            }
            if (!ups_done) {
                p.pro_slope = act_in ? 1.f : in_slope;
                const int urc = act_in ? si_launch_gemmcu_tc(ctx, p, st, true) : 1;
                if (urc < 0) return urc;
                if (urc > 0 && (rc = si_launch_tapgemm(ctx, G.math, p, st))) return rc;
            }
            const long nst = (long)Bc * Lo * cout;                    // elements of every tensor of this stage
            if (!r16 && (rc = si_tap(ctx, st, {U, nst}, upn[i]))) return rc;
            if ((rc = tap16(U16, nst, "ups%d.f16", i))) return rc;
            // B3: multi-receptive-field fusion: mean over the resblocks, accumulated into xs by the last conv of each
            const bool act_next = ups_takes_activated(i + 1, Lo, cout);
            // What the launch that ends a step of ResBlock j stores; the block's `last` one adds its share of the MRF mean (alpha) to the
            // earlier blocks' (accumulate).  The 16-bit copy is wanted by the block's next conv, or -- once the mean is complete -- by the next
            // stage's upsampler (conv_post reads fp32), and carries that reader's leaky-ReLU unless the reader applies it itself (fp16 stream).
            struct BlockOut { float alpha; int accumulate; bool copy16; float slope16; };
            auto block_out = [&](int j, bool last) {
                const bool completes = last && j == nk - 1;
                return BlockOut{last ? 1.0f / nk : 1.f, last && j > 0, r16 || !last || (completes && i + 1 < d.num_ups),
                                (r16 && !(completes && act_next)) ? 1.f : 0.1f};
            };
            for (int j = 0; j < nk; ++j) {
                const ResW& R = Ly.rbs[(size_t)i * nk + j];
                const int rk = d.rb_kernels[j];
                const float* y = U;
                const unsigned short* y16 = U16;
                const BlockOut whole = block_out(j, true);
                if (r16 && d.resblock_type != 2 && (fuse_mask & cout) && ctx->opt_voc_chain && d.num_dil == 3 && whole.slope16 == 1.f) {
                    // full-rate stage: the whole resblock (three pairs) as one kernel, residual stream in LDS (reschain.hip: raw fp16 out)
                    ResChainParams cp{};
                    cp.y16 = U16; cp.out16 = xs16; cp.B = Bc; cp.L = (int)Lo; cp.k = rk; cp.alpha = whole.alpha; cp.accumulate = whole.accumulate;
                    cp.lens = dLs(i + 1); cp.lens_host = hLs(i + 1);
                    for (int n = 0; n < 3; ++n) {
                        const TapGemmParams w1 = gemm_params(ctx, R.c1[n]), w2 = gemm_params(ctx, R.c2[n]);
                        cp.w1[n] = static_cast<const unsigned short*>(w1.w); cp.w2[n] = static_cast<const unsigned short*>(w2.w);
                        cp.b1[n] = w1.bias; cp.b2[n] = w2.bias; cp.dil[n] = d.rb_dilations[j][n];
                    }
                    const int crc = si_launch_reschain(ctx, cout, cp, st);
                    if (crc < 0) return crc;
                    if (crc == 0) {
                        if ((rc = tap16(xs16, nst, "stage%d.rb%d.p%d.f16", i, j, d.num_dil - 1))) return rc;
                        continue;
                    }
                }
                for (int n = 0; n < d.num_dil; ++n) {
                    const int dl = d.rb_dilations[j][n];
                    const bool last = (n == d.num_dil - 1);
                    float* ynext = last ? xs : buf[4 + (n & 1)];
                    unsigned short* ynext16 = last ? xs16 : h16[4 + (n & 1)];
                    const BlockOut o = block_out(j, last);
                    // the convolution that ends this step: G on (in, in16) -> (ynext, ynext16) = y + conv, scaled, accumulated and copied as `o` says
                    auto residual_conv = [&](const GemmW& G, int dil, float slope, const float* in, const unsigned short* in16) {
                        TapGemmParams q = stage_conv(G, i + 1, Lo, cout, cout, dil);
                        q.x = in; q.out = ynext; q.res = y; q.pro_slope = slope;
                        if (opr) {
                            q.x = nullptr; q.x16 = in16;
                            if (r16) { q.res = nullptr; q.res16 = y16; q.out = nullptr; }
                            if (o.copy16) { q.out16 = ynext16; q.out16_slope = o.slope16; }
                        }
                        q.alpha = o.alpha; q.accumulate = o.accumulate; q.acc16 = r16 && o.accumulate;
                        return si_launch_tapgemm(ctx, G.math, q, st);
                    };
                    if (d.resblock_type == 2) {
                        // ResBlock2 (I_ea/hifi_gan/models.py:63-68): per dilation x = x + conv_d(lrelu(x)) -- ONE convolution with the
                        // residual (and, on the block's last one, the 1 / num_kernels scale and the MRF accumulate) in its epilogue
                        if ((rc = residual_conv(R.c1[n], dl, in_slope, y, y16))) return rc;
                    } else {
                        int frc = 1;
                        if (r16 && (fuse_mask & cout)) {
                            // narrow stages: conv pair as one kernel, the intermediate stays in LDS (respair.hip)
                            const TapGemmParams w1 = gemm_params(ctx, R.c1[n]), w2 = gemm_params(ctx, R.c2[n]);
                            frc = si_launch_respair(ctx, cout, y16, ynext16, w1.w, w2.w, w1.bias, w2.bias, Bc, (int)Lo, rk, dl, o.alpha, o.accumulate, st,
                                                    dLs(i + 1), hLs(i + 1), o.slope16);
                            if (frc < 0) return frc;
                        }
                        if (frc > 0) {
                            float* t = buf[3];
                            TapGemmParams p = stage_conv(R.c1[n], i + 1, Lo, cout, cout, dl);
                            p.x = y; p.out = t; p.pro_slope = in_slope;
                            if (opr) { p.x = nullptr; p.x16 = y16; p.out = nullptr; p.out16 = t16; p.out16_slope = 0.1f; }
                            if ((rc = si_launch_tapgemm(ctx, R.c1[n].math, p, st))) return rc;
                            if ((rc = !opr ? tap32({t, nst}, "stage%d.rb%d.t%d", i, j, n)
                                           : tap32({t16, nst, 2}, d.vocoder_math == SI_MATH_F16 ? "stage%d.rb%d.t%d.f16" : "stage%d.rb%d.t%d.bf16", i, j, n))) return rc;
                            if ((rc = residual_conv(R.c2[n], 1, opr ? 1.f : 0.1f, t, t16))) return rc;   // (the intermediate is stored activated in the 16-bit modes)
                        }
                    }
                    if ((rc = tap16(ynext16, nst, "stage%d.rb%d.p%d.f16", i, j, n))) return rc;
                    if ((rc = tap32({ynext, nst}, "stage%d.rb%d.p%d", i, j, n))) return rc;
                    y = ynext;
                    y16 = ynext16;
                }
            }
            if (!r16 && (rc = si_tap(ctx, st, {xs, nst}, stn[i]))) return rc;
            if ((rc = tap16(xs16, nst, "stage%d.f16", i))) return rc;
            std::swap(x, xs);
            std::swap(x16, xs16);
            Lc = Lo; c = cout; act_in = act_next;
        }
        // B4: leaky_relu(0.01) -> conv_post -> tanh
        return si_launch_conv_post(ctx, x, wf(ctx, Ly.post_w), wf(ctx, Ly.post_b), Bc, (int)Lc, c, 7, wav_out + (size_t)b0 * Lwav, st,
                                   r16 ? x16 : nullptr, dLs(d.num_ups), hLs(d.num_ups));
    };

    for (int b0 = 0; b0 < B; b0 += Bc_max) {
        const int Bc = std::min(Bc_max, B - b0);
        if (int rc = run(b0, Bc, ext_ws, buf_ws, h16_ws, st)) return rc;
    }
    return SI_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ mel front-end (f-1)
namespace {

// constants of I_ea/dataset/mel_dump.py:11-20
constexpr int FE_NFFT = 1024, FE_HOP = 441, FE_PAD = 312, FE_NMEL = 80, FE_SR = 22050, FE_NBIN = FE_NFFT / 2 + 1;
constexpr double FE_FMIN = 0.0, FE_FMAX = 8000.0;
// The real DFT as two half-size exact-fp32 GEMMs.  With s_k = x[k] + x[N - k] and d_k = x[k] - x[N - k] (k = 1 .. N/2 - 1; s_0 = x[0],
// s_{N/2} = x[N/2]):  Re X[n] = sum_{k=0}^{N/2} s_k cos(2 pi n k / N),  Im X[n] = -sum_{k=1}^{N/2-1} d_k sin(2 pi n k / N) -- the
// frames are written folded ([s_0 .. s_512 | 15 zeros | 0, d_1 .. d_511]) and each half meets a 513 x 528 / 513 x 512 matrix
// instead of the whole frame a 1026 x 1024 one: half the MACs, the same products (one fp32 add per operand pair before them).
constexpr int FE_KC = 528, FE_KS = 512;                // folded frame: cosine operands (513 padded to a multiple of 16) | sine operands
constexpr int FE_FRAME = FE_KC + FE_KS;                // 1040 floats per folded frame
constexpr int FE_IMOFF = 516;                          // spec row = [re(0..512) | 3 pad | im(0..512) | 3 pad]
constexpr int FE_LDSPEC = 1032;                        // spec row stride (16-byte aligned halves)

// Slaney mel scale (librosa.filters.mel defaults htk=False, norm='slaney', as called at mel_dump.py:66)
double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

size_t fe_round(size_t b) { return (b + 255) / 256 * 256; }

int ensure_frontend(si_ctx* ctx) {
    if (ctx->fe_dev) return SI_OK;
    const int npad = si_round_up(FE_NBIN, si_pick_bn(FE_NBIN));
    ctx->fe_dft = 0;                                                   // [npad][FE_KC] cosines, then [npad][FE_KS] (minus) sines
    ctx->fe_hann = ctx->fe_dft + fe_round((size_t)npad * FE_FRAME * 4);
    ctx->fe_basis = ctx->fe_hann + fe_round((size_t)FE_NFFT * 4);
    ctx->fe_lo = ctx->fe_basis + fe_round((size_t)FE_NBIN * FE_NMEL * 4);
    ctx->fe_hi = ctx->fe_lo + fe_round((size_t)FE_NMEL * 4);
    const size_t total = ctx->fe_hi + fe_round((size_t)FE_NMEL * 4);
    std::vector<char> host(total, 0);
    float* dft = reinterpret_cast<float*>(host.data() + ctx->fe_dft);
    float* hann = reinterpret_cast<float*>(host.data() + ctx->fe_hann);
    float* basis_t = reinterpret_cast<float*>(host.data() + ctx->fe_basis);
    int32_t* lo = reinterpret_cast<int32_t*>(host.data() + ctx->fe_lo);
    int32_t* hi = reinterpret_cast<int32_t*>(host.data() + ctx->fe_hi);
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < FE_NFFT; ++k) hann[k] = (float)(0.5 - 0.5 * std::cos(two_pi * k / FE_NFFT));   // torch.hann_window (periodic)
    float* dsin = dft + (size_t)npad * FE_KC;
    for (int n = 0; n < FE_NBIN; ++n)
        for (int k = 0; k <= FE_NFFT / 2; ++k) {
            const double a = two_pi * ((long)n * k % FE_NFFT) / FE_NFFT;   // exact argument reduction
            dft[(size_t)n * FE_KC + k] = (float)std::cos(a);               // columns 0 .. 512 (513 .. 527 stay zero)
            if (k >= 1 && k < FE_NFFT / 2) dsin[(size_t)n * FE_KS + k] = (float)-std::sin(a);   // columns 1 .. 511 (d_0 = 0)
        }
    // triangular filters on the Slaney scale, area-normalised
    std::vector<double> mel_f(FE_NMEL + 2);
    const double m0 = hz_to_mel(FE_FMIN), m1 = hz_to_mel(FE_FMAX);
    for (int i = 0; i < FE_NMEL + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (FE_NMEL + 1));
    for (int i = 0; i < FE_NMEL; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        int first = FE_NBIN, last = -1;
        for (int f = 0; f < FE_NBIN; ++f) {
            const double hz = (double)FE_SR / 2.0 * f / (FE_NBIN - 1);
            const double lower = (hz - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - hz) / (mel_f[i + 2] - mel_f[i + 1]);
            const double w = std::max(0.0, std::min(lower, upper)) * enorm;
            const float wf32 = (float)w;
            basis_t[(size_t)f * FE_NMEL + i] = wf32;
            if (wf32 != 0.f) { first = std::min(first, f); last = f; }
        }
        lo[i] = last < 0 ? 0 : first;
        hi[i] = last < 0 ? 0 : last + 1;
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    char* dev = nullptr;
    SI_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dev), total));
    hipError_t e = hipMemcpy(dev, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dev); return si_fail_hip(ctx, e, "front-end table upload", __FILE__, __LINE__); }
    ctx->fe_dev = dev;
    return SI_OK;
}

size_t mel_ws_bytes(const si_ctx* ctx, int B, int N22) {
    const long Tm = (N22 + 2 * FE_PAD - FE_NFFT) / FE_HOP + 1;
    if (Tm < 1) return 0;
    return fe_round((size_t)B * 4) + fe_round((size_t)B * Tm * FE_FRAME * 4) + fe_round((size_t)B * Tm * FE_LDSPEC * 4) + 256 +
           fe_round((size_t)2 * B * 4) +                             // ragged batches: the length table
           MEL_WS_ZONES * ctx->ws_zone;
}

}  // namespace

extern "C" {

int si_mel_frames(int n22) { return n22 + 2 * FE_PAD < FE_NFFT ? 0 : (n22 + 2 * FE_PAD - FE_NFFT) / FE_HOP + 1; }

int si_mel_workspace_bytes(si_ctx* ctx, int B, int N22, size_t* out) {
    if (!ctx || !out || B <= 0 || si_mel_frames(N22) < 1) return si_fail(ctx, SI_EINVAL, "si_mel_workspace_bytes: bad argument");
    *out = mel_ws_bytes(ctx, B, N22);
    return SI_OK;
}

static int mel_run(si_ctx* ctx, const float* wave22, const int32_t* mask_start, const int32_t* mask_end, int normalize, int B,
                   int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream, const int32_t* host_len,
                   const SiSpans* spans = nullptr);

int si_mel_frontend_spans(si_ctx* ctx, const float* wave22, const si_span_table* spans, const int32_t* sample_len, int normalize,
                          int B, int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (B <= 0) return si_fail(ctx, SI_EINVAL, "si_mel_frontend_spans: NULL / empty argument");
    SiSpans sp;
    if (int rc = check_span_table(ctx, "si_mel_frontend_spans", spans, B, sp)) return rc;
    return mel_run(ctx, wave22, nullptr, nullptr, normalize, B, N22, mel_out, workspace, workspace_bytes, stream, sample_len, &sp);
}

int si_mel_frontend(si_ctx* ctx, const float* wave22, const int32_t* mask_start, const int32_t* mask_end, int normalize, int B,
                    int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream) {
    return mel_run(ctx, wave22, mask_start, mask_end, normalize, B, N22, mel_out, workspace, workspace_bytes, stream, nullptr);
}

int si_mel_frontend_varlen(si_ctx* ctx, const float* wave22, const int32_t* mask_start, const int32_t* mask_end, const int32_t* sample_len,
                           int normalize, int B, int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!sample_len) return si_fail(ctx, SI_EINVAL, "si_mel_frontend_varlen: NULL lengths");
    return mel_run(ctx, wave22, mask_start, mask_end, normalize, B, N22, mel_out, workspace, workspace_bytes, stream, sample_len);
}

// host_len (B, HOST) or null: ragged batch -- clip b holds host_len[b] samples of its row of N22 (peak, reflection and frame count are its own)
static int mel_run(si_ctx* ctx, const float* wave22, const int32_t* mask_start, const int32_t* mask_end, int normalize, int B,
                   int N22, float* mel_out, void* workspace, size_t workspace_bytes, si_stream_t stream, const int32_t* host_len,
                   const SiSpans* spans) {
    if (!ctx) return SI_EINVAL;
    if (!wave22 || !mel_out || !workspace || B <= 0) return si_fail(ctx, SI_EINVAL, "si_mel_frontend: NULL / empty argument");
    if ((mask_start == nullptr) != (mask_end == nullptr))
        return si_fail(ctx, SI_EINVAL, "si_mel_frontend: mask_start and mask_end must both be given or both be NULL");
    const int Tm = si_mel_frames(N22);
    if (Tm < 1 || N22 <= FE_PAD) return si_fail(ctx, SI_EINVAL, "clip of %d samples is too short for the %d-sample reflect pad / %d-point STFT", N22, FE_PAD, FE_NFFT);
    if (workspace_bytes < mel_ws_bytes(ctx, B, N22))
        return si_fail(ctx, SI_ENOMEM, "workspace of %zu bytes < %zu needed for B=%d N22=%d", workspace_bytes, mel_ws_bytes(ctx, B, N22), B, N22);
    int rc = ensure_frontend(ctx);
    if (rc) return rc;
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Carver W = carver(ctx, SI_WS_MEL, workspace, workspace_bytes);
    float* peak = W.floats((size_t)B, "peak");
    float* frames = W.floats((size_t)B * Tm * FE_FRAME, "frames");
    float* spec = W.floats((size_t)B * Tm * FE_LDSPEC, "spec");
    const int32_t *d_n = nullptr, *d_tm = nullptr;
    if (host_len) {                                                    // table [samples | frames] per clip
        VlTable tab;
        if ((rc = vl_table(ctx, W, (size_t)2 * B, st, "mel", tab, [&](int32_t* t) -> int {
            for (int b = 0; b < B; ++b) {
                if (host_len[b] <= FE_PAD || host_len[b] > N22 || si_mel_frames(host_len[b]) < 1)
                    return si_fail(ctx, SI_EINVAL, "ragged batch: clip %d holds %d samples: too short for the mel front-end or longer than its row (%d)", b, host_len[b], N22);
                t[b] = host_len[b];
                t[(size_t)B + b] = si_mel_frames(host_len[b]);
            }
            return SI_OK;
        }))) return rc;
        d_n = tab.dev; d_tm = tab.dev + B;
    }
    if (!W.ok) return si_fail(ctx, SI_ENOMEM, "internal: mel workspace carve exceeded its own estimate at region '%s'", W.failed);
    const float* hann = reinterpret_cast<const float*>(ctx->fe_dev + ctx->fe_hann);
    if (normalize && (rc = si_launch_wave_peak(ctx, wave22, mask_start, mask_end, B, N22, peak, st, d_n, spans))) return rc;
    if (normalize && !ctx->dbg_capture.empty() && (rc = si_tap(ctx, st, {peak, (long)B}, "mel_peak"))) return rc;   // (per-op tap)
    if ((rc = si_launch_mel_frames(ctx, wave22, mask_start, mask_end, peak, hann, B, N22, Tm, FE_HOP, FE_PAD, FE_NFFT, FE_KC, normalize, frames, st, d_n, d_tm, spans)))
        return rc;
    if ((rc = si_tap(ctx, st, {frames, (long)B * Tm * FE_FRAME}, "mel_frames"))) return rc;
    // STFT as two exact-fp32 GEMMs on the folded frames: (B*Tm, 528) x (528, 513) -> re, (B*Tm, 512) x (512, 513) -> im
    const int npad = si_round_up(FE_NBIN, si_pick_bn(FE_NBIN));
    for (int half = 0; half < 2; ++half) {
        TapGemmParams p{};
        p.w = ctx->fe_dev + ctx->fe_dft + (half ? (size_t)npad * FE_KC * 4 : 0); p.w_lo = nullptr; p.bias = nullptr; p.res = nullptr;
        p.x = frames + (half ? FE_KC : 0); p.out = spec + (half ? FE_IMOFF : 0);
        p.nseg = 1; p.Lin = B * Tm; p.M = B * Tm; p.ldx = FE_FRAME; p.x_seg_stride = 0;
        p.Cin = half ? FE_KS : FE_KC; p.N = FE_NBIN; p.Npad = npad; p.ntaps = 1; p.stride = 1; p.dil = 1; p.pad = 0; p.groups = 1;
        p.ldo = FE_LDSPEC; p.o_seg_stride = 0; p.ooff = 0; p.olimit = (long)B * Tm * FE_LDSPEC - (half ? FE_IMOFF : 0);
        p.pro_slope = 1.f; p.act = SI_ACT_NONE; p.alpha = 1.f; p.accumulate = 0;
        if ((rc = si_launch_tapgemm(ctx, SI_MATH_F32, p, st))) return rc;
    }
    if (!ctx->dbg_capture.empty() && (rc = si_tap(ctx, st, {spec, (long)B * Tm * FE_LDSPEC}, "mel_spec"))) return rc;   // (per-op tap)
    return si_launch_mel_project(ctx, spec, FE_LDSPEC, FE_NBIN, FE_IMOFF, reinterpret_cast<const float*>(ctx->fe_dev + ctx->fe_basis),
                                 reinterpret_cast<const int32_t*>(ctx->fe_dev + ctx->fe_lo),
                                 reinterpret_cast<const int32_t*>(ctx->fe_dev + ctx->fe_hi), FE_NMEL, B, Tm, mel_out, st, d_tm);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ patch mode
extern "C" {

int si_wave_peak(si_ctx* ctx, const float* wave22, const si_span_table* spans, const int32_t* sample_len, int B, int N22, float* peak_out,
                 si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!wave22 || !peak_out || B <= 0 || N22 <= 0) return si_fail(ctx, SI_EINVAL, "si_wave_peak: NULL / empty argument");
    SiSpans sp{};
    if (spans) if (int rc = check_span_table(ctx, "si_wave_peak", spans, B, sp)) return rc;
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_wave_peak(ctx, wave22, nullptr, nullptr, B, N22, peak_out, static_cast<hipStream_t>(stream), sample_len, spans ? &sp : nullptr);
}

int si_gather_windows(si_ctx* ctx, const float* ext, int B, int Tout, const int32_t* host_win, const int32_t* win, int W, int Wmax,
                      float* out, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!ext || !host_win || !win || !out || B <= 0 || Tout <= 0 || W <= 0 || Wmax <= 0)
        return si_fail(ctx, SI_EINVAL, "si_gather_windows: NULL / empty argument");
    for (int w = 0; w < W; ++w) {
        const int clip = host_win[w], w0 = host_win[W + w], w1 = host_win[2 * W + w];
        if (clip < 0 || clip >= B) return si_fail(ctx, SI_EINVAL, "si_gather_windows: window %d names clip %d of a batch of %d", w, clip, B);
        if (w0 < 0 || w1 <= w0 || w1 > Tout)
            return si_fail(ctx, SI_EINVAL, "si_gather_windows: window %d = frames [%d, %d) is outside its clip's %d stretched frames", w, w0, w1, Tout);
        if (w1 - w0 > Wmax) return si_fail(ctx, SI_EINVAL, "si_gather_windows: window %d holds %d frames, rows hold %d", w, w1 - w0, Wmax);
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_gather_windows(ctx, ext, win, W, ctx->d.num_mels, Tout, Wmax, out, static_cast<hipStream_t>(stream));
}

int si_patch_compose(si_ctx* ctx, const float* orig, const si_span_table* spans, const int32_t* sample_len, const si_patch_table* patch,
                     const float* gen, int Lrow, const float* gain, int B, int N22, float* out_f32, int16_t* out_pcm, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!orig || B <= 0 || N22 <= 0) return si_fail(ctx, SI_EINVAL, "si_patch_compose: NULL / empty argument");
    if (!out_f32 && !out_pcm) return si_fail(ctx, SI_EINVAL, "si_patch_compose: both outputs are NULL");
    SiSpans sp{};
    if (int rc = check_span_table(ctx, "si_patch_compose", spans, B, sp)) return rc;
    const si_patch_table* t = patch;
    if (!t || t->struct_size != (int32_t)sizeof(si_patch_table)) return si_fail(ctx, SI_EINVAL, "si_patch_compose: si_patch_table size mismatch");
    if (t->fade < 0 || (long)t->fade + N22 > 0x7fffffffL) return si_fail(ctx, SI_EINVAL, "si_patch_compose: fade of %d samples is negative or too long", t->fade);
    if (t->num_clips != B || t->num_spans != spans->num_spans || t->num_windows < 0)
        return si_fail(ctx, SI_EINVAL, "si_patch_compose: patch table for %d clips / %d spans / %d windows, call with %d clips / %d spans", t->num_clips,
                       t->num_spans, t->num_windows, B, spans->num_spans);
    const int W = t->num_windows;
    if (!t->host_lim || !t->lim || (t->fade > 0 && !t->ramp)) return si_fail(ctx, SI_EINVAL, "si_patch_compose: patch table with NULL lim / ramp");
    if (W > 0 && (!t->host_win_clip || !t->host_win_start || !t->host_win_len || !t->win_start || !t->win_len || !gen || Lrow <= 0))
        return si_fail(ctx, SI_EINVAL, "si_patch_compose: %d windows but NULL window arrays / generator rows", W);
    if (t->num_spans > 0 && (!t->host_span_win || !t->span_win)) return si_fail(ctx, SI_EINVAL, "si_patch_compose: patch table with NULL span_win");
    for (int w = 0; w < W; ++w) {
        const long c = t->host_win_clip[w], s = t->host_win_start[w], l = t->host_win_len[w];
        if (c < 0 || c >= B || s < 0 || l < 0 || l > Lrow || s + l > N22)
            return si_fail(ctx, SI_EINVAL, "si_patch_compose: window %d = clip %ld samples [%ld, +%ld) is outside its clip (%d clips of %d samples, rows of %d)",
                           w, c, s, l, B, N22, Lrow);
    }
    for (int b = 0; b < B; ++b) {
        const int n = sample_len ? sample_len[b] : N22, lim = t->host_lim[b];
        if (n < 0 || n > N22 || lim < 0 || lim > n)
            return si_fail(ctx, SI_EINVAL, "si_patch_compose: clip %d holds %d samples of its row of %d, lim %d", b, n, N22, lim);
        for (int k = spans->host_off[b]; k < spans->host_off[b + 1]; ++k) {
            const int s = spans->host_start[k], l = spans->host_len[k];
            if (l <= 0 || s >= lim) continue;
            const int w = t->host_span_win[k];
            if (w < 0 || w >= W) return si_fail(ctx, SI_EINVAL, "si_patch_compose: clip %d span %d names window %d of %d", b, k - spans->host_off[b], w, W);
            if (t->host_win_clip[w] != b)
                return si_fail(ctx, SI_EINVAL, "si_patch_compose: clip %d span %d names window %d, which belongs to clip %d", b, k - spans->host_off[b], w, t->host_win_clip[w]);
            const int e = std::min(s + l, lim);
            const int ra = std::max(s - t->fade, 0), rb = std::min(e + t->fade, lim);
            if (ra < t->host_win_start[w] || rb > t->host_win_start[w] + t->host_win_len[w])
                return si_fail(ctx, SI_EINVAL, "si_patch_compose: clip %d span %d blends samples [%d, %d), its window's row holds [%d, %d)", b,
                               k - spans->host_off[b], ra, rb, t->host_win_start[w], t->host_win_start[w] + t->host_win_len[w]);
        }
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    const SiPatch pt{t->win_start, t->win_len, t->span_win, t->lim, t->ramp, t->fade};
    return si_launch_patch_compose(ctx, orig, sp, pt, gen, Lrow, gain, B, N22, out_f32, out_pcm, static_cast<hipStream_t>(stream));
}

// ---- long recordings
static const long SI_MAX_REC = 0x7fffffffL - 2048;      // int32 sample indices, one chunk of headroom for the chunk's end

// ceiling != nullptr is si_cut_clips_valid: an invalid sample copied as +0.0 -- the same refusals under that entry's name, plus
// the ceiling's.
static int cut_clips_call(si_ctx* ctx, const char* fn, const float* src, int n_src, const int32_t* host_start, const int32_t* start, int C, int L,
                          float* out, si_stream_t stream, const float* ceiling) {
    if (!ctx) return SI_EINVAL;
    if (!src || !host_start || !start || !out || n_src <= 0 || C <= 0 || L <= 0) return si_fail(ctx, SI_EINVAL, "%s: NULL / empty argument", fn);
    if ((long)n_src > SI_MAX_REC) return si_fail(ctx, SI_EINVAL, "%s: a source of %d samples, at most %ld", fn, n_src, SI_MAX_REC);
    if (C > 65535) return si_fail(ctx, SI_EINVAL, "%s: %d clips in one call, at most 65535 (the launch grid's second dimension)", fn, C);
    if (ceiling && !(*ceiling > 0.f)) return si_fail(ctx, SI_EINVAL, "%s: ceiling = %g is not above 0, or is NaN", fn, (double)*ceiling);
    for (int c = 0; c < C; ++c) {
        const long s = host_start[c];
        if (s < 0 || s + L > n_src)
            return si_fail(ctx, SI_EINVAL, "%s: clip %d = samples [%ld, %ld) is outside the source's %d samples", fn, c, s, s + L, n_src);
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_cut_clips(ctx, src, start, C, L, ceiling, out, static_cast<hipStream_t>(stream));
}

int si_cut_clips(si_ctx* ctx, const float* src, int n_src, const int32_t* host_start, const int32_t* start, int C, int L, float* out,
                 si_stream_t stream) {
    return cut_clips_call(ctx, "si_cut_clips", src, n_src, host_start, start, C, L, out, stream, nullptr);
}

int si_cut_clips_valid(si_ctx* ctx, const float* src, int n_src, const int32_t* host_start, const int32_t* start, int C, int L, float ceiling,
                       float* out, si_stream_t stream) {
    return cut_clips_call(ctx, "si_cut_clips_valid", src, n_src, host_start, start, C, L, out, stream, &ceiling);
}

int si_patch_regions(si_ctx* ctx, const float* orig, int N22, const si_region_table* table, const float* gen, int Lrow, const float* gain,
                     float* out_f32, int16_t* out_pcm, si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (!orig || N22 <= 0) return si_fail(ctx, SI_EINVAL, "si_patch_regions: NULL / empty argument");
    if ((long)N22 > SI_MAX_REC) return si_fail(ctx, SI_EINVAL, "si_patch_regions: a recording of %d samples, at most %ld", N22, SI_MAX_REC);
    if (!out_f32 && !out_pcm) return si_fail(ctx, SI_EINVAL, "si_patch_regions: both outputs are NULL");
    const si_region_table* t = table;
    if (!t || t->struct_size != (int32_t)sizeof(si_region_table)) return si_fail(ctx, SI_EINVAL, "si_patch_regions: si_region_table size mismatch");
    if (t->fade < 0 || (long)t->fade + N22 > 0x7fffffffL) return si_fail(ctx, SI_EINVAL, "si_patch_regions: fade of %d samples is negative or too long", t->fade);
    const int C = t->num_contexts, W = t->num_windows, K = t->num_spans, Q = t->num_chunks, fade = t->fade;
    if (C < 0 || W < 0 || K < 0 || Q < 0)
        return si_fail(ctx, SI_EINVAL, "si_patch_regions: region table with %d contexts / %d windows / %d spans / %d chunks", C, W, K, Q);
    if (fade > 0 && K > 0 && !t->ramp) return si_fail(ctx, SI_EINVAL, "si_patch_regions: region table with NULL ramp");
    if (W > 0 && (!t->host_win_ctx || !t->host_win_start || !t->host_win_len || !t->win_ctx || !t->win_start || !t->win_len || !gen || Lrow <= 0))
        return si_fail(ctx, SI_EINVAL, "si_patch_regions: %d windows but NULL window arrays / generator rows", W);
    if (K > 0 && (!t->host_start || !t->host_len || !t->host_span_win || !t->host_span_lim || !t->start || !t->len || !t->span_win || !t->span_lim))
        return si_fail(ctx, SI_EINVAL, "si_patch_regions: %d spans but NULL span arrays", K);
    if (Q > 0 && (!t->host_chunk || !t->host_k0 || !t->host_k1 || !t->chunk || !t->k0 || !t->k1))
        return si_fail(ctx, SI_EINVAL, "si_patch_regions: %d chunks but NULL chunk arrays", Q);
    for (int w = 0; w < W; ++w) {
        const long c = t->host_win_ctx[w], s = t->host_win_start[w], l = t->host_win_len[w];
        if (c < 0 || c >= C) return si_fail(ctx, SI_EINVAL, "si_patch_regions: window %d names context %ld of %d", w, c, C);
        if (s < 0 || l < 0 || l > Lrow || s + l > N22)
            return si_fail(ctx, SI_EINVAL, "si_patch_regions: window %d = samples [%ld, +%ld) is outside the recording (%d samples, rows of %d)", w, s, l,
                           N22, Lrow);
    }
    for (int q = 0; q < Q; ++q) {
        const long c = t->host_chunk[q];
        if (c < 0 || c * 2048 >= N22) return si_fail(ctx, SI_EINVAL, "si_patch_regions: chunk entry %d names chunk %ld, at or past the recording's %d samples", q, c, N22);
        if (q && c <= t->host_chunk[q - 1])
            return si_fail(ctx, SI_EINVAL, "si_patch_regions: chunk entry %d names chunk %ld after chunk %d: not strictly increasing", q, c, t->host_chunk[q - 1]);
        if (t->host_k0[q] < 0 || t->host_k0[q] > t->host_k1[q] || t->host_k1[q] > K)
            return si_fail(ctx, SI_EINVAL, "si_patch_regions: chunk entry %d walks spans [%d, %d) of %d", q, t->host_k0[q], t->host_k1[q], K);
    }
    for (int k = 0; k < K; ++k) {
        const long s = t->host_start[k], l = t->host_len[k], lim = t->host_span_lim[k];
        if (s < 0 || l <= 0 || lim <= s || lim > N22)
            return si_fail(ctx, SI_EINVAL, "si_patch_regions: span %d = samples [%ld, +%ld) with lim %ld does not lie in the recording's %d samples", k, s, l, lim, N22);
        if (k && s < (long)t->host_start[k - 1] + t->host_len[k - 1])
            return si_fail(ctx, SI_EINVAL, "si_patch_regions: span %d starts at %ld, before span %d ends: unsorted or overlapping", k, s, k - 1);
    }
    int q = 0;                                                     // the spans are sorted: the chunk list is walked (nearly) once
    for (int k = 0; k < K; ++k) {
        const long s = t->host_start[k], l = t->host_len[k], lim = t->host_span_lim[k];
        const int w = t->host_span_win[k];
        if (w < 0 || w >= W) return si_fail(ctx, SI_EINVAL, "si_patch_regions: span %d names window %d of %d", k, w, W);
        const long ra = std::max(s - fade, 0L), rb = std::min(s + l + fade, lim);
        if (ra < t->host_win_start[w] || rb > (long)t->host_win_start[w] + t->host_win_len[w])
            return si_fail(ctx, SI_EINVAL, "si_patch_regions: span %d blends samples [%ld, %ld), its window's row holds [%d, %d)", k, ra, rb,
                           t->host_win_start[w], t->host_win_start[w] + t->host_win_len[w]);
        const long qa = ra / 2048, qb = (rb - 1) / 2048;
        while (q > 0 && t->host_chunk[q - 1] >= qa) --q;            // a region may start in the chunk its predecessor ended in
        for (long c = qa; c <= qb; ++c) {
            while (q < Q && t->host_chunk[q] < c) ++q;
            if (q >= Q || t->host_chunk[q] != c)
                return si_fail(ctx, SI_EINVAL, "si_patch_regions: span %d blends samples [%ld, %ld), the chunk list lacks chunk %ld", k, ra, rb, c);
            if (k < t->host_k0[q] || k >= t->host_k1[q])
                return si_fail(ctx, SI_EINVAL, "si_patch_regions: chunk entry %d (chunk %ld) walks spans [%d, %d) and omits span %d, which blends samples [%ld, %ld)",
                               q, c, t->host_k0[q], t->host_k1[q], k, ra, rb);
        }
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    const SiRegions rt{t->start, t->len, t->span_win, t->span_lim, t->win_ctx, t->win_start, t->chunk, t->k0, t->k1, t->ramp, fade};
    return si_launch_patch_regions(ctx, orig, rt, Q, gen, Lrow, gain, N22, out_f32, out_pcm, static_cast<hipStream_t>(stream));
}

// ---- repair at the file's own sample rate
// The mono entry points and their interleaved siblings share one validation each: `fn` names the entry in the message;
// inter = false is the mono call (its own kernel; channels and channel are not read), inter = true the interleaved one, with n / n_file
// counting sample times.
#define SI_FAIL_FN(fmt, ...) si_fail(ctx, SI_EINVAL, "%s: " fmt, fn, ##__VA_ARGS__)

static int si_check_channels(si_ctx* ctx, const char* fn, int channels, int channel, int lowest) {
    if (channels < 1 || channels > SI_MAX_CHANNELS) return SI_FAIL_FN("channels = %d, outside 1 .. SI_MAX_CHANNELS = %d", channels, SI_MAX_CHANNELS);
    if (channel < lowest || channel >= channels) return SI_FAIL_FN("channel = %d, outside %d .. %d", channel, lowest, channels - 1);
    return SI_OK;
}

// (P, Q) = (target, sr) / gcd: sample j of the target rate's axis sits at position j Q / P of the axis at sr
static void si_rate_ratio(long target, long sr, long* P, long* Q) {
    long ga = target, gb = sr;
    while (gb) { const long r = ga % gb; ga = gb; gb = r; }
    *P = target / ga, *Q = sr / ga;
}

static int patch_rate_call(si_ctx* ctx, const char* fn, bool inter, const void* orig, int is_pcm16, int n_file, int channels, int channel, int sr,
                           const si_rate_table* table, const float* gen, int Lrow, const float* gain, const si_sinc_filter* filt, void* out,
                           si_stream_t stream) {
    if (!ctx) return SI_EINVAL;
    if (inter && si_check_channels(ctx, fn, channels, channel, 0) != SI_OK) return SI_EINVAL;
    if (!orig || !out || n_file <= 0) return SI_FAIL_FN("NULL / empty argument");
    if (orig == out) return SI_FAIL_FN("out is orig (orig is read while out is written)");
    if (sr < 4000 || sr > 192000) return SI_FAIL_FN("sr = %d Hz, outside 4000 .. 192000", sr);
    if (sr == 22050) return SI_FAIL_FN("sr = 22050 Hz is the generator's own rate: that file is si_patch_regions'");
    if ((long)n_file > SI_MAX_REC) return SI_FAIL_FN("a file of %d samples, at most %ld", n_file, SI_MAX_REC);
    long P, Qr;
    si_rate_ratio(22050, sr, &P, &Qr);
    const long N22 = ((long)n_file * P + Qr - 1) / Qr;              // the recording's samples on the 22.05 kHz axis, ceil(n_file P / Q)
    if (N22 > SI_MAX_REC) return SI_FAIL_FN("%d samples at %d Hz are %ld samples at 22050 Hz, at most %ld", n_file, sr, N22, SI_MAX_REC);
    const si_sinc_filter* f = filt;
    if (!f || f->struct_size != (int32_t)sizeof(si_sinc_filter)) return SI_FAIL_FN("si_sinc_filter size mismatch");
    if (!f->win || !f->dwin || f->nwin < 2 || f->num_table < 1 || f->step < 1 || !(f->scale > 0.0 && f->scale <= 1.0))
        return SI_FAIL_FN("bad filter table (nwin %d, num_table %d, step %d, scale %g)", f->nwin, f->num_table, f->step, f->scale);
    const long H = ((long)f->nwin + f->step - 1) / f->step;
    const long row_cap = 2047 * P / Qr + 2 + 2 * H;
    if (row_cap * (long)sizeof(float) > 65536)
        return SI_FAIL_FN("bad filter table: %ld taps per wing at %d Hz need %ld staged samples per chunk, at most 16384", H, sr, row_cap);
    const si_rate_table* t = table;
    if (!t || t->struct_size != (int32_t)sizeof(si_rate_table)) return SI_FAIL_FN("si_rate_table size mismatch");
    if (t->fade < 0 || (long)t->fade + n_file > 0x7fffffffL) return SI_FAIL_FN("fade of %d samples is negative or too long", t->fade);
    const int C = t->num_contexts, W = t->num_windows, K = t->num_spans, Q = t->num_chunks, fade = t->fade;
    if (C < 0 || W < 0 || K < 0 || Q < 0)
        return SI_FAIL_FN("rate table with %d contexts / %d windows / %d spans / %d chunks", C, W, K, Q);
    if (fade > 0 && K > 0 && !t->ramp) return SI_FAIL_FN("rate table with NULL ramp");
    if (W > 0 && (!t->host_win_ctx || !t->host_win_start || !t->host_win_len || !t->host_win_lim || !t->win_ctx || !t->win_start || !t->win_len ||
                  !t->win_lim || !gen || Lrow <= 0))
        return SI_FAIL_FN("%d windows but NULL window arrays / generator rows", W);
    if (K > 0 && (!t->host_start || !t->host_len || !t->host_span_win || !t->host_span_lim || !t->start || !t->len || !t->span_win || !t->span_lim))
        return SI_FAIL_FN("%d spans but NULL span arrays", K);
    if (Q > 0 && (!t->host_chunk || !t->host_k0 || !t->host_k1 || !t->chunk || !t->k0 || !t->k1))
        return SI_FAIL_FN("%d chunks but NULL chunk arrays", Q);
    for (int w = 0; w < W; ++w) {
        const long c = t->host_win_ctx[w], s = t->host_win_start[w], l = t->host_win_len[w], lim = t->host_win_lim[w];
        if (c < 0 || c >= C) return SI_FAIL_FN("window %d names context %ld of %d", w, c, C);
        if (s < 0 || l < 0 || l > Lrow || s + l > N22)
            return SI_FAIL_FN("window %d = 22.05 kHz samples [%ld, +%ld) is outside the recording (%ld samples, rows of %d)", w, s, l,
                           N22, Lrow);
        if (lim <= s || lim > N22)
            return SI_FAIL_FN("window %d starts at 22.05 kHz sample %ld, its context's audio ends at %ld of %ld", w, s, lim, N22);
    }
    for (int q = 0; q < Q; ++q) {
        const long c = t->host_chunk[q];
        if (c < 0 || c * 2048 >= n_file) return SI_FAIL_FN("chunk entry %d names chunk %ld, at or past the file's %d samples", q, c, n_file);
        if (q && c <= t->host_chunk[q - 1])
            return SI_FAIL_FN("chunk entry %d names chunk %ld after chunk %d: not strictly increasing", q, c, t->host_chunk[q - 1]);
        if (t->host_k0[q] < 0 || t->host_k0[q] > t->host_k1[q] || t->host_k1[q] > K)
            return SI_FAIL_FN("chunk entry %d walks spans [%d, %d) of %d", q, t->host_k0[q], t->host_k1[q], K);
    }
    for (int k = 0; k < K; ++k) {
        const long s = t->host_start[k], l = t->host_len[k], lim = t->host_span_lim[k];
        if (s < 0 || l <= 0 || lim <= s || lim > n_file)
            return SI_FAIL_FN("span %d = samples [%ld, +%ld) with lim %ld does not lie in the file's %d samples", k, s, l, lim, n_file);
        if (k && s < (long)t->host_start[k - 1] + t->host_len[k - 1])
            return SI_FAIL_FN("span %d starts at %ld, before span %d ends: unsorted or overlapping", k, s, k - 1);
    }
    int q = 0;                                                     // the spans are sorted: the chunk list is walked (nearly) once
    for (int k = 0; k < K; ++k) {
        const long s = t->host_start[k], l = t->host_len[k], lim = t->host_span_lim[k];
        const int w = t->host_span_win[k];
        if (w < 0 || w >= W) return SI_FAIL_FN("span %d names window %d of %d", k, w, W);
        const long ws = t->host_win_start[w], we = ws + t->host_win_len[w], wlim = t->host_win_lim[w];
        if ((lim - 1) * P >= wlim * Qr)
            return SI_FAIL_FN("span %d writes up to file sample %ld = 22.05 kHz sample %ld, its context's audio ends at %ld", k, lim,
                           (lim - 1) * P / Qr, wlim);
        const long ra = std::max(s - fade, 0L), rb = std::min(s + l + fade, lim);
        const long xa = std::max(ra * P / Qr - H, 0L), xb = std::min((rb - 1) * P / Qr + 1 + H, wlim);      // what the taps read inside [0, win_lim)
        if (xa < ws || xb > we)
            return SI_FAIL_FN("span %d blends file samples [%ld, %ld) and reads 22.05 kHz samples [%ld, %ld), its window's row holds [%ld, %ld)",
                           k, ra, rb, xa, xb, ws, we);
        const long qa = ra / 2048, qb = (rb - 1) / 2048;
        while (q > 0 && t->host_chunk[q - 1] >= qa) --q;            // a region may start in the chunk its predecessor ended in
        for (long c = qa; c <= qb; ++c) {
            while (q < Q && t->host_chunk[q] < c) ++q;
            if (q >= Q || t->host_chunk[q] != c)
                return SI_FAIL_FN("span %d blends samples [%ld, %ld), the chunk list lacks chunk %ld", k, ra, rb, c);
            if (k < t->host_k0[q] || k >= t->host_k1[q])
                return SI_FAIL_FN("chunk entry %d (chunk %ld) walks spans [%d, %d) and omits span %d, which blends samples [%ld, %ld)",
                               q, c, t->host_k0[q], t->host_k1[q], k, ra, rb);
        }
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    // the tables run 22 050 -> sr: the file is the target axis, so its ratio is (Qr, P)
    const SiRate rt{t->start, t->len, t->span_win, t->span_lim, t->win_ctx, t->win_start, t->win_len, t->win_lim, t->chunk, t->k0, t->k1, t->ramp, fade,
                    SiTaps{f->win, f->dwin, f->nwin, f->num_table, f->step, f->scale, (int)Qr, (int)P, (int)H}, (int)row_cap};
    return si_launch_patch_rate(ctx, orig, si_sample_format(is_pcm16), n_file, inter ? channels : 0, inter ? channel : 0, rt, Q, gen, Lrow, gain, out,
                                static_cast<hipStream_t>(stream));
}

int si_patch_rate(si_ctx* ctx, const void* orig, int is_pcm16, int n_file, int sr, const si_rate_table* table, const float* gen, int Lrow,
                  const float* gain, const si_sinc_filter* filt, void* out, si_stream_t stream) {
    return patch_rate_call(ctx, "si_patch_rate", false, orig, is_pcm16, n_file, 0, 0, sr, table, gen, Lrow, gain, filt, out, stream);
}

int si_patch_rate_ch(si_ctx* ctx, const void* orig, int is_pcm16, int n_file, int channels, int channel, int sr, const si_rate_table* table,
                     const float* gen, int Lrow, const float* gain, const si_sinc_filter* filt, void* out, si_stream_t stream) {
    return patch_rate_call(ctx, "si_patch_rate_ch", true, orig, is_pcm16, n_file, channels, channel, sr, table, gen, Lrow, gain, filt, out, stream);
}

// ---- context clips cut at the file's own sample rate
// One rate's tables of a feed call, sr -> the rate whose ratio to sr is P / Q: the checks every feed puts to a filter, under the
// argument's own name.
static int feed_taps(si_ctx* ctx, const char* fn, const char* arg, const si_sinc_filter* f, long P, long Q, SiTaps* r) {
    if (!f || f->struct_size != (int32_t)sizeof(si_sinc_filter)) return SI_FAIL_FN("%s: si_sinc_filter size mismatch", arg);
    if (!f->win || !f->dwin || f->nwin < 2 || f->num_table < 1 || f->step < 1 || !(f->scale > 0.0 && f->scale <= 1.0))
        return SI_FAIL_FN("%s: bad filter table (nwin %d, num_table %d, step %d, scale %g)", arg, f->nwin, f->num_table, f->step, f->scale);
    *r = SiTaps{f->win, f->dwin, f->nwin, f->num_table, f->step, f->scale, (int)P, (int)Q, (int)(((long)f->nwin + f->step - 1) / f->step)};
    return SI_OK;
}

// ceiling != nullptr is si_cut_rate_valid: the same checks, one more, and the launch that stages invalid samples as +0.0.
static int cut_rate_call(si_ctx* ctx, const char* fn, bool inter, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr,
                         const int32_t* host_start, const int32_t* start, int C, int L, const si_sinc_filter* filt, float* out, si_stream_t stream,
                         const float* ceiling = nullptr) {
    if (!ctx) return SI_EINVAL;
    if ((inter || ceiling) && si_check_channels(ctx, fn, channels, channel, 0) != SI_OK) return SI_EINVAL;
    if (ceiling && !(*ceiling > 0.f)) return SI_FAIL_FN("ceiling = %g is not above 0, or is NaN", (double)*ceiling);
    if (sr < 4000 || sr > 192000) return SI_FAIL_FN("sr = %d Hz, outside 4000 .. 192000", sr);
    if (sr == 22050) return SI_FAIL_FN("sr = 22050 Hz is the model's own rate: that file is si_cut_clips'");
    if (n_file < 1) return SI_FAIL_FN("n_file = %d", n_file);
    if ((long)n_file > SI_MAX_REC) return SI_FAIL_FN("n_file = %d samples, at most %ld", n_file, SI_MAX_REC);
    long P, Qr;
    si_rate_ratio(22050, sr, &P, &Qr);
    const long N22 = ((long)n_file * P + Qr - 1) / Qr;              // the recording's samples on the 22.05 kHz axis, ceil(n_file P / Q)
    if (N22 > SI_MAX_REC) return SI_FAIL_FN("n_file = %d samples at %d Hz are %ld samples at 22050 Hz, at most %ld", n_file, sr, N22, SI_MAX_REC);
    SiFeed fd{};
    if (feed_taps(ctx, fn, "filt", filt, P, Qr, &fd.r) != SI_OK) return SI_EINVAL;
    const long H = fd.r.H;
    const long cap = (RF_TILE - 1) * Qr / P + 2 + 2 * H;            // file samples one tile stages in LDS: 5 581 at 192 kHz with kaiser_best, of 160 KB
    if (cap * (long)sizeof(float) > 65536)
        return SI_FAIL_FN("filt: bad filter table: %ld taps per wing at %d Hz need %ld staged samples per tile, at most 16384", H, sr, cap);
    if (C < 0 || C > 65535) return SI_FAIL_FN("C = %d clips in one call, 0 .. 65535 (the launch grid's second dimension)", C);
    if (L < 1) return SI_FAIL_FN("L = %d", L);
    if (C == 0) return SI_OK;                                       // nothing is read or written
    if (!x || !out || !host_start || !start)
        return SI_FAIL_FN("%s is NULL", !x ? "x" : !out ? "out" : !host_start ? "host_start" : "start");
    for (int c = 0; c < C; ++c) {
        const long s = host_start[c];
        if (s < 0 || s + L > N22)
            return SI_FAIL_FN("start[%d]: clip = 22.05 kHz samples [%ld, %ld) is outside the recording's %ld samples", c, s, s + L, N22);
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    fd.cap = (int)cap, fd.N22 = (int)N22;
    return si_launch_cut_rate(ctx, x, si_sample_format(is_pcm16), n_file, inter ? channels : 0, inter ? channel : 0, start, C, L, fd, ceiling, out,
                              static_cast<hipStream_t>(stream));
}

int si_cut_rate(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int sr, const int32_t* host_start, const int32_t* start, int C, int L,
                const si_sinc_filter* filt, float* out, si_stream_t stream) {
    return cut_rate_call(ctx, "si_cut_rate", false, x, is_pcm16, n_file, 0, 0, sr, host_start, start, C, L, filt, out, stream);
}

int si_cut_rate_ch(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_start,
                   const int32_t* start, int C, int L, const si_sinc_filter* filt, float* out, si_stream_t stream) {
    return cut_rate_call(ctx, "si_cut_rate_ch", true, x, is_pcm16, n_file, channels, channel, sr, host_start, start, C, L, filt, out, stream);
}

// channels = 1 is the mono file (the mono kernel); channels >= 2 reads channel `channel` of the interleaved file: si_dead_runs' convention.
int si_cut_rate_valid(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_start,
                      const int32_t* start, int C, int L, const si_sinc_filter* filt, float ceiling, float* out, si_stream_t stream) {
    return cut_rate_call(ctx, "si_cut_rate_valid", channels >= 2, x, is_pcm16, n_file, channels, channel, sr, host_start, start, C, L, filt, out, stream,
                         &ceiling);
}

// ---- both clip sets of a pass cut straight from the file
// One rate's tables of a pair call: feed_taps, and the bound that lets cut_pair_call form the tile's staged samples.
static int pair_filter(si_ctx* ctx, const char* fn, const char* arg, const si_sinc_filter* f, int target, int sr, SiTaps* r) {
    long P, Q;
    si_rate_ratio(target, sr, &P, &Q);
    if (feed_taps(ctx, fn, arg, f, P, Q, r) != SI_OK) return SI_EINVAL;
    if (r->H > 16384) return SI_FAIL_FN("%s: bad filter table: %ld taps per wing at %d Hz, no tile's staged samples fit 64 KB", arg, (long)r->H, sr);
    return SI_OK;
}

static int cut_pair_call(si_ctx* ctx, const char* fn, bool inter, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr,
                         const int32_t* host_frame, const int32_t* frame, int C, int L22, int L16, const si_sinc_filter* filt22,
                         const si_sinc_filter* filt16, float* out22, float* out16, si_stream_t stream, const float* ceiling = nullptr) {
    if (!ctx) return SI_EINVAL;
    if ((inter || ceiling) && si_check_channels(ctx, fn, channels, channel, 0) != SI_OK) return SI_EINVAL;
    if (ceiling && !(*ceiling > 0.f)) return SI_FAIL_FN("ceiling = %g is not above 0, or is NaN", (double)*ceiling);   // si_cut_pair_valid
    if (sr < 4000 || sr > 192000) return SI_FAIL_FN("sr = %d Hz, outside 4000 .. 192000", sr);
    if (sr == 22050) return SI_FAIL_FN("sr = 22050 Hz is the model's own rate: that file is si_cut_clips'");
    if (n_file < 1) return SI_FAIL_FN("n_file = %d", n_file);
    if ((long)n_file > SI_MAX_REC) return SI_FAIL_FN("n_file = %d samples, at most %ld", n_file, SI_MAX_REC);
    SiPair pr{};
    if (pair_filter(ctx, fn, "filt22", filt22, 22050, sr, &pr.r22) != SI_OK) return SI_EINVAL;
    const long P = pr.r22.P, Qr = pr.r22.Q;
    const long N22 = ((long)n_file * P + Qr - 1) / Qr;              // the recording's samples on the 22.05 kHz axis, ceil(n_file P / Q)
    if (N22 > SI_MAX_REC) return SI_FAIL_FN("n_file = %d samples at %d Hz are %ld samples at 22050 Hz, at most %ld", n_file, sr, N22, SI_MAX_REC);
    if (sr == 16000) {
        if (filt16) return SI_FAIL_FN("filt16 is not NULL at sr = 16000 Hz: the 16 kHz clips are the file's own samples, no filter is applied");
        pr.r16 = SiTaps{nullptr, nullptr, 0, 1, 1, 1.0, 1, 1, 0};
        pr.direct16 = 1;
    } else {
        if (!filt16) return SI_FAIL_FN("filt16 is NULL at sr = %d Hz: only a 16000 Hz file goes without the 16 kHz filter", sr);
        if (pair_filter(ctx, fn, "filt16", filt16, 16000, sr, &pr.r16) != SI_OK) return SI_EINVAL;
    }
    const long N16 = ((long)n_file * pr.r16.P + pr.r16.Q - 1) / pr.r16.Q;      // ceil(n_file P16 / Q16) <= lim16 <= N16 + 1
    const long lim16 = (N22 * 320 + 440) / 441;
    const long H = std::max(pr.r22.H, pr.r16.H);
    const long cap = ((long)RF_PAIR_FRAMES * sr + 49) / 50 + 2 + 2 * H;         // file samples one tile stages in LDS: 5 404 at 192 kHz with kaiser_best
    if (cap * (long)sizeof(float) > 65536)
        return SI_FAIL_FN("%s: bad filter table: %ld taps per wing at %d Hz need %ld staged samples per tile, at most 16384",
                          pr.r22.H >= pr.r16.H ? "filt22" : "filt16", H, sr, cap);
    if (C < 0 || C > 65535) return SI_FAIL_FN("C = %d clips in one call, 0 .. 65535 (the launch grid's second dimension)", C);
    if (L22 < 1) return SI_FAIL_FN("L22 = %d", L22);
    if (L16 < 1) return SI_FAIL_FN("L16 = %d", L16);
    if (C == 0) return SI_OK;                                       // nothing is read or written
    if (!x || !out22 || !out16 || !host_frame || !frame)
        return SI_FAIL_FN("%s is NULL", !x ? "x" : !out22 ? "out22" : !out16 ? "out16" : !host_frame ? "host_frame" : "frame");
    for (int c = 0; c < C; ++c) {
        const long f = host_frame[c];
        if (f < 0 || 441 * f + L22 > N22)
            return SI_FAIL_FN("frame[%d] = %ld: clip = 22.05 kHz samples [%ld, %ld) is outside the recording's %ld samples", c, f, 441 * f,
                              441 * f + L22, N22);
        if (320 * f + L16 > lim16)
            return SI_FAIL_FN("frame[%d] = %ld: clip = 16 kHz samples [%ld, %ld) ends past ceil(N22 320 / 441) = %ld (N22 = %ld)", c, f, 320 * f,
                              320 * f + L16, lim16, N22);
    }
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    pr.cap = (int)cap, pr.N22 = (int)N22, pr.N16 = (int)N16, pr.lim16 = (int)lim16;
    return si_launch_cut_pair(ctx, x, si_sample_format(is_pcm16), n_file, inter ? channels : 0, inter ? channel : 0, frame, C, L22, L16, pr, ceiling, out22,
                              out16, static_cast<hipStream_t>(stream));
}

int si_cut_pair(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int sr, const int32_t* host_frame, const int32_t* frame, int C, int L22,
                int L16, const si_sinc_filter* filt22, const si_sinc_filter* filt16, float* out22, float* out16, si_stream_t stream) {
    return cut_pair_call(ctx, "si_cut_pair", false, x, is_pcm16, n_file, 0, 0, sr, host_frame, frame, C, L22, L16, filt22, filt16, out22, out16,
                         stream);
}

int si_cut_pair_ch(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_frame,
                   const int32_t* frame, int C, int L22, int L16, const si_sinc_filter* filt22, const si_sinc_filter* filt16, float* out22,
                   float* out16, si_stream_t stream) {
    return cut_pair_call(ctx, "si_cut_pair_ch", true, x, is_pcm16, n_file, channels, channel, sr, host_frame, frame, C, L22, L16, filt22, filt16,
                         out22, out16, stream);
}

int si_cut_pair_valid(si_ctx* ctx, const void* x, int is_pcm16, int n_file, int channels, int channel, int sr, const int32_t* host_frame,
                      const int32_t* frame, int C, int L22, int L16, const si_sinc_filter* filt22, const si_sinc_filter* filt16, float ceiling,
                      float* out22, float* out16, si_stream_t stream) {
    return cut_pair_call(ctx, "si_cut_pair_valid", channels >= 2, x, is_pcm16, n_file, channels, channel, sr, host_frame, frame, C, L22, L16, filt22,
                         filt16, out22, out16, stream, &ceiling);
}

// ---- dropout detection
// The detector's scratch for n samples: the context's own, grown on demand (a context is single-threaded and its calls stream-ordered by contract).
static int det_scratch_reserve(si_ctx* ctx, int n, si_stream_t stream) {
    const size_t need = si_detect_scratch_bytes(n);
    if (need > ctx->det_scratch_cap) {
        if (ctx->det_scratch) { SI_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream))); SI_HIP_CHECK(hipFree(ctx->det_scratch)); ctx->det_scratch = nullptr; ctx->det_scratch_cap = 0; }
        const size_t cap = std::max(need, (size_t)1 << 20);
        SI_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx->det_scratch), cap));
        ctx->det_scratch_cap = cap;
    }
    return SI_OK;
}

// What si_quiet_runs and its siblings refuse, in one order.
static int quiet_runs_check(si_ctx* ctx, const char* fn, bool inter, const void* x, int n, int channels, int channel, float threshold, int min_len,
                            const int32_t* runs, int max_runs, const int32_t* n_runs) {
    if (inter && si_check_channels(ctx, fn, channels, channel, -1) != SI_OK) return SI_EINVAL;
    if (!x) return SI_FAIL_FN("x is NULL");
    if (!n_runs) return SI_FAIL_FN("n_runs is NULL");
    if (max_runs < 0) return SI_FAIL_FN("max_runs = %d is negative", max_runs);
    if (!runs && max_runs > 0) return SI_FAIL_FN("runs is NULL with max_runs = %d", max_runs);
    if (n < 1 || (long)n > SI_MAX_REC) return SI_FAIL_FN("n = %d samples, outside 1 .. %ld", n, SI_MAX_REC);
    if (!(threshold >= 0.f)) return SI_FAIL_FN("threshold = %g is negative or NaN", (double)threshold);
    if (min_len < 1) return SI_FAIL_FN("min_len = %d samples, at least 1", min_len);
    return SI_OK;
}

// The two range checks that more than one route makes, each with its one text.
static int check_finite_threshold(si_ctx* ctx, const char* fn, float threshold) {
    return __builtin_isinf(threshold) ? SI_FAIL_FN("threshold = %g is not finite", (double)threshold) : SI_OK;
}
static int check_rel_threshold(si_ctx* ctx, const char* fn, float rel_threshold, float top) {       // top: 1 (a fraction of the peak) or 4 (|d| <= 4 * peak)
    if (rel_threshold >= 0.f && rel_threshold <= top) return SI_OK;
    return top == 1.f ? SI_FAIL_FN("rel_threshold = %g is NaN or outside [0, 1]", (double)rel_threshold)
                      : SI_FAIL_FN("rel_threshold = %g is NaN or outside [0, 4]", (double)rel_threshold);
}

// What route d.route alone refuses, in that route's order.  A new detector adds its case here.
static int detect_route_check(si_ctx* ctx, const char* fn, const SiDetect& d, float threshold) {
    switch (d.route) {
    case SI_DET_DEAD:
        if (d.kind < 1 || d.kind > 3) return SI_FAIL_FN("kind = %d, outside 1 .. 3 (SI_DEAD_QUIET | SI_DEAD_HELD)", d.kind);
        if (check_rel_threshold(ctx, fn, d.rel, 1.f) != SI_OK) return SI_EINVAL;
        if (!(d.tol >= 0.f)) return SI_FAIL_FN("held_tol = %g is negative or NaN", (double)d.tol);
        return SI_OK;
    case SI_DET_LEVEL:
    case SI_DET_BURST:                                                 // the same window; a second difference reaches 4 * the peak
        if (d.half < 0 || d.half > SI_LEVEL_MAX_HALF) return SI_FAIL_FN("half = %d samples, outside 0 .. SI_LEVEL_MAX_HALF = %d", d.half, SI_LEVEL_MAX_HALF);
        if (check_finite_threshold(ctx, fn, threshold) != SI_OK) return SI_EINVAL;
        return check_rel_threshold(ctx, fn, d.rel, d.route == SI_DET_LEVEL ? 1.f : 4.f);
    case SI_DET_INVALID:
        if (!(d.ceiling > 0.f)) return SI_FAIL_FN("ceiling = %g is not above 0, or is NaN", (double)d.ceiling);
        return SI_OK;
    case SI_DET_IMPULSE:
        if (d.order < 2 || d.order > SI_IMPULSE_MAX_ORDER) return SI_FAIL_FN("order = %d, outside 2 .. SI_IMPULSE_MAX_ORDER = %d", d.order, SI_IMPULSE_MAX_ORDER);
        if (d.guard < 0 || d.guard > SI_IMPULSE_MAX_GUARD) return SI_FAIL_FN("guard = %d samples, outside 0 .. SI_IMPULSE_MAX_GUARD = %d", d.guard, SI_IMPULSE_MAX_GUARD);
        if (d.half < d.guard + 1 || d.half > SI_IMPULSE_MAX_HALF)
            return SI_FAIL_FN("half = %d samples, outside guard + 1 = %d .. SI_IMPULSE_MAX_HALF = %d", d.half, d.guard + 1, SI_IMPULSE_MAX_HALF);
        if (d.pad < 0 || d.pad > SI_IMPULSE_MAX_PAD) return SI_FAIL_FN("pad = %d samples, outside 0 .. SI_IMPULSE_MAX_PAD = %d", d.pad, SI_IMPULSE_MAX_PAD);
        if (d.half + d.pad > SI_IMPULSE_MAX_HALF) return SI_FAIL_FN("half + pad = %d samples, above SI_IMPULSE_MAX_HALF = %d", d.half + d.pad, SI_IMPULSE_MAX_HALF);
        if (!(d.ratio >= 1.f && d.ratio <= 1e6f)) return SI_FAIL_FN("ratio = %g is NaN or outside [1, 1e6]", (double)d.ratio);
        if (check_finite_threshold(ctx, fn, threshold) != SI_OK) return SI_EINVAL;
        return check_rel_threshold(ctx, fn, d.rel, 4.f);
    default:
        return SI_OK;                                                  // SI_DET_QUIET: nothing of its own
    }
}

// One detection call: what every detector refuses, then what the route alone refuses, and only then the device: the
// scratch and the route's launches.  inter = false is si_quiet_runs, the one entry point with no channels.
static int detect_call(si_ctx* ctx, const char* fn, bool inter, const void* x, int is_pcm16, int n, int channels, int channel, float threshold, int min_len,
                       int32_t* runs, int max_runs, int32_t* n_runs, si_stream_t stream, const SiDetect& d) {
    if (!ctx) return SI_EINVAL;
    if (quiet_runs_check(ctx, fn, inter, x, n, channels, channel, threshold, min_len, runs, max_runs, n_runs) != SI_OK) return SI_EINVAL;
    if (detect_route_check(ctx, fn, d, threshold) != SI_OK) return SI_EINVAL;
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = det_scratch_reserve(ctx, n, stream)) return rc;
    return si_launch_detect(ctx, x, si_sample_format(is_pcm16), n, inter ? channels : 0, inter ? channel : 0, threshold, min_len, runs, max_runs, n_runs,
                            ctx->det_scratch, static_cast<hipStream_t>(stream), d);
}

int si_quiet_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, float threshold, int min_len, int32_t* runs, int max_runs, int32_t* n_runs,
                  si_stream_t stream) {
    const SiDetect d{SI_DET_QUIET};
    return detect_call(ctx, "si_quiet_runs", false, x, is_pcm16, n, 0, 0, threshold, min_len, runs, max_runs, n_runs, stream, d);
}

int si_quiet_runs_ch(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, float threshold, int min_len, int32_t* runs,
                     int max_runs, int32_t* n_runs, si_stream_t stream) {
    const SiDetect d{SI_DET_QUIET};
    return detect_call(ctx, "si_quiet_runs_ch", true, x, is_pcm16, n, channels, channel, threshold, min_len, runs, max_runs, n_runs, stream, d);
}

// ---- held-sample and peak-relative dropouts
int si_dead_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int kind, float threshold, float rel_threshold,
                 float held_tol, int min_len, int32_t* runs, int max_runs, int32_t* n_runs, float* threshold_out, si_stream_t stream) {
    SiDetect d{SI_DET_DEAD};
    d.kind = kind, d.rel = rel_threshold, d.tol = held_tol, d.thr_out = threshold_out;
    return detect_call(ctx, "si_dead_runs", true, x, is_pcm16, n, channels, channel, threshold, min_len, runs, max_runs, n_runs, stream, d);
}

// ---- dropouts by windowed RMS level
int si_level_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int half, float threshold, float rel_threshold,
                  int min_len, int32_t* runs, int max_runs, int32_t* n_runs, float* threshold_out, si_stream_t stream) {
    const SiDetect d{SI_DET_LEVEL, rel_threshold, threshold_out, half};
    return detect_call(ctx, "si_level_runs", true, x, is_pcm16, n, channels, channel, threshold, min_len, runs, max_runs, n_runs, stream, d);
}

// ---- corrupted blocks by second-difference level
int si_burst_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int half, float threshold, float rel_threshold,
                  int min_len, int32_t* runs, int max_runs, int32_t* n_runs, float* threshold_out, si_stream_t stream) {
    const SiDetect d{SI_DET_BURST, rel_threshold, threshold_out, half};
    return detect_call(ctx, "si_burst_runs", true, x, is_pcm16, n, channels, channel, threshold, min_len, runs, max_runs, n_runs, stream, d);
}

// ---- NaN, inf and out-of-range samples: no threshold, so none is checked and none reaches a kernel
int si_invalid_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, float ceiling, int min_len, int32_t* runs,
                    int max_runs, int32_t* n_runs, si_stream_t stream) {
    SiDetect d{SI_DET_INVALID};
    d.ceiling = ceiling;
    return detect_call(ctx, "si_invalid_runs", true, x, is_pcm16, n, channels, channel, 0.f, min_len, runs, max_runs, n_runs, stream, d);
}

// ---- clicks and pops by locally scaled AR prediction error
int si_impulse_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int order, int half, int guard, int pad,
                    float ratio, float threshold, float rel_threshold, int min_len, int32_t* runs, int max_runs, int32_t* n_runs,
                    float* threshold_out, si_stream_t stream) {
    SiDetect d{SI_DET_IMPULSE};
    d.order = order, d.half = half, d.guard = guard, d.pad = pad, d.ratio = ratio, d.rel = rel_threshold, d.thr_out = threshold_out;
    return detect_call(ctx, "si_impulse_runs", true, x, is_pcm16, n, channels, channel, threshold, min_len, runs, max_runs, n_runs, stream, d);
}

int si_impulse_residual(si_ctx* ctx, const void* x, int is_pcm16, int n, int channels, int channel, int order, double* e, si_stream_t stream) {
    const char* fn = "si_impulse_residual";
    if (!ctx) return SI_EINVAL;
    if (si_check_channels(ctx, fn, channels, channel, 0) != SI_OK) return SI_EINVAL;
    if (!x) return SI_FAIL_FN("x is NULL");
    if (!e) return SI_FAIL_FN("e is NULL");
    if (n < 1 || (long)n > SI_MAX_REC) return SI_FAIL_FN("n = %d samples, outside 1 .. %ld", n, SI_MAX_REC);
    if (order < 2 || order > SI_IMPULSE_MAX_ORDER) return SI_FAIL_FN("order = %d, outside 2 .. SI_IMPULSE_MAX_ORDER = %d", order, SI_IMPULSE_MAX_ORDER);
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_impulse_residual(ctx, x, si_sample_format(is_pcm16), n, channels, channel, order, e, static_cast<hipStream_t>(stream));
}

// ---- short runs mended in place by least-squares AR interpolation
int si_mend_runs(si_ctx* ctx, void* x, int is_pcm16, int n, int channels, int channel, const int32_t* runs, int n_runs, int max_len,
                 int order, int context, int32_t* status, si_stream_t stream) {
    const char* fn = "si_mend_runs";
    if (!ctx) return SI_EINVAL;
    if (si_check_channels(ctx, fn, channels, channel, 0) != SI_OK) return SI_EINVAL;
    if (!x) return SI_FAIL_FN("x is NULL");
    if (n < 1 || (long)n > SI_MAX_REC) return SI_FAIL_FN("n = %d samples, outside 1 .. %ld", n, SI_MAX_REC);
    if (n_runs < 0 || n_runs > SI_MEND_MAX_RUNS) return SI_FAIL_FN("n_runs = %d rows, outside 0 .. SI_MEND_MAX_RUNS = %d", n_runs, SI_MEND_MAX_RUNS);
    if (!runs && n_runs > 0) return SI_FAIL_FN("runs is NULL with n_runs = %d", n_runs);
    if (!status && n_runs > 0) return SI_FAIL_FN("status is NULL with n_runs = %d", n_runs);
    if (max_len < 1 || max_len > SI_MEND_MAX_LEN) return SI_FAIL_FN("max_len = %d samples, outside 1 .. SI_MEND_MAX_LEN = %d", max_len, SI_MEND_MAX_LEN);
    if (order < 2 || order > SI_MEND_MAX_ORDER) return SI_FAIL_FN("order = %d, outside 2 .. SI_MEND_MAX_ORDER = %d", order, SI_MEND_MAX_ORDER);
    if (context < 4 * order || context > SI_MEND_MAX_CONTEXT)
        return SI_FAIL_FN("context = %d samples, outside 4 * order = %d .. SI_MEND_MAX_CONTEXT = %d", context, 4 * order, SI_MEND_MAX_CONTEXT);
    if (n_runs == 0) return SI_OK;
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    return si_launch_mend_runs(ctx, x, si_sample_format(is_pcm16), n, channels, channel, runs, n_runs, max_len, order, context, status,
                               static_cast<hipStream_t>(stream));
}

#undef SI_FAIL_FN

}  // extern "C"

extern "C" {

int si_profile_start(si_ctx* ctx, int max_launches) {
    if (!ctx || max_launches <= 0) return si_fail(ctx, SI_EINVAL, "si_profile_start: bad argument");
    SI_HIP_CHECK(hipSetDevice(ctx->device));
    while (ctx->prof_pool.size() < (size_t)max_launches * 2) {
        hipEvent_t e;
        SI_HIP_CHECK(hipEventCreate(&e));
        ctx->prof_pool.push_back(e);
    }
    ctx->prof_recs.clear();
    ctx->prof_names.clear();
    ctx->prof_used = 0;
    ctx->prof_open = -1;
    ctx->prof_on = true;
    return SI_OK;
}

int si_profile_filter(si_ctx* ctx, const char* family) {
    if (!ctx) return SI_EINVAL;
    ctx->prof_filter = family ? family : "";
    return SI_OK;
}

int si_profile_stop(si_ctx* ctx, si_profile_entry* out, int capacity, int* count) {
    if (!ctx || !count) return si_fail(ctx, SI_EINVAL, "si_profile_stop: bad argument");
    ctx->prof_on = false;
    std::vector<si_profile_entry> agg(ctx->prof_names.size());
    for (size_t i = 0; i < agg.size(); ++i) {
        memset(&agg[i], 0, sizeof(si_profile_entry));
        snprintf(agg[i].name, sizeof(agg[i].name), "%s", ctx->prof_names[i].c_str());
    }
    for (const auto& r : ctx->prof_recs) {
        SI_HIP_CHECK(hipEventSynchronize(r.b));
        float ms = 0.f;
        SI_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
        si_profile_entry& e = agg[r.name];
        e.launches += 1; e.ms += ms; e.flops += r.flops; e.bytes += r.bytes;
    }
    *count = (int)agg.size();
    for (int i = 0; i < (int)agg.size() && i < capacity && out; ++i) out[i] = agg[i];
    ctx->prof_recs.clear();
    ctx->prof_used = 0;
    return SI_OK;
}

int si_debug_capture(si_ctx* ctx, const char* name, float* dst, long capacity) {
    if (!ctx || !name) return SI_EINVAL;
    if (!dst || capacity <= 0) ctx->dbg_capture.erase(name);
    else ctx->dbg_capture[name] = {dst, capacity};
    return SI_OK;
}

long si_debug_size(si_ctx* ctx, const char* name) {
    if (!ctx || !name) return SI_EINVAL;
    auto it = ctx->dbg_size.find(name);
    if (it == ctx->dbg_size.end()) return si_fail(ctx, SI_EINVAL, "no intermediate named '%s' in the last forward", name);
    return it->second;
}

int si_debug_ws_regions(si_ctx* ctx, int which, si_ws_region* out, int capacity, int* count) {
    if (!ctx || !count || capacity < 0 || (capacity > 0 && !out)) return si_fail(ctx, SI_EINVAL, "si_debug_ws_regions: NULL / bad argument");
    if (which < SI_WS_ENCODER || which > SI_WS_MEL) return si_fail(ctx, SI_EINVAL, "si_debug_ws_regions: pass %d unknown (0 encoder, 1 generator, 2 mel)", which);
    const si_ctx::WsLog& log = ctx->ws_log[which];
    *count = log.n;
    for (int i = 0; i < log.n && i < capacity; ++i) {
        snprintf(out[i].name, sizeof(out[i].name), "%s", log.r[i].name);
        out[i].offset = log.r[i].offset; out[i].bytes = log.r[i].bytes;
    }
    return SI_OK;
}

}  // extern "C"
