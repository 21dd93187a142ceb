// weights_host.cpp -- descriptor check, layout plan and checkpoint packer (weights_host.h).  Plain host C++: no HIP header,
// so the unit also builds with a host compiler under sanitizers (the `packcheck` target).
//
// Host-side work done here, once per checkpoint load:
//   * weight-norm folding, w = g * v / ||v||  (generator convs: norm over all dims but 0,
//     I_ea/hifi_gan/models.py:125-132; positional conv: over all dims but 2, modeling_hubert.py:78)
//   * re-layout of every Conv1d / ConvTranspose1d / Linear weight into the tap-GEMM form
//     W[group][tap][n][ci] (ci contiguous), q/k/v fused into one (3H, H) matrix, ConvTranspose1d split into
//     its `stride` output phases (n = phase*Cout + co, taps q = 0..k/stride-1 read input row u-q)
//   * conversion to the arithmetic of the model desc (fp32 / bf16 / bf16 hi+lo / fp16)
//   * codebook tables: centred centroids, 1/||centred||, raw centroids (I_ea/loss_fn.py:10-14)
// What the packer refuses (SI_EWEIGHTS, naming the tensor or the index line): an empty or malformed index, more than 8 dims, a
// negative dim, dims whose product overflows, an offset that is negative, misaligned or past the blob, a name given twice, a
// missing or mis-shaped tensor, a weight-norm magnitude vector of the wrong count, a module with neither `.weight` nor a
// weight-norm pair, a weight-norm row of zero norm, and a non-finite value in anything that is packed (tested on the fp32 value
// before the cast: a finite weight beyond +-65504 is still clamped silently in the fp16 mode, as documented).
#include "weights_host.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <sstream>
#include <string>

namespace siw {

char g_create_err[512] = "";

bool env_flag(const char* name) { const char* v = getenv(name); return v ? atoi(v) != 0 : true; }
PackOpts pack_opts_from_env() { PackOpts o; o.voc_opready = env_flag("SI_VOC_OPREADY"); o.voc_res16 = env_flag("SI_VOC_RES16"); return o; }

int fail(Err e, int code, const char* fmt, ...) {
    if (e.buf && e.cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(e.buf, e.cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

// ------------------------------------------------------------------------------------------------ descriptor
namespace {
bool in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }
}  // namespace

int check_desc(const si_model_desc* d, Err e) {
    if (!d || d->struct_size != (int32_t)sizeof(si_model_desc))
        return fail(e, SI_EINVAL, "si_model_desc size mismatch (struct_size=%d, library expects %zu)", d ? d->struct_size : -1, sizeof(si_model_desc));
    if (!in_range(d->num_conv, 2, SI_MAX_CONV)) return fail(e, SI_EINVAL, "num_conv=%d out of range 2..%d", d->num_conv, SI_MAX_CONV);
    if (!in_range(d->num_ups, 1, SI_MAX_UPS)) return fail(e, SI_EINVAL, "num_ups=%d out of range 1..%d", d->num_ups, SI_MAX_UPS);
    if (!in_range(d->num_rb, 1, SI_MAX_RB)) return fail(e, SI_EINVAL, "num_rb=%d: resblock shape out of range 1..%d", d->num_rb, SI_MAX_RB);
    if (!in_range(d->num_dil, 1, SI_MAX_DIL)) return fail(e, SI_EINVAL, "num_dil=%d: resblock shape out of range 1..%d", d->num_dil, SI_MAX_DIL);
    if (!in_range(d->hidden_size, 64, 4096) || d->hidden_size % 64)
        return fail(e, SI_EINVAL, "hidden_size=%d must be a multiple of 64 in 64..4096", d->hidden_size);
    if (d->num_heads != d->hidden_size / 64)                 // (no product: num_heads may be anything)
        return fail(e, SI_EINVAL, "hidden_size=%d / num_heads=%d: the attention kernel needs head_dim 64", d->hidden_size, d->num_heads);
    if (!in_range(d->num_layers, 1, 64)) return fail(e, SI_EINVAL, "num_layers=%d out of range 1..64", d->num_layers);
    if (!in_range(d->intermediate_size, 16, 16384) || d->intermediate_size % 16)
        return fail(e, SI_EINVAL, "intermediate_size=%d must be a multiple of 16 in 16..16384", d->intermediate_size);
    if (d->pos_conv_groups <= 0 || d->hidden_size % d->pos_conv_groups || (d->hidden_size / d->pos_conv_groups) % 16)
        return fail(e, SI_EINVAL, "pos_conv_groups=%d: positional conv: hidden/groups must be a multiple of 16", d->pos_conv_groups);
    if (!in_range(d->pos_conv_kernel, 1, 1024)) return fail(e, SI_EINVAL, "pos_conv_kernel=%d out of range 1..1024", d->pos_conv_kernel);
    for (int i = 0; i < d->num_conv; ++i) {
        if (!in_range(d->conv_dim[i], 16, 4096) || d->conv_dim[i] % 16)
            return fail(e, SI_EINVAL, "conv_dim[%d]=%d must be a multiple of 16 in 16..4096", i, d->conv_dim[i]);
        if (!in_range(d->conv_kernel[i], 1, 1024)) return fail(e, SI_EINVAL, "conv_kernel[%d]=%d out of range 1..1024", i, d->conv_kernel[i]);
        if (!in_range(d->conv_stride[i], 1, 1024)) return fail(e, SI_EINVAL, "conv_stride[%d]=%d out of range 1..1024", i, d->conv_stride[i]);
    }
    // Widths that pass the ranges above and that a kernel of the first forward refuses (the launchers keep their own checks):
    // the waveform conv is written for HuBERT's 10 taps and 4 * 2^j channels (conv0_check), a LayerNorm row lives in 8 registers
    // of 256 lanes (si_launch_layernorm).
    if (d->conv_kernel[0] != 10) return fail(e, SI_EINVAL, "conv_kernel[0]=%d: the waveform conv kernel is written for 10 taps", d->conv_kernel[0]);
    if (d->conv_dim[0] > 1024 || (d->conv_dim[0] & (d->conv_dim[0] - 1)))
        return fail(e, SI_EINVAL, "conv_dim[0]=%d: the waveform conv kernel needs 4 * 2^j channels, at most 1024", d->conv_dim[0]);
    if (d->hidden_size > SI_LN_MAX_WIDTH) return fail(e, SI_EINVAL, "hidden_size=%d: a LayerNorm row is at most %d wide", d->hidden_size, SI_LN_MAX_WIDTH);
    for (int i = 0; i < d->num_conv; ++i) {
        const bool normed = d->feat_norm_layer || (i == d->num_conv - 1 && d->feat_proj_layer_norm);
        if (normed && d->conv_dim[i] > SI_LN_MAX_WIDTH)
            return fail(e, SI_EINVAL, "conv_dim[%d]=%d: a LayerNorm row is at most %d wide", i, d->conv_dim[i], SI_LN_MAX_WIDTH);
    }
    if (!(std::isfinite(d->layer_norm_eps) && d->layer_norm_eps > 0.f))
        return fail(e, SI_EINVAL, "layer_norm_eps=%g must be finite and > 0", (double)d->layer_norm_eps);
    if (!in_range(d->codebook_dim, 1, 128)) return fail(e, SI_EINVAL, "codebook_dim=%d out of range 1..128 (codebook unsupported)", d->codebook_dim);
    if (!in_range(d->num_clusters, 1, 65536)) return fail(e, SI_EINVAL, "num_clusters=%d out of range 1..65536 (codebook unsupported)", d->num_clusters);
    if (!in_range(d->num_mels, 1, 4096)) return fail(e, SI_EINVAL, "num_mels=%d out of range 1..4096", d->num_mels);
    if (!in_range(d->up_initial_channel, 32, 8192)) return fail(e, SI_EINVAL, "up_initial_channel=%d out of range 32..8192", d->up_initial_channel);
    int c = d->up_initial_channel;
    long hop = 1;
    for (int i = 0; i < d->num_ups; ++i) {
        if (!in_range(d->up_rates[i], 1, 64)) return fail(e, SI_EINVAL, "up_rates[%d]=%d out of range 1..64", i, d->up_rates[i]);
        // output length rate * L needs padding (k - u) / 2 exact; k need not be a multiple of u (I_da's 11 / 5)
        if (!in_range(d->up_kernels[i], d->up_rates[i], 1024) || (d->up_kernels[i] - d->up_rates[i]) % 2)
            return fail(e, SI_EINVAL, "up_kernels[%d]=%d: upsample kernel must be in rate %d .. 1024 with an even difference", i, d->up_kernels[i], d->up_rates[i]);
        if (c % 32) return fail(e, SI_EINVAL, "up_initial_channel=%d: upsample %d has %d input channels, which must be a multiple of 32", d->up_initial_channel, i, c);
        c /= 2;
        hop *= d->up_rates[i];
        if (hop > 65536) return fail(e, SI_EINVAL, "up_rates[%d]=%d: the product of the rates up to here is %ld, above 65536", i, d->up_rates[i], hop);
    }
    if (c % 4) return fail(e, SI_EINVAL, "up_initial_channel=%d: final generator width %d must be a multiple of 4", d->up_initial_channel, c);
    // conv_post_kernel keeps 256 + 6 rows of c + 4 floats and its 7 taps of c weights in LDS (si_launch_conv_post)
    if (((size_t)(256 + 6) * (c + 4) + (size_t)7 * c) * 4 > SI_POST_MAX_LDS)
        return fail(e, SI_EINVAL, "up_initial_channel=%d: final generator width %d is more than conv_post holds in LDS (at most 148 channels)", d->up_initial_channel, c);
    for (int j = 0; j < d->num_rb; ++j) {
        if (!in_range(d->rb_kernels[j], 1, 255) || d->rb_kernels[j] % 2 == 0)
            return fail(e, SI_EINVAL, "rb_kernels[%d]=%d: resblock kernel must be odd in 1..255", j, d->rb_kernels[j]);
        for (int n = 0; n < d->num_dil; ++n)
            if (!in_range(d->rb_dilations[j][n], 1, 4096)) return fail(e, SI_EINVAL, "rb_dilations[%d][%d]=%d out of range 1..4096", j, n, d->rb_dilations[j][n]);
    }
    if (!in_range(d->resblock_type, 0, 2)) return fail(e, SI_EINVAL, "resblock_type=%d: 1 (ResBlock1) or 2 (ResBlock2)", d->resblock_type);
    if (!in_range(d->encoder_math, SI_MATH_F32, SI_MATH_F16)) return fail(e, SI_EINVAL, "encoder_math=%d: unknown math mode", d->encoder_math);
    if (!in_range(d->vocoder_math, SI_MATH_F32, SI_MATH_F16)) return fail(e, SI_EINVAL, "vocoder_math=%d: unknown math mode", d->vocoder_math);
    return SI_OK;
}

// ------------------------------------------------------------------------------------------------ layout
namespace {

size_t elem_bytes(int math) { return math == SI_MATH_F32 ? 4 : 2; }

struct Planner {
    size_t cur = 0;
    size_t take(size_t bytes) { size_t o = cur; cur += (bytes + 255) / 256 * 256; return o; }
    size_t floats(size_t n) { return take(n * 4); }
    GemmW gemm(int math, int groups, int ntaps, int N, int Cin, bool bias) {
        GemmW g;
        g.math = math; g.groups = groups; g.ntaps = ntaps; g.N = N; g.Cin = Cin; g.has_bias = bias;
        g.Npad = si_round_up(N, si_pick_bn(N));
        const size_t n = (size_t)groups * ntaps * g.Npad * Cin;
        g.w = take(n * elem_bytes(math));
        if (math == SI_MATH_BF16X3) g.w_lo = take(n * 2);
        if (bias) g.bias = floats((size_t)groups * N);
        return g;
    }
};

}  // namespace

// Channel count of upsampling stage i as the kernels see it.  On the fp16 activation stream a stage narrower than 32 channels
// (I_da's unit vocoder ends on 16) is carried PADDED to 32: its weights, biases and therefore activations are zero in the extra
// channels, and the stage runs on the 32-channel chain kernel (three launches per stage) instead of 18 tap-GEMM launches that
// move the stream at a tenth of the HBM rate; `conv_post` reads the padded rows with zero weights.  Other modes keep the real width
// (their per-stage taps are compared against the reference's tensors).
int stage_channels(const si_model_desc& d, const PackOpts& o, int i) {
    const int real = d.up_initial_channel >> (i + 1);
    const bool r16 = o.voc_opready && o.voc_res16 && d.vocoder_math == SI_MATH_F16;
    return (r16 && real < 32 && real >= 4) ? 32 : real;
}

int plan_layout(const si_model_desc& d, const PackOpts& o, Layout& L) {
    Planner P;
    P.take(256);                                           // offset 0 is reserved to mean "absent"
    const int em = d.encoder_math, vm = d.vocoder_math;
    const int H = d.hidden_size;
    // encoder
    L.conv0_w = P.floats((size_t)d.conv_dim[0] * d.conv_kernel[0]);
    L.conv0_bias = d.conv_bias ? P.floats(d.conv_dim[0]) : 0;
    L.conv0_g = P.floats(d.conv_dim[0]);
    L.conv0_b = P.floats(d.conv_dim[0]);
    L.convs.clear();
    for (int i = 1; i < d.num_conv; ++i) {
        ConvW c;
        c.g = P.gemm(em, 1, d.conv_kernel[i], d.conv_dim[i], d.conv_dim[i - 1], d.conv_bias != 0);
        if (d.feat_norm_layer) { c.ln_g = P.floats(d.conv_dim[i]); c.ln_b = P.floats(d.conv_dim[i]); }
        L.convs.push_back(c);
    }
    const int CF = d.conv_dim[d.num_conv - 1];
    L.fp_ln_g = P.floats(CF); L.fp_ln_b = P.floats(CF);
    L.proj = P.gemm(em, 1, 1, H, CF, true);
    L.pos = P.gemm(em, d.pos_conv_groups, d.pos_conv_kernel, H / d.pos_conv_groups, H / d.pos_conv_groups, true);
    L.enc_ln_g = P.floats(H); L.enc_ln_b = P.floats(H);
    L.layers.clear();
    for (int l = 0; l < d.num_layers; ++l) {
        LayerW w;
        w.qkv = P.gemm(em, 1, 1, 3 * H, H, true);
        w.out = P.gemm(em, 1, 1, H, H, true);
        w.ln1_g = P.floats(H); w.ln1_b = P.floats(H);
        w.ffn1 = P.gemm(em, 1, 1, d.intermediate_size, H, true);
        w.ffn2 = P.gemm(em, 1, 1, H, d.intermediate_size, true);
        w.ln2_g = P.floats(H); w.ln2_b = P.floats(H);
        L.layers.push_back(w);
    }
    L.head_ln_g = P.floats(H); L.head_ln_b = P.floats(H);
    L.head = P.gemm(SI_MATH_F32, 1, 1, d.codebook_dim, H, true);       // the arg-max input stays fp32
    L.cb_centered = P.floats((size_t)d.num_clusters * d.codebook_dim);
    L.cb_raw = P.floats((size_t)d.num_clusters * d.codebook_dim);
    L.cb_rnorm = P.floats(d.num_clusters);
    // vocoder
    L.mel_ld = si_round_up(d.num_mels, 32);
    const int C0 = d.up_initial_channel;
    L.pre = P.gemm(vm, 1, 7, C0, L.mel_ld, true);
    L.ups.clear(); L.rbs.clear();
    int c = C0;
    for (int i = 0; i < d.num_ups; ++i) {
        const int u = d.up_rates[i], k = d.up_kernels[i], cout = stage_channels(d, o, i);
        L.ups.push_back(P.gemm(vm, 1, (k + u - 1) / u, u * cout, c, true));   // taps q = j div u; absent (phase, tap) pairs stay zero
        c = cout;
        for (int j = 0; j < d.num_rb; ++j) {
            ResW r;
            for (int n = 0; n < d.num_dil; ++n) {
                r.c1[n] = P.gemm(vm, 1, d.rb_kernels[j], c, c, true);
                if (d.resblock_type != 2) r.c2[n] = P.gemm(vm, 1, d.rb_kernels[j], c, c, true);   // ResBlock2 has one conv per dilation
            }
            L.rbs.push_back(r);
        }
    }
    L.post_C = c;
    L.post_w = P.floats((size_t)7 * c);
    L.post_b = P.floats(1);
    L.total = P.cur;
    return SI_OK;
}

// The packed blob's layout is a function of the model desc AND of the arithmetic-path options (stage_channels: the padded widths
// of the fp16 stream).  A rank that receives the blob by broadcast must have planned the SAME layout as the rank that packed it;
// the first 32 bytes of the blob carry a fingerprint of the plan so that a mismatch is an error instead of silently mis-read weights.
uint64_t layout_fingerprint(const si_model_desc& d, const PackOpts& o, const Layout& L) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
    mix(&d, sizeof(d));
    const uint64_t total = L.total; mix(&total, 8);
    for (int i = 0; i < d.num_ups; ++i) { const int c = stage_channels(d, o, i); mix(&c, 4); mix(&L.ups[i].w, sizeof(size_t)); }
    mix(&L.post_w, sizeof(size_t)); mix(&L.post_C, 4); mix(&L.cb_raw, sizeof(size_t)); mix(&L.head.w, sizeof(size_t));
    return h;
}
BlobHeader blob_header(const si_model_desc& d, const PackOpts& o, const Layout& L) {
    return BlobHeader{BLOB_MAGIC, (uint32_t)SI_ABI_VERSION, layout_fingerprint(d, o, L), (uint64_t)L.total, 0};
}

// ---- host packing helpers ------------------------------------------------------------------------
unsigned short h_f2bf(float f) {
    unsigned u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
// fp32 -> fp16, round to nearest even, saturating at +-65504 (NaN stays NaN).  Integer arithmetic, so that every host compiler
// builds it (g++ has no _Float16 in C++) and gives the bits of the hardware conversion.
unsigned short h_f2h(float f) {
    if (f != f) return 0x7e00;
    const float c = f > 65504.f ? 65504.f : (f < -65504.f ? -65504.f : f);
    unsigned u; memcpy(&u, &c, 4);
    const unsigned short sign = (unsigned short)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u >= 0x38800000u) {                                // >= 2^-14: a normal fp16; rebias the exponent, round off 13 bits
        u -= 0x38000000u;
        return (unsigned short)(sign | ((u + 0xFFFu + ((u >> 13) & 1u)) >> 13));
    }
    if (u < 0x33000000u) return sign;                      // < 2^-25: zero (2^-25 itself is the tie below, to even = zero)
    const int shift = 126 - (int)(u >> 23);                // subnormal fp16: in units of 2^-24, 14 <= shift <= 24
    const unsigned m = (u & 0x7fffffu) | 0x800000u, half = 1u << (shift - 1), rem = m & ((1u << shift) - 1u);
    unsigned q = m >> shift;
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return (unsigned short)(sign | q);
}
float h_bf2f(unsigned short h) { unsigned u = ((unsigned)h) << 16; float f; memcpy(&f, &u, 4); return f; }

namespace {

struct HostTensor {
    const float* data = nullptr;
    std::vector<long> shape;
    size_t n = 0;                        // element count, computed with an overflow check by parse_index
    long numel() const { return (long)n; }
};

// The packer runs twice over the same code: a DRY pass that only looks tensors up and compares shapes (no image exists yet),
// then, once nothing is missing, the pass that writes.
struct Packer {
    Err err;
    std::map<std::string, HostTensor> t;
    std::vector<char>* img = nullptr;
    bool dry = true;
    int rc = SI_OK;

    char* base() { return img->data(); }
    bool all_finite(const std::string& name, const float* p, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(p[i])) {
                if (!rc) rc = fail(err, SI_EWEIGHTS, "tensor '%s' holds a non-finite value (%g at element %zu)", name.c_str(), (double)p[i], i);
                return false;
            }
        return true;
    }
    const HostTensor* get(const std::string& name, std::initializer_list<long> shape) {
        auto it = t.find(name);
        if (it == t.end()) { if (!rc) rc = fail(err, SI_EWEIGHTS, "checkpoint is missing tensor '%s'", name.c_str()); return nullptr; }
        std::vector<long> want(shape);
        if (it->second.shape != want) {
            std::ostringstream a, b;
            for (long v : it->second.shape) a << v << ' ';
            for (long v : want) b << v << ' ';
            if (!rc) rc = fail(err, SI_EWEIGHTS, "tensor '%s' has shape [%s] but the model needs [%s]", name.c_str(), a.str().c_str(), b.str().c_str());
            return nullptr;
        }
        if (!dry && !all_finite(name, it->second.data, it->second.n)) return nullptr;
        return &it->second;
    }
    bool has(const std::string& n) const { return t.count(n) != 0; }
    float* fptr(size_t off) { return reinterpret_cast<float*>(base() + off); }
    void copy_floats(size_t off, const std::string& name, long n) {
        const HostTensor* h = get(name, {n});
        if (h && !dry) memcpy(base() + off, h->data, (size_t)n * 4);
    }
    // Folded weight of a conv-like module (shape `shape`); norm_dim = the dim weight_norm keeps.  Dry pass: look-ups only, false.
    bool folded(const std::string& prefix, std::initializer_list<long> shape, int norm_dim, std::vector<float>& w) {
        std::vector<long> sh(shape);
        long n = 1; for (long v : sh) n *= v;
        if (has(prefix + ".weight")) {
            const HostTensor* h = get(prefix + ".weight", shape);
            if (!h || dry) return false;
            w.assign(h->data, h->data + n);
            return true;
        }
        std::string gn = prefix + ".weight_g", vn = prefix + ".weight_v";
        if (!has(gn)) { gn = prefix + ".parametrizations.weight.original0"; vn = prefix + ".parametrizations.weight.original1"; }
        if (!has(gn)) { if (!rc) rc = fail(err, SI_EWEIGHTS, "checkpoint has neither '%s.weight' nor a weight-norm pair", prefix.c_str()); return false; }
        const HostTensor* v = get(vn, shape);
        if (!v) return false;
        auto git = t.find(gn);
        const long keep = sh[norm_dim];
        if (git->second.numel() != keep) { if (!rc) rc = fail(err, SI_EWEIGHTS, "'%s' must hold %ld magnitudes", gn.c_str(), keep); return false; }
        if (dry) return false;
        if (!all_finite(gn, git->second.data, git->second.n)) return false;
        long inner = 1; for (size_t i = norm_dim + 1; i < sh.size(); ++i) inner *= sh[i];
        std::vector<double> ss(keep, 0.0);
        for (long i = 0; i < n; ++i) { const long kidx = (i / inner) % keep; ss[kidx] += (double)v->data[i] * v->data[i]; }
        for (long kidx = 0; kidx < keep; ++kidx)
            if ((float)std::sqrt(ss[kidx]) == 0.f) {
                if (!rc) rc = fail(err, SI_EWEIGHTS, "'%s': weight-norm row %ld has zero norm (g / ||v|| is undefined)", vn.c_str(), kidx);
                return false;
            }
        w.resize(n);
        for (long i = 0; i < n; ++i) {
            const long kidx = (i / inner) % keep;
            // same operation order as torch._weight_norm: v * (g / norm), all in fp32
            const float nrm = (float)std::sqrt(ss[kidx]);
            w[i] = v->data[i] * (git->second.data[kidx] / nrm);
        }
        return all_finite(prefix + " (folded weight)", w.data(), w.size());
    }
    // store element (g, tap, n, ci) of a tap-GEMM weight
    void put(const GemmW& G, int g, int tap, int n, int ci, float v) {
        const size_t idx = (((size_t)g * G.ntaps + tap) * G.Npad + n) * G.Cin + ci;
        if (G.math == SI_MATH_F32) { fptr(G.w)[idx] = v; return; }
        if (G.math == SI_MATH_F16) { reinterpret_cast<unsigned short*>(base() + G.w)[idx] = h_f2h(v); return; }
        const unsigned short hi = h_f2bf(v);
        reinterpret_cast<unsigned short*>(base() + G.w)[idx] = hi;
        if (G.math == SI_MATH_BF16X3) reinterpret_cast<unsigned short*>(base() + G.w_lo)[idx] = h_f2bf(v - h_bf2f(hi));
    }
    // Conv1d weight (Cout, Cin/groups, k) -> W[g][tap][n][ci]; cin_valid < G.Cin leaves zero padding
    void conv(const GemmW& G, const std::vector<float>& w, int cout_total, int cin_g, int k) {
        const int npg = cout_total / G.groups;
        for (int co = 0; co < cout_total; ++co)
            for (int ci = 0; ci < cin_g; ++ci)
                for (int tp = 0; tp < k; ++tp)
                    put(G, co / npg, tp, co % npg, ci, w[((size_t)co * cin_g + ci) * k + tp]);
    }
    void bias(const GemmW& G, const std::string& name, long n) { if (G.has_bias) copy_floats(G.bias, name, n); }
};

int parse_index(Err err, const char* index, const void* blob, size_t nbytes, std::map<std::string, HostTensor>& out) {
    std::istringstream in(index ? index : "");
    std::string line;
    int lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string name; long long off; int nd;
        if (!(ls >> name >> off >> nd) || nd < 0 || nd > 8) return fail(err, SI_EWEIGHTS, "index line %d is malformed: '%.200s'", lineno, line.c_str());
        HostTensor t;
        size_t n = 1;
        bool overflow = false;
        for (int i = 0; i < nd; ++i) {
            long v;
            if (!(ls >> v) || v < 0) return fail(err, SI_EWEIGHTS, "index line %d: bad dims of tensor '%.200s'", lineno, name.c_str());
            t.shape.push_back(v);
            if (__builtin_mul_overflow(n, (size_t)v, &n)) overflow = true;
        }
        size_t bytes = 0;
        if (overflow || __builtin_mul_overflow(n, (size_t)4, &bytes) || bytes > (size_t)1 << 62)
            return fail(err, SI_EWEIGHTS, "index line %d: the dims of tensor '%.200s' overflow", lineno, name.c_str());
        t.n = n;
        if (off < 0 || off % 4 || (size_t)off > nbytes || bytes > nbytes - (size_t)off)
            return fail(err, SI_EWEIGHTS, "tensor '%.200s' (offset %lld, %zu floats) does not fit the %zu-byte blob", name.c_str(), off, n, nbytes);
        t.data = reinterpret_cast<const float*>(static_cast<const char*>(blob) + off);
        if (out.count(name)) return fail(err, SI_EWEIGHTS, "index line %d: tensor '%.200s' is listed twice", lineno, name.c_str());
        out[name] = t;
    }
    if (out.empty()) return fail(err, SI_EWEIGHTS, "checkpoint index is empty");
    return SI_OK;
}

int pack_weights(const si_model_desc& d, const PackOpts& o, const Layout& L, Packer& P) {
    const std::string B = "base_model.";
    const int H = d.hidden_size;
    const bool wr = !P.dry;
    std::vector<float> w;
    // ---- feature extractor
    {
        const std::string p0 = B + "feature_extractor.conv_layers.0.";
        const HostTensor* h = P.get(p0 + "conv.weight", {d.conv_dim[0], 1, d.conv_kernel[0]});
        if (h && wr) memcpy(P.base() + L.conv0_w, h->data, (size_t)h->numel() * 4);
        if (d.conv_bias) P.copy_floats(L.conv0_bias, p0 + "conv.bias", d.conv_dim[0]);
        P.copy_floats(L.conv0_g, p0 + "layer_norm.weight", d.conv_dim[0]);
        P.copy_floats(L.conv0_b, p0 + "layer_norm.bias", d.conv_dim[0]);
    }
    for (int i = 1; i < d.num_conv; ++i) {
        const std::string p = B + "feature_extractor.conv_layers." + std::to_string(i) + ".";
        const ConvW& c = L.convs[i - 1];
        const HostTensor* h = P.get(p + "conv.weight", {d.conv_dim[i], d.conv_dim[i - 1], d.conv_kernel[i]});
        if (h && wr) { w.assign(h->data, h->data + h->numel()); P.conv(c.g, w, d.conv_dim[i], d.conv_dim[i - 1], d.conv_kernel[i]); }
        P.bias(c.g, p + "conv.bias", d.conv_dim[i]);
        if (d.feat_norm_layer) { P.copy_floats(c.ln_g, p + "layer_norm.weight", d.conv_dim[i]); P.copy_floats(c.ln_b, p + "layer_norm.bias", d.conv_dim[i]); }
    }
    const int CF = d.conv_dim[d.num_conv - 1];
    if (d.feat_proj_layer_norm) {
        P.copy_floats(L.fp_ln_g, B + "feature_projection.layer_norm.weight", CF);
        P.copy_floats(L.fp_ln_b, B + "feature_projection.layer_norm.bias", CF);
    }
    auto linear = [&](const GemmW& G, const std::string& name, int nout, int nin, int row0 = 0) {
        const HostTensor* h = P.get(name + ".weight", {nout, nin});
        if (h && wr) for (int o2 = 0; o2 < nout; ++o2) for (int i = 0; i < nin; ++i) P.put(G, 0, 0, row0 + o2, i, h->data[(size_t)o2 * nin + i]);
        const HostTensor* b = P.get(name + ".bias", {nout});
        if (b && wr) memcpy(P.fptr(G.bias) + row0, b->data, (size_t)nout * 4);
    };
    linear(L.proj, B + "feature_projection.projection", H, CF);
    {
        const int cg = H / d.pos_conv_groups;
        if (P.folded(B + "encoder.pos_conv_embed.conv", {H, cg, d.pos_conv_kernel}, 2, w)) P.conv(L.pos, w, H, cg, d.pos_conv_kernel);
        P.bias(L.pos, B + "encoder.pos_conv_embed.conv.bias", H);
    }
    P.copy_floats(L.enc_ln_g, B + "encoder.layer_norm.weight", H);
    P.copy_floats(L.enc_ln_b, B + "encoder.layer_norm.bias", H);
    for (int l = 0; l < d.num_layers; ++l) {
        const std::string p = B + "encoder.layers." + std::to_string(l) + ".";
        const LayerW& W = L.layers[l];
        linear(W.qkv, p + "attention.q_proj", H, H, 0);
        linear(W.qkv, p + "attention.k_proj", H, H, H);
        linear(W.qkv, p + "attention.v_proj", H, H, 2 * H);
        linear(W.out, p + "attention.out_proj", H, H);
        P.copy_floats(W.ln1_g, p + "layer_norm.weight", H); P.copy_floats(W.ln1_b, p + "layer_norm.bias", H);
        linear(W.ffn1, p + "feed_forward.intermediate_dense", d.intermediate_size, H);
        linear(W.ffn2, p + "feed_forward.output_dense", H, d.intermediate_size);
        P.copy_floats(W.ln2_g, p + "final_layer_norm.weight", H); P.copy_floats(W.ln2_b, p + "final_layer_norm.bias", H);
    }
    P.copy_floats(L.head_ln_g, "final_layers.0.weight", H);
    P.copy_floats(L.head_ln_b, "final_layers.0.bias", H);
    linear(L.head, "final_layers.1", d.codebook_dim, H);
    // ---- codebook tables (I_ea/loss_fn.py:10-14): centre = mean over K; centred; 1/max(||centred||, 1e-8)
    {
        const int K = d.num_clusters, D = d.codebook_dim;
        const HostTensor* c = P.get("codebook", {K, D});
        if (c && wr) {
            std::vector<float> center(D, 0.f);
            for (int j = 0; j < D; ++j) { float s = 0.f; for (int k = 0; k < K; ++k) s += c->data[(size_t)k * D + j]; center[j] = s / K; }
            float* cc = P.fptr(L.cb_centered); float* raw = P.fptr(L.cb_raw); float* rn = P.fptr(L.cb_rnorm);
            for (int k = 0; k < K; ++k) {
                double ss = 0;
                for (int j = 0; j < D; ++j) {
                    const float v = c->data[(size_t)k * D + j] - center[j];
                    cc[(size_t)k * D + j] = v;
                    raw[(size_t)k * D + j] = v + center[j];        // predict.py:184: all_embeds_t_c + center_
                    ss += (double)v * v;
                }
                rn[k] = 1.0f / fmaxf((float)std::sqrt(ss), 1e-8f);
            }
            // finite centroids can still overflow the fp32 column sum
            if (P.all_finite("codebook (centred table)", cc, (size_t)K * D) && P.all_finite("codebook (raw table)", raw, (size_t)K * D))
                P.all_finite("codebook (1 / norm table)", rn, (size_t)K);
        }
    }
    // ---- generator
    const std::string G = "generator.";
    const int C0 = d.up_initial_channel;
    if (P.folded(G + "conv_pre", {C0, d.num_mels, 7}, 0, w)) P.conv(L.pre, w, C0, d.num_mels, 7);
    P.bias(L.pre, G + "conv_pre.bias", C0);
    int c = C0;                                            // REAL channel counts here; the packed matrices have the padded strides
    for (int i = 0; i < d.num_ups; ++i) {
        const int u = d.up_rates[i], k = d.up_kernels[i], cout = c / 2, coutp = stage_channels(d, o, i);
        const GemmW& U = L.ups[i];
        // ConvTranspose1d weight (Cin, Cout, k), weight-norm over dim 0 (= Cin).  Phase p = j mod u, tap q = j / u.
        if (P.folded(G + "ups." + std::to_string(i), {c, cout, k}, 0, w))
            for (int ci = 0; ci < c; ++ci)
                for (int co = 0; co < cout; ++co)
                    for (int j = 0; j < k; ++j) P.put(U, 0, j / u, (j % u) * coutp + co, ci, w[((size_t)ci * cout + co) * k + j]);
        const HostTensor* b = P.get(G + "ups." + std::to_string(i) + ".bias", {cout});
        if (b && wr) for (int ph = 0; ph < u; ++ph) memcpy(P.fptr(U.bias) + (size_t)ph * coutp, b->data, (size_t)cout * 4);
        c = cout;
        for (int j = 0; j < d.num_rb; ++j) {
            const ResW& R = L.rbs[(size_t)i * d.num_rb + j];
            const std::string rp = G + "resblocks." + std::to_string(i * d.num_rb + j) + ".";
            for (int n = 0; n < d.num_dil; ++n) {
                if (d.resblock_type == 2) {                       // ResBlock2: `convs.<n>` (I_ea/hifi_gan/models.py:56-61)
                    const std::string a = rp + "convs." + std::to_string(n);
                    if (P.folded(a, {c, c, d.rb_kernels[j]}, 0, w)) P.conv(R.c1[n], w, c, c, d.rb_kernels[j]);
                    P.bias(R.c1[n], a + ".bias", c);
                    continue;
                }
                const std::string a = rp + "convs1." + std::to_string(n), bb = rp + "convs2." + std::to_string(n);
                if (P.folded(a, {c, c, d.rb_kernels[j]}, 0, w)) P.conv(R.c1[n], w, c, c, d.rb_kernels[j]);
                P.bias(R.c1[n], a + ".bias", c);
                if (P.folded(bb, {c, c, d.rb_kernels[j]}, 0, w)) P.conv(R.c2[n], w, c, c, d.rb_kernels[j]);
                P.bias(R.c2[n], bb + ".bias", c);
            }
        }
    }
    if (P.folded(G + "conv_post", {1, c, 7}, 0, w))
        for (int ci = 0; ci < c; ++ci) for (int k = 0; k < 7; ++k) P.fptr(L.post_w)[(size_t)k * L.post_C + ci] = w[(size_t)ci * 7 + k];
    P.copy_floats(L.post_b, G + "conv_post.bias", 1);
    return P.rc;
}

}  // namespace

int pack_image(const si_model_desc& d, const PackOpts& o, const Layout& L, const void* blob, size_t nbytes, const char* index,
               std::vector<char>& image, Err e) {
    try {
        image.clear();
        Packer P;
        P.err = e;
        int rc = parse_index(e, index, blob, nbytes, P.t);
        if (rc) return rc;
        P.dry = true;                                       // every required tensor present and of the right shape ...
        rc = pack_weights(d, o, L, P);
        if (rc) return rc;
        try {
            image.assign(L.total, 0);                       // ... before the image is allocated
        } catch (const std::bad_alloc&) {
            return fail(e, SI_ENOMEM, "cannot allocate the %zu-byte packed weight image on the host", L.total);
        }
        P.img = &image;
        P.dry = false;
        rc = pack_weights(d, o, L, P);
        if (rc) { std::vector<char>().swap(image); return rc; }
        const BlobHeader hd = blob_header(d, o, L);
        memcpy(image.data(), &hd, sizeof(hd));
        return SI_OK;
    } catch (const std::bad_alloc&) {
        std::vector<char>().swap(image);
        return fail(e, SI_ENOMEM, "out of host memory while packing the checkpoint");
    } catch (...) {
        std::vector<char>().swap(image);
        return fail(e, SI_EINVAL, "internal error while packing the checkpoint");
    }
}

}  // namespace siw

// ------------------------------------------------------------------------------------------------ C ABI (no device needed)
extern "C" {

int si_plan_weights(const si_model_desc* desc, size_t* total_bytes) {
    const siw::Err e{siw::g_create_err, sizeof(siw::g_create_err)};
    siw::g_create_err[0] = 0;
    if (!total_bytes) return siw::fail(e, SI_EINVAL, "si_plan_weights: total_bytes is NULL");
    *total_bytes = 0;
    try {
        if (int rc = siw::check_desc(desc, e)) return rc;
        siw::Layout L;
        siw::plan_layout(*desc, siw::pack_opts_from_env(), L);
        *total_bytes = L.total;
        return SI_OK;
    } catch (...) {
        return siw::fail(e, SI_ENOMEM, "si_plan_weights: out of host memory");
    }
}

int si_pack_weights_host(const si_model_desc* desc, const void* blob, size_t nbytes, const char* index, void* out, size_t capacity,
                         size_t* needed, char* err, size_t errcap) {
    const siw::Err e{err, errcap};
    if (err && errcap) err[0] = 0;
    if (needed) *needed = 0;
    try {
        if (int rc = siw::check_desc(desc, e)) return rc;
        if (!blob || !index) return siw::fail(e, SI_EINVAL, "si_pack_weights_host: NULL argument");
        const siw::PackOpts o = siw::pack_opts_from_env();
        siw::Layout L;
        siw::plan_layout(*desc, o, L);
        if (needed) *needed = L.total;
        if (!out || capacity < L.total)
            return siw::fail(e, SI_ENOMEM, "si_pack_weights_host: the packed image needs %zu bytes, the output buffer holds %zu", L.total, out ? capacity : (size_t)0);
        std::vector<char> image;
        if (int rc = siw::pack_image(*desc, o, L, blob, nbytes, index, image, e)) return rc;
        memcpy(out, image.data(), L.total);
        return SI_OK;
    } catch (...) {
        return siw::fail(e, SI_ENOMEM, "si_pack_weights_host: out of host memory");
    }
}

}  // extern "C"
