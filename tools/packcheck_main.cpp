// packcheck -- the descriptor check, the planner and the checkpoint packer (csrc/weights_host.cpp) as a stand-alone host program,
// built with -fsanitize=address,undefined by `make -C speech_inpainting_amd/csrc packcheck`.  It needs no device and nothing
// preloaded.  A tiny model pair in the four arithmetic modes: the good load in three checkpoint spellings, then every malformed
// index, every refused tensor and a table of refused descriptors.  One line per case; the last line is the summary.  Exit status
// 0 = every case answered as expected (a sanitizer report ends the program with its own status).
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "weights_host.h"

namespace {

struct Tensor { std::string name; std::vector<long> shape; std::vector<float> data; };
struct Ckpt {
    std::vector<Tensor> t;
    Tensor* find(const std::string& n) { for (auto& x : t) if (x.name == n) return &x; return nullptr; }
    void drop(const std::string& n) { for (size_t i = 0; i < t.size(); ++i) if (t[i].name == n) { t.erase(t.begin() + i); return; } }
};

uint32_t g_rng = 12345u;
float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return ((g_rng >> 8) / 16777216.0f - 0.5f) * 0.5f; }

si_model_desc tiny_desc(int em, int vm) {
    si_model_desc d;
    memset(&d, 0, sizeof(d));
    d.struct_size = (int32_t)sizeof(d);
    d.hidden_size = 128; d.num_layers = 1; d.num_heads = 2; d.intermediate_size = 128;
    d.num_conv = 3;
    const int ck[3] = {10, 3, 2}, cs[3] = {5, 2, 2};
    for (int i = 0; i < 3; ++i) { d.conv_dim[i] = 32; d.conv_kernel[i] = ck[i]; d.conv_stride[i] = cs[i]; }
    d.conv_bias = 1; d.feat_norm_layer = 1; d.stable_layer_norm = 0;
    d.pos_conv_kernel = 8; d.pos_conv_groups = 4; d.feat_proj_layer_norm = 1; d.layer_norm_eps = 1e-5f;
    d.codebook_dim = 80; d.num_clusters = 10;
    d.num_mels = 80; d.num_ups = 2;
    d.up_rates[0] = 5; d.up_kernels[0] = 11; d.up_rates[1] = 2; d.up_kernels[1] = 4;     // 11 taps at rate 5: absent (phase, tap) pairs
    d.up_initial_channel = 64;                                                             // 64 -> 32 -> 16: padded to 32 on the fp16 stream
    d.num_rb = 2; d.rb_kernels[0] = 3; d.rb_kernels[1] = 5; d.num_dil = 2;
    for (int j = 0; j < 2; ++j) { d.rb_dilations[j][0] = 1; d.rb_dilations[j][1] = 3; }
    d.encoder_math = em; d.vocoder_math = vm; d.vocoder_chunk = 0; d.resblock_type = 1;
    return d;
}

// spelling: 0 = weight_g / weight_v, 1 = parametrizations.weight.original0 / 1, 2 = folded `.weight` (values as they come)
Ckpt make_ckpt(const si_model_desc& d, int spelling) {
    Ckpt c;
    g_rng = 12345u;
    auto T = [&](const std::string& n, std::vector<long> sh) {
        Tensor t; t.name = n; t.shape = sh;
        long k = 1; for (long v : sh) k *= v;
        t.data.resize(k); for (float& v : t.data) v = rnd();
        c.t.push_back(t);
    };
    auto M = [&](const std::string& p, std::vector<long> sh, int keep) {
        if (spelling == 2) { T(p + ".weight", sh); return; }
        std::vector<long> g(sh.size(), 1); g[keep] = sh[keep];
        T(p + (spelling ? ".parametrizations.weight.original0" : ".weight_g"), g);
        T(p + (spelling ? ".parametrizations.weight.original1" : ".weight_v"), sh);
    };
    const std::string B = "base_model.", G = "generator.";
    const long H = d.hidden_size;
    for (int i = 0; i < d.num_conv; ++i) {
        const std::string p = B + "feature_extractor.conv_layers." + std::to_string(i) + ".";
        T(p + "conv.weight", {d.conv_dim[i], i ? d.conv_dim[i - 1] : 1, d.conv_kernel[i]});
        if (d.conv_bias) T(p + "conv.bias", {d.conv_dim[i]});
        if (i == 0 || d.feat_norm_layer) { T(p + "layer_norm.weight", {d.conv_dim[i]}); T(p + "layer_norm.bias", {d.conv_dim[i]}); }
    }
    const long CF = d.conv_dim[d.num_conv - 1];
    T(B + "feature_projection.layer_norm.weight", {CF}); T(B + "feature_projection.layer_norm.bias", {CF});
    auto lin = [&](const std::string& n, long o, long i) { T(n + ".weight", {o, i}); T(n + ".bias", {o}); };
    lin(B + "feature_projection.projection", H, CF);
    M(B + "encoder.pos_conv_embed.conv", {H, H / d.pos_conv_groups, d.pos_conv_kernel}, 2);
    T(B + "encoder.pos_conv_embed.conv.bias", {H});
    T(B + "encoder.layer_norm.weight", {H}); T(B + "encoder.layer_norm.bias", {H});
    for (int l = 0; l < d.num_layers; ++l) {
        const std::string p = B + "encoder.layers." + std::to_string(l) + ".";
        for (const char* nm : {"q_proj", "k_proj", "v_proj", "out_proj"}) lin(p + "attention." + nm, H, H);
        T(p + "layer_norm.weight", {H}); T(p + "layer_norm.bias", {H});
        lin(p + "feed_forward.intermediate_dense", d.intermediate_size, H);
        lin(p + "feed_forward.output_dense", H, d.intermediate_size);
        T(p + "final_layer_norm.weight", {H}); T(p + "final_layer_norm.bias", {H});
    }
    T("final_layers.0.weight", {H}); T("final_layers.0.bias", {H});
    lin("final_layers.1", d.codebook_dim, H);
    T("codebook", {d.num_clusters, d.codebook_dim});
    long ch = d.up_initial_channel;
    M(G + "conv_pre", {ch, d.num_mels, 7}, 0); T(G + "conv_pre.bias", {ch});
    for (int i = 0; i < d.num_ups; ++i) {
        M(G + "ups." + std::to_string(i), {ch, ch / 2, d.up_kernels[i]}, 0); T(G + "ups." + std::to_string(i) + ".bias", {ch / 2});
        ch /= 2;
        for (int j = 0; j < d.num_rb; ++j)
            for (int n = 0; n < d.num_dil; ++n)
                for (const char* fam : {"convs1.", "convs2."}) {
                    const std::string a = G + "resblocks." + std::to_string(i * d.num_rb + j) + "." + fam + std::to_string(n);
                    M(a, {ch, ch, d.rb_kernels[j]}, 0); T(a + ".bias", {ch});
                }
    }
    M(G + "conv_post", {1, ch, 7}, 0); T(G + "conv_post.bias", {1});
    return c;
}

void flatten(const Ckpt& c, std::vector<float>& blob, std::string& index) {
    blob.clear(); index.clear();
    for (const Tensor& t : c.t) {
        index += t.name + " " + std::to_string(blob.size() * 4) + " " + std::to_string(t.shape.size());
        for (long v : t.shape) index += " " + std::to_string(v);
        index += "\n";
        blob.insert(blob.end(), t.data.begin(), t.data.end());
    }
}

int g_cases = 0, g_bad = 0;
void report(const std::string& what, int rc, int want, const char* msg, const char* must = nullptr) {
    const bool ok = rc == want && (!must || strstr(msg, must));
    ++g_cases; if (!ok) ++g_bad;
    printf("%-4s %-58s rc=%d %s\n", ok ? "ok" : "BAD", what.c_str(), rc, msg);
}

int pack(const si_model_desc& d, const std::vector<float>& blob, const std::string& index, std::vector<unsigned char>& out, char* err) {
    size_t total = 0, need = 0;
    if (int rc = si_plan_weights(&d, &total)) { snprintf(err, 512, "%s", siw::g_create_err); return rc; }
    out.assign(total + 64, 0xA5);
    const int rc = si_pack_weights_host(&d, blob.data(), blob.size() * 4, index.c_str(), out.data(), total, &need, err, 512);
    for (size_t i = total; i < out.size(); ++i) if (out[i] != 0xA5) { snprintf(err, 512, "wrote past `needed`"); return -99; }
    if (rc) for (size_t i = 0; i < total; ++i) if (out[i] != 0xA5) { snprintf(err, 512, "a refused load wrote into the output"); return -99; }
    return rc;
}

}  // namespace

int main() {
    char err[512];
    std::vector<unsigned char> out, first;
    std::vector<float> blob;
    std::string index;
    const char* mname[4] = {"fp32", "bf16", "bf16x3", "fp16"};
    // ---- good loads: four modes, three spellings (the two weight-norm spellings must give equal bytes)
    for (int m = 0; m < 4; ++m) {
        const si_model_desc d = tiny_desc(m == 3 ? 1 : m & 1, m);
        for (int sp = 0; sp < 3; ++sp) {
            flatten(make_ckpt(d, sp), blob, index);
            err[0] = 0;
            int rc = pack(d, blob, index, out, err);
            if (sp == 0) first = out;
            if (rc == 0 && sp == 1 && out != first) { rc = -98; snprintf(err, 512, "the two weight-norm spellings gave different bytes"); }
            report(std::string("good load, vocoder ") + mname[m] + ", spelling " + std::to_string(sp), rc, SI_OK, err);
        }
    }
    // ---- malformed indexes and refused tensors (fp16 vocoder: the padded last stage)
    const si_model_desc d = tiny_desc(1, 3);
    const Ckpt good = make_ckpt(d, 0);
    flatten(good, blob, index);
    const std::string nb = std::to_string(blob.size() * 4);
    const std::pair<const char*, std::string> lines[] = {
        {"empty index", ""}, {"blank lines only", "\n\n"}, {"malformed line", index + "foo bar\n"}, {"nd > 8", index + "x 0 9 1 1 1 1 1 1 1 1 1\n"},
        {"nd < 0", index + "x 0 -1\n"}, {"negative dim", index + "x 0 2 4 -3\n"}, {"missing dim", index + "x 0 2 4\n"},
        {"dims overflow a signed count", index + "x 0 2 3037000500 3037000500\n"}, {"dims overflow size_t", index + "x 0 3 4294967296 4294967296 4\n"},
        {"byte count overflows", index + "x 0 2 2147483648 2147483648\n"}, {"offset negative", index + "x -4 1 1\n"},
        {"offset misaligned", index + "x 2 1 1\n"}, {"offset past the blob", index + "x " + nb + " 1 1\n"},
        {"offset near 2^63", index + "x 9223372036854775804 1 1\n"}, {"duplicate name", index + "codebook 0 2 10 80\n"},
        {"very long line", index + std::string(5000, 'y') + " zz\n"}};
    for (const auto& l : lines) { err[0] = 0; report(l.first, pack(d, blob, l.second, out, err), SI_EWEIGHTS, err); }
    for (const Tensor& t : good.t) {                                // each tensor missing, each tensor mis-shaped, each tensor with a NaN
        Ckpt c = good; c.drop(t.name); flatten(c, blob, index);
        err[0] = 0; report("missing " + t.name, pack(d, blob, index, out, err), SI_EWEIGHTS, err);
        c = good; c.find(t.name)->shape.push_back(1); flatten(c, blob, index);
        const bool mag = t.name.size() > 9 && t.name.compare(t.name.size() - 9, 9, ".weight_g") == 0;   // magnitudes: only their count matters
        err[0] = 0; report("extra dim of 1 on " + t.name, pack(d, blob, index, out, err), mag ? SI_OK : SI_EWEIGHTS, err, mag ? nullptr : t.name.c_str());
        c = good; c.find(t.name)->data[t.data.size() / 2] = NAN; flatten(c, blob, index);
        err[0] = 0; report("NaN in " + t.name, pack(d, blob, index, out, err), SI_EWEIGHTS, err, "non-finite");
    }
    {
        Ckpt c = good; Tensor* v = c.find("generator.ups.0.weight_v");
        const long row = v->shape[1] * v->shape[2];
        for (long i = 0; i < row; ++i) v->data[3 * row + i] = 0.f;
        flatten(c, blob, index); err[0] = 0; report("zero-norm weight-norm row", pack(d, blob, index, out, err), SI_EWEIGHTS, err, "zero norm");
        c = good; c.find("generator.conv_pre.weight_g")->data.push_back(1.f); c.find("generator.conv_pre.weight_g")->shape = {65};
        flatten(c, blob, index); err[0] = 0; report("weight_g with the wrong count", pack(d, blob, index, out, err), SI_EWEIGHTS, err, "magnitudes");
        c = good; c.find("generator.conv_pre.weight_g")->data[0] = INFINITY;
        flatten(c, blob, index); err[0] = 0; report("inf magnitude", pack(d, blob, index, out, err), SI_EWEIGHTS, err, "non-finite");
        c = make_ckpt(d, 2); c.find("generator.conv_pre.weight")->data[5] = 1e6f;
        flatten(c, blob, index); err[0] = 0; report("finite weight beyond the fp16 range (clamped)", pack(d, blob, index, out, err), SI_OK, err);
    }
    // ---- refused descriptors: every integer field and every used array element at 0, -1, minus its alignment and INT_MAX
    flatten(good, blob, index);
    struct Field { const char* name; std::function<int32_t*(si_model_desc&)> at; int align; bool zero_ok; };
    std::vector<Field> fields = {
        {"struct_size", [](si_model_desc& x) { return &x.struct_size; }, 1, false}, {"hidden_size", [](si_model_desc& x) { return &x.hidden_size; }, 64, false},
        {"num_layers", [](si_model_desc& x) { return &x.num_layers; }, 1, false}, {"num_heads", [](si_model_desc& x) { return &x.num_heads; }, 1, false},
        {"intermediate_size", [](si_model_desc& x) { return &x.intermediate_size; }, 16, false}, {"num_conv", [](si_model_desc& x) { return &x.num_conv; }, 1, false},
        {"pos_conv_kernel", [](si_model_desc& x) { return &x.pos_conv_kernel; }, 1, false}, {"pos_conv_groups", [](si_model_desc& x) { return &x.pos_conv_groups; }, 1, false},
        {"codebook_dim", [](si_model_desc& x) { return &x.codebook_dim; }, 1, false}, {"num_clusters", [](si_model_desc& x) { return &x.num_clusters; }, 1, false},
        {"num_mels", [](si_model_desc& x) { return &x.num_mels; }, 1, false}, {"num_ups", [](si_model_desc& x) { return &x.num_ups; }, 1, false},
        {"up_initial_channel", [](si_model_desc& x) { return &x.up_initial_channel; }, 32, false}, {"num_rb", [](si_model_desc& x) { return &x.num_rb; }, 1, false},
        {"num_dil", [](si_model_desc& x) { return &x.num_dil; }, 1, false}, {"encoder_math", [](si_model_desc& x) { return &x.encoder_math; }, 1, true},
        {"vocoder_math", [](si_model_desc& x) { return &x.vocoder_math; }, 1, true}, {"resblock_type", [](si_model_desc& x) { return &x.resblock_type; }, 1, true}};
    for (int i = 0; i < d.num_conv; ++i) {
        fields.push_back({"conv_dim[i]", [i](si_model_desc& x) { return &x.conv_dim[i]; }, 16, false});
        fields.push_back({"conv_kernel[i]", [i](si_model_desc& x) { return &x.conv_kernel[i]; }, 1, false});
        fields.push_back({"conv_stride[i]", [i](si_model_desc& x) { return &x.conv_stride[i]; }, 1, false});
    }
    for (int i = 0; i < d.num_ups; ++i) {
        fields.push_back({"up_rates[i]", [i](si_model_desc& x) { return &x.up_rates[i]; }, 1, false});
        fields.push_back({"up_kernels[i]", [i](si_model_desc& x) { return &x.up_kernels[i]; }, 1, false});
    }
    for (int j = 0; j < d.num_rb; ++j) {
        fields.push_back({"rb_kernels[j]", [j](si_model_desc& x) { return &x.rb_kernels[j]; }, 1, false});
        for (int n = 0; n < d.num_dil; ++n) fields.push_back({"rb_dilations[j][n]", [j, n](si_model_desc& x) { return &x.rb_dilations[j][n]; }, 1, false});
    }
    for (const Field& f : fields)
        for (int v : {0, -1, -f.align, INT_MAX}) {
            if ((v == 0 && f.zero_ok) || (v == -f.align && f.align == 1)) continue;
            si_model_desc x = d; *f.at(x) = v;
            err[0] = 0;
            const int rc = pack(x, blob, index, out, err);
            const std::string stem(f.name, strcspn(f.name, "["));
            report(std::string("desc ") + f.name + " = " + std::to_string(v), rc, SI_EINVAL, err, stem.c_str());
        }
    for (float e : {NAN, INFINITY, -1.f, 0.f}) {
        si_model_desc x = d; x.layer_norm_eps = e;
        err[0] = 0; report("desc layer_norm_eps = " + std::to_string(e), pack(x, blob, index, out, err), SI_EINVAL, err, "layer_norm_eps");
    }
    {
        si_model_desc x = d; x.up_rates[1] = 0; x.up_kernels[1] = 0;      // once a division by zero in the planner
        err[0] = 0; report("desc up_rates[1] = up_kernels[1] = 0", pack(x, blob, index, out, err), SI_EINVAL, err, "up_rates");
        x = d; x.up_rates[1] = -2; x.up_kernels[1] = 0;
        err[0] = 0; report("desc up_rates[1] = -2, up_kernels[1] = 0", pack(x, blob, index, out, err), SI_EINVAL, err, "up_rates");
    }
    printf("packcheck: %d cases, %d answered as expected, %d not\n", g_cases, g_cases - g_bad, g_bad);
    return g_bad ? 1 : 0;
}
