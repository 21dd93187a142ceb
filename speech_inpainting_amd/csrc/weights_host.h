// weights_host.h -- everything between a model desc and the packed weight image, as plain host C++ (no HIP header):
// the descriptor check, the layout plan, its fingerprint and header, and the checkpoint packer.  api.hip keeps the context
// and the device; it calls into this unit, and so do si_plan_weights / si_pack_weights_host, which need no device at all
// (tests/test_weights_host.py, tools/packcheck_main.cpp).
//
// Bounds of the descriptor (check_desc refuses anything outside, naming the field).  They are chosen so that no `int` or
// `size_t` expression of plan_layout, enc_dims, ups_geom or the workspace sizing can overflow, and they leave HuBERT-base /
// -large (H 768 / 1024, 12 / 24 layers, FFN 3072 / 4096, conv 512), HiFi-GAN V1 / V3 (512 / 256 channels, hop 256) and the unit
// vocoder (512 channels, 384 input channels, hop 320) a wide margin:
//   hidden_size        64 .. 4096, = 64 * num_heads              num_layers        1 .. 64
//   intermediate_size  16 .. 16384, multiple of 16               num_conv          2 .. SI_MAX_CONV
//   conv_dim[i]        16 .. 4096, multiple of 16                conv_kernel[i], conv_stride[i]   1 .. 1024
//   pos_conv_kernel    1 .. 1024                                 pos_conv_groups   >= 1, divides hidden_size into multiples of 16
//   layer_norm_eps     finite, > 0                               codebook_dim      1 .. 128
//   num_clusters       1 .. 65536                                num_mels          1 .. 4096
//   num_ups            1 .. SI_MAX_UPS                           up_rates[i]       1 .. 64, their product (the hop) <= 65536
//   up_kernels[i]      up_rates[i] .. 1024, even difference      up_initial_channel  32 .. 8192, a multiple of 32 at every stage's input
//   num_rb / num_dil   1 .. SI_MAX_RB / SI_MAX_DIL               rb_kernels[j]     odd, 1 .. 255
//   rb_dilations[j][n] 1 .. 4096                                 resblock_type     0 .. 2;  encoder_math / vocoder_math  0 .. 3
// The largest plan inside these bounds is below 2^37 bytes; every product that forms it is taken in size_t.
// The flags (conv_bias, feat_norm_layer, stable_layer_norm, feat_proj_layer_norm) are read as booleans and vocoder_chunk <= 0
// means the library default, so every value of those is legal.  Only the USED elements of the arrays are looked at.
// Inside those ranges check_desc also refuses the widths a dedicated kernel of the first forward would refuse (what is left to the
// first forward: a tap-GEMM tile past its prefetch registers or LDS -- strides, kernels or (k - 1) * dilation in the hundreds):
//   conv_kernel[0]     10 (the waveform conv)                    conv_dim[0]       a power of two, <= 1024 (4 * 2^j)
//   hidden_size, every LayerNormed conv_dim[i] (all of them in the layer flavour, the last one under feat_proj_layer_norm)  <= SI_LN_MAX_WIDTH
//   up_initial_channel >> num_ups (conv_post's input width)      <= 148: 262 rows of width + 4 floats and 7 width weights in SI_POST_MAX_LDS
// (num_mels needs no such rule: conv_pre's input rows are padded to a multiple of 32 channels, mel_ld.)
#ifndef SI_WEIGHTS_HOST_H
#define SI_WEIGHTS_HOST_H

#define SI_LN_MAX_WIDTH 2048            /* si_launch_layernorm: 8 registers x 256 lanes */
#define SI_POST_MAX_LDS (160 * 1024)    /* si_launch_conv_post: bytes of LDS a workgroup may have */

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/si_hip.h"

static inline int si_pick_bn(int N) { return N >= 128 ? 128 : (N > 32 ? 64 : 32); }
static inline int si_round_up(int a, int b) { return (a + b - 1) / b * b; }

namespace siw {

struct GemmW {              // one tap-GEMM weight inside the packed blob
    size_t w = 0, w_lo = 0, bias = 0;   // byte offsets (bias: 0 = none)
    int Cin = 0, N = 0, Npad = 0, ntaps = 0, groups = 1, math = 0;
    bool has_bias = false;
};

struct LayerW { GemmW qkv, out, ffn1, ffn2; size_t ln1_g, ln1_b, ln2_g, ln2_b; };
struct ConvW { GemmW g; size_t ln_g = 0, ln_b = 0; };
struct ResW { GemmW c1[SI_MAX_DIL], c2[SI_MAX_DIL]; };

struct Layout {
    size_t total = 0;
    // encoder
    size_t conv0_w, conv0_bias, conv0_g, conv0_b;
    std::vector<ConvW> convs;            // conv layers 1..n-1
    size_t fp_ln_g, fp_ln_b; GemmW proj;
    GemmW pos; size_t enc_ln_g, enc_ln_b;
    std::vector<LayerW> layers;
    size_t head_ln_g, head_ln_b; GemmW head;
    size_t cb_centered, cb_raw, cb_rnorm;
    // vocoder
    GemmW pre; std::vector<GemmW> ups; std::vector<ResW> rbs;   // rbs[stage*num_rb + j]
    size_t post_w, post_b; int post_C = 0;
    int mel_ld = 0;                      // padded mel channel count (conv_pre Cin)
};

// The two arithmetic-path options that move bytes of the packed image (stage_channels), read from the environment
// (SI_VOC_OPREADY, SI_VOC_RES16; both default to on) by si_create and by the host entries alike.
struct PackOpts { bool voc_opready = true, voc_res16 = true; };
bool env_flag(const char* name);         // unset: true; otherwise atoi(value) != 0
PackOpts pack_opts_from_env();

// Where an error message goes (a context's buffer, si_create's, or the caller's of the host entries); buf may be NULL.
struct Err { char* buf; size_t cap; };
int fail(Err e, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
extern char g_create_err[512];           // messages of the calls that have no context: si_create, si_plan_weights (si_last_error(NULL))

int check_desc(const si_model_desc* d, Err e);
int stage_channels(const si_model_desc& d, const PackOpts& o, int i);
int plan_layout(const si_model_desc& d, const PackOpts& o, Layout& L);

// The first 32 bytes of the blob (offset 0 is reserved).  `reserved` is not part of the layout check: the engine records there
// what the source rank's checkpoint held (speech_inpainting_amd/engine.py), the library writes 0 and never reads it.
struct BlobHeader { uint32_t magic, version; uint64_t fingerprint, total; uint64_t reserved; };
constexpr uint32_t BLOB_MAGIC = 0x42574953u;   // "SIWB"
uint64_t layout_fingerprint(const si_model_desc& d, const PackOpts& o, const Layout& L);
BlobHeader blob_header(const si_model_desc& d, const PackOpts& o, const Layout& L);

unsigned short h_f2bf(float f);
unsigned short h_f2h(float f);
float h_bf2f(unsigned short h);

// Checkpoint (fp32 blob + text index) -> the packed image of L.total bytes, header included: the bytes si_load_weights copies to
// the device.  Every required tensor is looked up and its shape checked BEFORE the image is allocated; a failed allocation is
// SI_ENOMEM; no C++ exception leaves this function.  On any failure `image` is left empty.
int pack_image(const si_model_desc& d, const PackOpts& o, const Layout& L, const void* blob, size_t nbytes, const char* index,
               std::vector<char>& image, Err e);

}  // namespace siw

#endif
