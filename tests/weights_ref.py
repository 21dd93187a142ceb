"""The weight plan and the checkpoint packer restated in numpy, from DESIGN.md section 3 and the comments of csrc/weights_host.cpp.
Nothing here calls the library: tests/test_weights_host.py compares the library's packed image with this one byte for byte, and
tests/test_weights_ref.py shows that this restatement is right (float64, torch's casts, the oracle's tables) and sensitive (each
planted mistake of BUGS changes bytes).

The plan: a cursor that hands out 256-byte aligned regions; offset 0 (the first 256 bytes) is reserved and holds the 32-byte header
{u32 magic "SIWB", u32 version, u64 fingerprint, u64 total, u64 reserved}.  A tap-GEMM weight is W[g][tap][n][ci] (ci contiguous)
with n padded to Npad = round_up(N, pick_bn(N)), pick_bn = 128 for N >= 128, 64 for N > 32, else 32; it takes its matrix, then (bf16x3)
the lo plane, then (if it has one) its bias of groups * N floats.  Order: conv0 (weight, [bias], norm weight, norm bias); conv layers
1.. (gemm, [norm pair]); projection norm pair, projection; positional conv; encoder norm pair; per layer qkv (q | k | v at rows 0, H, 2H),
out, norm pair, ffn1, ffn2, norm pair; head norm pair, head (always fp32); centred / raw / 1-over-norm codebook tables; conv_pre
(Cin = round_up(num_mels, 32)); per stage the upsampler (ntaps = ceil(k / u), N = u * width) and its resblock convs; conv_post as
[7][width] floats and its bias.
"""
import numpy as np

F32, BF16, BF16X3, F16 = 0, 1, 2, 3
MAGIC, VERSION = 0x42574953, 3
BUGS = ("tap_ci", "div_mod", "pos_dim0", "qkv_order", "lo_from_bf16", "pad_rows", "bias_once", "raw_is_c")


# ---------------------------------------------------------------------------------------------------------------- casts
def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest, ties to even; NaN stays NaN (quiet bit set)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_val(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_split_bits(x, bug=()):
    """(hi, lo) planes of bf16x3: hi = bf16(v), lo = bf16(v - hi) with the subtraction in fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_bits(x)
    if "lo_from_bf16" in bug:                                   # planted: lo = bf16(v) - hi
        return hi, bf16_bits(bf16_val(bf16_bits(x)) - bf16_val(hi))
    return hi, bf16_bits(x - bf16_val(hi))


def f16_bits(x):
    """fp32 -> fp16 bits, round to nearest even, saturating at +-65504 (NaN stays NaN)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(x > 65504.0, np.float32(65504.0), np.where(x < -65504.0, np.float32(-65504.0), x)).astype(np.float32)
        h = c.astype(np.float16).view(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7E00), h).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------- fold, tables
def fold(v, g, norm_dim, g_dim=None):
    """v * (g / nrm) in fp32, nrm = the correctly rounded fp32 square root of the float64 sum of squares over every dim but norm_dim.
    g_dim (planted mistakes only): the dim the magnitudes g belong to, when it is not norm_dim."""
    v = np.asarray(v, dtype=np.float32)
    axes = tuple(a for a in range(v.ndim) if a != norm_dim)
    ss = (v.astype(np.float64) ** 2).sum(axis=axes, keepdims=True)
    nrm = np.sqrt(ss).astype(np.float32)
    gshape = [1] * v.ndim
    gshape[norm_dim if g_dim is None else g_dim] = -1
    gg = np.asarray(g, dtype=np.float32).reshape(gshape)
    return (v * (gg / nrm)).astype(np.float32)


def codebook_tables(c, bug=()):
    """(centred, raw, 1 / norm): centre = (sequential fp32 sum over K) / K; v = c - centre; raw = v + centre;
    1 / max(float(sqrt(double sum of v^2)), 1e-8f)."""
    c = np.asarray(c, dtype=np.float32)
    K = c.shape[0]
    s = np.zeros(c.shape[1], dtype=np.float32)
    for k in range(K):
        s = (s + c[k]).astype(np.float32)
    centre = (s / np.float32(K)).astype(np.float32)
    v = (c - centre).astype(np.float32)
    raw = c.copy() if "raw_is_c" in bug else (v + centre).astype(np.float32)
    nrm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    rn = (np.float32(1.0) / np.maximum(nrm, np.float32(1e-8))).astype(np.float32)
    return v, raw, rn, centre


# ---------------------------------------------------------------------------------------------------------------- plan
def pick_bn(N):
    return 128 if N >= 128 else (64 if N > 32 else 32)


def round_up(a, b):
    return (a + b - 1) // b * b


class Gemm:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Planner:
    def __init__(self):
        self.cur = 0

    def take(self, nbytes):
        o = self.cur
        self.cur += (nbytes + 255) // 256 * 256
        return o

    def floats(self, n):
        return self.take(4 * n)

    def gemm(self, math, groups, ntaps, N, Cin, bias):
        g = Gemm(math=math, groups=groups, ntaps=ntaps, N=N, Cin=Cin, has_bias=bias, Npad=round_up(N, pick_bn(N)), w_lo=0, bias=0)
        n = groups * ntaps * g.Npad * Cin
        g.w = self.take(n * (4 if math == F32 else 2))
        if math == BF16X3:
            g.w_lo = self.take(n * 2)
        if bias:
            g.bias = self.floats(groups * N)
        return g


def stage_channels(d, i, opready=True, res16=True):
    """Width of stage i as the kernels carry it: on the fp16 stream (both options on) a width in [4, 32) is padded to 32."""
    real = d.up_initial_channel >> (i + 1)
    return 32 if (opready and res16 and d.vocoder_math == F16 and 4 <= real < 32) else real


def plan(d, opready=True, res16=True):
    """-> a namespace of regions (byte offsets / Gemm records) and .total."""
    P, L = _Planner(), Gemm()
    P.take(256)
    em, vm, H = d.encoder_math, d.vocoder_math, d.hidden_size
    L.conv0_w = P.floats(d.conv_dim[0] * d.conv_kernel[0])
    L.conv0_bias = P.floats(d.conv_dim[0]) if d.conv_bias else 0
    L.conv0_g, L.conv0_b = P.floats(d.conv_dim[0]), P.floats(d.conv_dim[0])
    L.convs = []
    for i in range(1, d.num_conv):
        c = Gemm(g=P.gemm(em, 1, d.conv_kernel[i], d.conv_dim[i], d.conv_dim[i - 1], bool(d.conv_bias)), ln_g=0, ln_b=0)
        if d.feat_norm_layer:
            c.ln_g, c.ln_b = P.floats(d.conv_dim[i]), P.floats(d.conv_dim[i])
        L.convs.append(c)
    CF = d.conv_dim[d.num_conv - 1]
    L.fp_ln_g, L.fp_ln_b = P.floats(CF), P.floats(CF)
    L.proj = P.gemm(em, 1, 1, H, CF, True)
    cg = H // d.pos_conv_groups
    L.pos = P.gemm(em, d.pos_conv_groups, d.pos_conv_kernel, cg, cg, True)
    L.enc_ln_g, L.enc_ln_b = P.floats(H), P.floats(H)
    L.layers = []
    for _ in range(d.num_layers):
        w = Gemm()
        w.qkv, w.out = P.gemm(em, 1, 1, 3 * H, H, True), P.gemm(em, 1, 1, H, H, True)
        w.ln1_g, w.ln1_b = P.floats(H), P.floats(H)
        w.ffn1, w.ffn2 = P.gemm(em, 1, 1, d.intermediate_size, H, True), P.gemm(em, 1, 1, H, d.intermediate_size, True)
        w.ln2_g, w.ln2_b = P.floats(H), P.floats(H)
        L.layers.append(w)
    L.head_ln_g, L.head_ln_b = P.floats(H), P.floats(H)
    L.head = P.gemm(F32, 1, 1, d.codebook_dim, H, True)
    L.cb_centered = P.floats(d.num_clusters * d.codebook_dim)
    L.cb_raw = P.floats(d.num_clusters * d.codebook_dim)
    L.cb_rnorm = P.floats(d.num_clusters)
    L.mel_ld = round_up(d.num_mels, 32)
    c = d.up_initial_channel
    L.pre = P.gemm(vm, 1, 7, c, L.mel_ld, True)
    L.ups, L.rbs = [], []
    for i in range(d.num_ups):
        u, k, cout = d.up_rates[i], d.up_kernels[i], stage_channels(d, i, opready, res16)
        L.ups.append(P.gemm(vm, 1, (k + u - 1) // u, u * cout, c, True))
        c = cout
        for j in range(d.num_rb):
            r = Gemm(c1=[], c2=[])
            for _n in range(d.num_dil):
                r.c1.append(P.gemm(vm, 1, d.rb_kernels[j], c, c, True))
                if d.resblock_type != 2:
                    r.c2.append(P.gemm(vm, 1, d.rb_kernels[j], c, c, True))
            L.rbs.append(r)
    L.post_C = c
    L.post_w, L.post_b = P.floats(7 * c), P.floats(1)
    L.total = P.cur
    return L


# ---------------------------------------------------------------------------------------------------------------- required tensors
def required(d):
    """What a checkpoint must hold: ("tensor", name, shape) and ("module", prefix, shape, norm_dim) -- a module's weight comes as
    `.weight`, or as a weight-norm pair in either spelling; its bias is listed as a tensor of its own."""
    out, B, H = [], "base_model.", d.hidden_size
    T = lambda name, *shape: out.append(("tensor", name, tuple(shape)))
    M = lambda prefix, shape, nd: out.append(("module", prefix, tuple(shape), nd))
    p0 = B + "feature_extractor.conv_layers.0."
    T(p0 + "conv.weight", d.conv_dim[0], 1, d.conv_kernel[0])
    if d.conv_bias:
        T(p0 + "conv.bias", d.conv_dim[0])
    T(p0 + "layer_norm.weight", d.conv_dim[0]); T(p0 + "layer_norm.bias", d.conv_dim[0])
    for i in range(1, d.num_conv):
        p = B + f"feature_extractor.conv_layers.{i}."
        T(p + "conv.weight", d.conv_dim[i], d.conv_dim[i - 1], d.conv_kernel[i])
        if d.conv_bias:
            T(p + "conv.bias", d.conv_dim[i])
        if d.feat_norm_layer:
            T(p + "layer_norm.weight", d.conv_dim[i]); T(p + "layer_norm.bias", d.conv_dim[i])
    CF = d.conv_dim[d.num_conv - 1]
    if d.feat_proj_layer_norm:
        T(B + "feature_projection.layer_norm.weight", CF); T(B + "feature_projection.layer_norm.bias", CF)
    lin = lambda name, nout, nin: (T(name + ".weight", nout, nin), T(name + ".bias", nout))
    lin(B + "feature_projection.projection", H, CF)
    M(B + "encoder.pos_conv_embed.conv", (H, H // d.pos_conv_groups, d.pos_conv_kernel), 2)
    T(B + "encoder.pos_conv_embed.conv.bias", H)
    T(B + "encoder.layer_norm.weight", H); T(B + "encoder.layer_norm.bias", H)
    for l in range(d.num_layers):
        p = B + f"encoder.layers.{l}."
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "attention." + nm, H, H)
        T(p + "layer_norm.weight", H); T(p + "layer_norm.bias", H)
        lin(p + "feed_forward.intermediate_dense", d.intermediate_size, H)
        lin(p + "feed_forward.output_dense", H, d.intermediate_size)
        T(p + "final_layer_norm.weight", H); T(p + "final_layer_norm.bias", H)
    T("final_layers.0.weight", H); T("final_layers.0.bias", H)
    lin("final_layers.1", d.codebook_dim, H)
    T("codebook", d.num_clusters, d.codebook_dim)
    G, c = "generator.", d.up_initial_channel
    M(G + "conv_pre", (c, d.num_mels, 7), 0); T(G + "conv_pre.bias", c)
    for i in range(d.num_ups):
        M(G + f"ups.{i}", (c, c // 2, d.up_kernels[i]), 0); T(G + f"ups.{i}.bias", c // 2)
        c //= 2
        for j in range(d.num_rb):
            rp = G + f"resblocks.{i * d.num_rb + j}."
            for n in range(d.num_dil):
                for fam in (("convs",) if d.resblock_type == 2 else ("convs1", "convs2")):
                    M(rp + f"{fam}.{n}", (c, c, d.rb_kernels[j]), 0); T(rp + f"{fam}.{n}.bias", c)
    M(G + "conv_post", (1, c, 7), 0); T(G + "conv_post.bias", 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- packer
class _Image:
    def __init__(self, total, bug):
        self.b = np.zeros(total, dtype=np.uint8)
        self.bug = bug

    def f32(self, off, n):
        return self.b[off:off + 4 * n].view(np.float32)

    def put(self, G, W):
        """W: fp32 [groups][ntaps][Npad][Cin], zero where nothing is stored."""
        n = W.size
        if G.math == F32:
            self.f32(G.w, n)[:] = W.reshape(-1)
        elif G.math == F16:
            self.b[G.w:G.w + 2 * n].view(np.uint16)[:] = f16_bits(W.reshape(-1))
        else:
            hi, lo = bf16_split_bits(W.reshape(-1), self.bug)
            self.b[G.w:G.w + 2 * n].view(np.uint16)[:] = hi
            if G.math == BF16X3:
                self.b[G.w_lo:G.w_lo + 2 * n].view(np.uint16)[:] = lo

    def blank(self, G):
        W = np.zeros((G.groups, G.ntaps, G.Npad, G.Cin), dtype=np.float32)
        if "pad_rows" in self.bug and G.Npad > G.N:
            W[:, :, G.N:, :] = 1.0                                  # planted: padding rows left non-zero
        return W


def module_weight(sd, prefix, norm_dim, g_dim=None):
    """The folded fp32 weight of a module from a name -> numpy dict in any of the three spellings."""
    if prefix + ".weight" in sd:
        return np.asarray(sd[prefix + ".weight"], dtype=np.float32)
    gn, vn = prefix + ".weight_g", prefix + ".weight_v"
    if gn not in sd:
        gn, vn = prefix + ".parametrizations.weight.original0", prefix + ".parametrizations.weight.original1"
    return fold(sd[vn], sd[gn], norm_dim, g_dim)


def pack(d, sd, opready=True, res16=True, bug=()):
    """sd: name -> fp32 numpy array with the index's names ("base_model.*", "final_layers.*", "generator.*", "codebook").
    -> dict(image=bytes from offset 32 on (uint8), total, magic, version, layout)."""
    bug = tuple(bug)
    assert all(b in BUGS for b in bug)
    L = plan(d, opready, res16)
    I = _Image(L.total, bug)
    A = lambda name: np.asarray(sd[name], dtype=np.float32)
    B, H = "base_model.", d.hidden_size

    def floats(off, name):
        a = A(name).reshape(-1)
        I.f32(off, a.size)[:] = a

    def conv(G, w):
        """Conv1d weight (Cout, Cin / groups, k) -> W[g][tap][n][ci]."""
        cout, cin_g, k = w.shape
        W = I.blank(G)
        if "tap_ci" in bug:                                         # planted: tap and ci swapped -- the source read as (Cout, k, Cin)
            W[:, :k, :cout // G.groups, :cin_g] = w.reshape(G.groups, cout // G.groups, k, cin_g).transpose(0, 2, 1, 3)
        else:
            W[:, :k, :cout // G.groups, :cin_g] = w.reshape(G.groups, cout // G.groups, cin_g, k).transpose(0, 3, 1, 2)
        I.put(G, W)

    def bias(G, name):
        if G.has_bias:
            floats(G.bias, name)

    def linear(G, parts):
        """parts: (name, row0) stacked into ONE matrix; biases at the same rows."""
        W = I.blank(G)
        for name, row0 in parts:
            w = A(name + ".weight")
            W[0, 0, row0:row0 + w.shape[0], :w.shape[1]] = w
            I.f32(G.bias, G.N)[row0:row0 + w.shape[0]] = A(name + ".bias")
        I.put(G, W)

    p0 = B + "feature_extractor.conv_layers.0."
    floats(L.conv0_w, p0 + "conv.weight")
    if d.conv_bias:
        floats(L.conv0_bias, p0 + "conv.bias")
    floats(L.conv0_g, p0 + "layer_norm.weight"); floats(L.conv0_b, p0 + "layer_norm.bias")
    for i in range(1, d.num_conv):
        p, c = B + f"feature_extractor.conv_layers.{i}.", L.convs[i - 1]
        conv(c.g, A(p + "conv.weight"))
        bias(c.g, p + "conv.bias")
        if d.feat_norm_layer:
            floats(c.ln_g, p + "layer_norm.weight"); floats(c.ln_b, p + "layer_norm.bias")
    if d.feat_proj_layer_norm:
        floats(L.fp_ln_g, B + "feature_projection.layer_norm.weight"); floats(L.fp_ln_b, B + "feature_projection.layer_norm.bias")
    linear(L.proj, [(B + "feature_projection.projection", 0)])
    pos = B + "encoder.pos_conv_embed.conv"                        # planted: the norm over dim 0, as the generator's modules have it
    conv(L.pos, module_weight(sd, pos, 0, 2) if "pos_dim0" in bug else module_weight(sd, pos, 2))
    bias(L.pos, B + "encoder.pos_conv_embed.conv.bias")
    floats(L.enc_ln_g, B + "encoder.layer_norm.weight"); floats(L.enc_ln_b, B + "encoder.layer_norm.bias")
    for l in range(d.num_layers):
        p, W = B + f"encoder.layers.{l}.", L.layers[l]
        order = ("k_proj", "q_proj", "v_proj") if "qkv_order" in bug else ("q_proj", "k_proj", "v_proj")
        linear(W.qkv, [(p + "attention." + nm, r * H) for r, nm in enumerate(order)])
        linear(W.out, [(p + "attention.out_proj", 0)])
        floats(W.ln1_g, p + "layer_norm.weight"); floats(W.ln1_b, p + "layer_norm.bias")
        linear(W.ffn1, [(p + "feed_forward.intermediate_dense", 0)])
        linear(W.ffn2, [(p + "feed_forward.output_dense", 0)])
        floats(W.ln2_g, p + "final_layer_norm.weight"); floats(W.ln2_b, p + "final_layer_norm.bias")
    floats(L.head_ln_g, "final_layers.0.weight"); floats(L.head_ln_b, "final_layers.0.bias")
    linear(L.head, [("final_layers.1", 0)])
    cc, raw, rn, _ = codebook_tables(A("codebook"), bug)
    I.f32(L.cb_centered, cc.size)[:] = cc.reshape(-1)
    I.f32(L.cb_raw, raw.size)[:] = raw.reshape(-1)
    I.f32(L.cb_rnorm, rn.size)[:] = rn
    G = "generator."
    conv(L.pre, module_weight(sd, G + "conv_pre", 0))
    bias(L.pre, G + "conv_pre.bias")
    c = d.up_initial_channel
    for i in range(d.num_ups):
        u, k, cout, coutp, U = d.up_rates[i], d.up_kernels[i], c // 2, stage_channels(d, i, opready, res16), L.ups[i]
        w = module_weight(sd, G + f"ups.{i}", 0)                   # ConvTranspose1d weight (Cin, Cout, k)
        W = I.blank(U)
        if "pad_rows" in bug:
            W[:] = 0.0                                              # (keep this planted mistake to the plain convs: here absent pairs interleave)
        for j in range(k):
            tap, ph = (j % u, j // u) if "div_mod" in bug else (j // u, j % u)
            if tap < U.ntaps and ph * coutp + cout <= U.Npad:
                W[0, tap, ph * coutp:ph * coutp + cout, :c] = w[:, :, j].T
        I.put(U, W)
        b = A(G + f"ups.{i}.bias")
        for ph in range(1 if "bias_once" in bug else u):
            I.f32(U.bias, U.N)[ph * coutp:ph * coutp + cout] = b
        c = cout
        for j in range(d.num_rb):
            R, rp = L.rbs[i * d.num_rb + j], G + f"resblocks.{i * d.num_rb + j}."
            for n in range(d.num_dil):
                fams = (("convs", R.c1),) if d.resblock_type == 2 else (("convs1", R.c1), ("convs2", R.c2))
                for fam, gs in fams:
                    conv(gs[n], module_weight(sd, rp + f"{fam}.{n}", 0))
                    bias(gs[n], rp + f"{fam}.{n}.bias")
    w = module_weight(sd, G + "conv_post", 0)                      # (1, c, 7) -> [k][post_C]
    pw = I.f32(L.post_w, 7 * L.post_C).reshape(7, L.post_C)
    pw[:, :c] = w[0].T
    floats(L.post_b, G + "conv_post.bias")
    return dict(image=I.b[32:].copy(), total=L.total, magic=MAGIC, version=VERSION, layout=L)


def state_arrays(hubert_sd, gen_sd, codebook):
    """The three parts of a checkpoint as ONE name -> numpy dict with the names the index carries."""
    out = {k: np.ascontiguousarray(v.detach().float().numpy()) for k, v in hubert_sd.items()}
    out.update({"generator." + k: np.ascontiguousarray(v.detach().float().numpy()) for k, v in gen_sd.items()})
    out["codebook"] = np.ascontiguousarray(codebook.detach().float().numpy())
    return out


def flatten(sd):
    """name -> numpy dict -> the (blob, index) pair of si_load_weights."""
    lines, parts, off = [], [], 0
    for name, a in sd.items():
        a = np.asarray(a, dtype=np.float32)
        parts.append(a.reshape(-1))
        lines.append(" ".join([name, str(off * 4), str(a.ndim)] + [str(s) for s in a.shape]))
        off += a.size
    return np.concatenate(parts) if parts else np.zeros(0, np.float32), "\n".join(lines) + "\n"
