"""The shape rule of every launcher that sits between a model descriptor and a dedicated kernel, restated, with the cases that stand on
both sides of every term of every rule and `reaches(case)`: the kernel family each op of a case must run on by these rules alone.

A plain module: no fixture, no GPU.  tests/test_shape_rules_host.py holds the constants below to the ones in csrc/*.hip and the case
tables to the coverage claim (per term: a case at the limit, a case that breaks that term and no other); tests/test_gpu_shape_rules.py
runs the cases and holds the profiled family names to `reaches`.

Rules as the source states them (launcher: terms; a launcher that returns 1 hands the op to the tap-GEMM):
  si_launch_respair (+ _wide)   C in {32, 64, 128, 256}; k odd in 3..11; (k - 1) dil <= 50; biases
  si_launch_reschain            C = 32; 3 <= k <= RC_KMAX; (k - 1) / 2 dil_n <= RC_MARG for each pair; 2 (k - 1) / 2 (d0 + d1 + d2 + 3) <=
                                RC_R / 4; api.hip: ResBlock1, num_dil == 3
  si_launch_upsample_stream     api.hip: u == 2, k == 4; taps == UP_TAPS; N == Cin in {64, 128}
  gemmcu_tc_pick                ntaps == 2; N % 256 == 0; Cin % C_BK == 0          (N = u Cout)
  si_launch_lingemm / _gemmcu   N % LG_BN == 0; K % LG_BK == 0 (per tap: Cin % LG_BK); lda % 8; ldo % 4; an instantiation 256 wide: N % 256
  ln_fuse (api.hip)             H % 128 == 0; I % 64 == 0; no capture registered; post-LN; bf16 with SI_ENC_LINGEMM on;
                                (BT + 128) (I + 128) 2 < 2e9
  si_launch_posconv             Cg in {48, 64}; (ntaps Cg) % (32 PC_KC) == 0; pad <= 127; ntaps <= 128
  launch_math (tapgemm.hip)     the 256-row tile while (255 stride + (ntaps - 1) |dil| + 1) (BK / 4) <= cap: tests/cases._config
  check_desc (weights_host.cpp) conv_kernel[0] == 10; conv_dim[0] = 4 * 2^j <= 1024; LayerNorm widths <= 2048; conv_post's width <= 148"""
import collections

# ------------------------------------------------------------------------------------------------------------ constants restated
PAIR_HALO = 50                     # respair.hip RPN_HALO, respair_wide.hip RPW_HALO and the literal in si_launch_respair
PAIR_C = (32, 64, 128, 256)
PAIR_KMIN, PAIR_KMAX = 3, 11
RC_C, RC_R, RC_MARG, RC_KMAX = 32, 768, 32, 11
UP_TAPS = 2
UP_CIN = (64, 128)
TC_TAPS, TC_BN = 2, 256
C_BK = 64                          # gemmcu.hip
LG_BN, LG_BK = 128, 64             # lingemm.hip
LNFUSE_H, LNFUSE_I = 128, 64       # api.hip, ln_fuse
LNFUSE_BYTES = 2.0e9               # ... and its bound on (BT + 128) (I + 128) 2 bytes of FFN intermediate
PC_KC = 4                          # posconv.hip: k-steps of 32 per weight chunk
PC_CG = (48, 64)
PC_PAD_MAX, PC_TAPS_MAX = 127, 128
LN_MAX = 2048                      # si_launch_layernorm, SI_LN_MAX_WIDTH
CONV0_K, CONV0_CMAX = 10, 1024     # conv0_check
POST_CMAX = 148                    # conv_post_kernel: (262 (C + 4) + 7 C) floats in 160 KiB


# ------------------------------------------------------------------------------------------------------------ the rules, term by term
# A rule: an ordered dict  term -> f(shape) -> (holds, at the limit).  `shape` is a dict of the launcher's arguments.  "At the limit" has
# one meaning per kind of term: an inequality holds with equality; a set term holds (every member is an edge of the set); a modulus term
# `x % m == 0` holds with an ODD count x / m -- the smallest multiple is one, and no wider tile (2 m) divides x.
def _rule(*terms):
    return collections.OrderedDict(terms)


def _mod(x, m):
    return x % m == 0, x % m == 0 and (x // m) % 2 == 1


def _le(x, limit):
    return x <= limit, x == limit


def _ge(x, limit):
    return x >= limit, x == limit


def _in(x, members):
    return x in members, x in members


PAIR = _rule(
    ("C in {32, 64, 128, 256}", lambda s: _in(s["C"], PAIR_C)),
    ("k >= 3", lambda s: _ge(s["k"], PAIR_KMIN)),
    ("k <= 11", lambda s: _le(s["k"], PAIR_KMAX)),
    ("(k - 1) dil <= 50", lambda s: _le((s["k"] - 1) * s["d"], PAIR_HALO)),
)


def _chain_h(s):
    return (s["k"] - 1) // 2 * (sum(s["dils"]) + 3)


CHAIN = _rule(
    ("C == 32", lambda s: _in(s["C"], (RC_C,))),
    ("k >= 3", lambda s: _ge(s["k"], 3)),
    ("k <= RC_KMAX", lambda s: _le(s["k"], RC_KMAX)),
    ("num_dil == 3", lambda s: _in(len(s["dils"]), (3,))),
    ("(k - 1) / 2 dil <= RC_MARG", lambda s: _le(max((s["k"] - 1) // 2 * d for d in s["dils"][:3]), RC_MARG)),
    ("2 H <= RC_R / 4", lambda s: _le(2 * _chain_h(s), RC_R // 4) if len(s["dils"]) == 3 else (True, False)),     # (H is defined over three pairs)
)

STREAM = _rule(
    ("u == 2 (N == Cin)", lambda s: _in(s["u"], (2,))),
    ("k == 4 (taps == UP_TAPS)", lambda s: _in(s["k"], (4,))),
    ("Cin in {64, 128}", lambda s: _in(s["Cin"], UP_CIN)),
)

TC = _rule(
    ("ntaps == 2", lambda s: _in(-(-s["k"] // s["u"]), (TC_TAPS,))),
    ("N % 256 == 0", lambda s: _mod(s["u"] * s["Cin"] // 2, TC_BN)),
    ("Cin % C_BK == 0", lambda s: _mod(s["Cin"], C_BK)),
)

LINGEMM = _rule(
    ("N % LG_BN == 0", lambda s: _mod(s["N"], LG_BN)),                 # (an odd count of 128-column tiles: no 256-wide instantiation divides N)
    ("K % LG_BK == 0", lambda s: _mod(s["K"], LG_BK)),                 # (K = 64 is one k-step: fewer than a ring has stages)
    ("lda % 8 == 0", lambda s: _mod(s["lda"], 8)),
    ("ldo % 4 == 0", lambda s: _mod(s["ldo"], 4)),
)

# (api.hip's ln_fuse has three more terms that no case here turns: bf16 with SI_ENC_LINGEMM on -- reaches_encoder's `ded` --, a post-LN
#  encoder, and (BT + 128) (I + 128) 2 < 2e9 bytes, a workspace bound no test shape comes near; test_shape_rules_host.py reads them too)
LNFUSE = _rule(
    ("H % 128 == 0", lambda s: _mod(s["H"], LNFUSE_H)),
    ("I % 64 == 0", lambda s: _mod(s["I"], LNFUSE_I)),
    ("no capture", lambda s: _in(s["captures"], (False,))),
)

POSCONV = _rule(
    ("Cg in {48, 64}", lambda s: _in(s["Cg"], PC_CG)),
    ("(ntaps Cg) % 128 == 0", lambda s: _mod(s["k"] * s["Cg"], 32 * PC_KC)),
    ("pad <= 127", lambda s: _le(s["k"] // 2, PC_PAD_MAX)),
    ("ntaps <= 128", lambda s: _le(s["k"], PC_TAPS_MAX)),
)

RULES = {"respair": PAIR, "reschain": CHAIN, "upsample_stream": STREAM, "gemmcu_tc": TC, "lingemm": LINGEMM, "ln_fuse": LNFUSE, "posconv": POSCONV}


# Terms that no descriptor breaks on their own: intermediate_size is a multiple of 16 and SI_ENC_FFNPAD of 8, so lda % 8 and ldo % 4 always
# hold; pad = ntaps / 2, so pad <= 127 follows from ntaps <= 128.
NOT_BREAKABLE_ALONE = {("lingemm", "lda % 8 == 0"), ("lingemm", "ldo % 4 == 0"), ("posconv", "pad <= 127")}
# Terms whose limit no descriptor reaches: pad = ntaps / 2 <= 64 under ntaps <= 128, so pad = 127 never occurs (the largest, 64, runs in P64k128);
# every row stride the encoder forms is a multiple of 16, an even count of 8 and of 4.
LIMIT_NOT_REACHABLE = {("posconv", "pad <= 127"), ("lingemm", "lda % 8 == 0"), ("lingemm", "ldo % 4 == 0")}


def holds(rule, shape):
    return all(f(shape)[0] for f in RULES[rule].values())


def broken(rule, shape):
    """The terms of `rule` that `shape` breaks."""
    return [t for t, f in RULES[rule].items() if not f(shape)[0]]


def at_limit(rule, shape):
    """The terms of `rule` that `shape` satisfies at their last accepted value."""
    return [t for t, f in RULES[rule].items() if all(f(shape))]


# ------------------------------------------------------------------------------------------------------------ generator cases
# One-stage architectures (tests/cases._arch).  A case: name, group, C (the stage's channels), the upsampler (u, ku), the blocks
# (ks, dils: one tuple of dilations per block), the environment of the engine, and what else the test does with it.
Gen = collections.namedtuple("Gen", "name group C u ku ks dils env lens note")


def _gen(name, group, C, ks, dils, u=1, ku=3, env=None, lens=None, note=""):
    dils = tuple(dils) if isinstance(dils[0], tuple) else (tuple(dils),) * len(ks)
    return Gen(name, group, C, u, ku, tuple(ks), dils, dict(env or {}), lens, note)


NOCHAIN = {"SI_VOC_CHAIN": "0"}
UPS_LIN = (1, 2, 255, 256, 257)
ONE = ((3,), ((1,),))              # the cheapest block behind an upsampler under test

GEN_CASES = []
for _C in PAIR_C:                  # pairs inside the rule: (k, d) nobody has run, (3, 25) at the halo's limit
    GEN_CASES += [_gen(f"pairs C={_C} k=5", "pairs inside", _C, (5,), (2, 4, 6), env=NOCHAIN),
                  _gen(f"pairs C={_C} k=9", "pairs inside", _C, (9,), (1, 2, 6), env=NOCHAIN),
                  _gen(f"pairs C={_C} k=3 d=25", "pairs inside", _C, (3,), (1, 12, 25), env=NOCHAIN)]
for _C in (64, 128):               # one step past: every pair on the tap-GEMM
    GEN_CASES += [_gen(f"past C={_C} k=3 d=26", "pairs past", _C, (3,), (26,), env=NOCHAIN),
                  _gen(f"past C={_C} k=11 d=6", "pairs past", _C, (11,), (6,), env=NOCHAIN),
                  _gen(f"past C={_C} k=13", "pairs past", _C, (13,), (1, 2, 4), env=NOCHAIN),
                  _gen(f"past C={_C} k=1", "pairs past", _C, (1,), (1, 3, 5), env=NOCHAIN)]
GEN_CASES += [_gen("past C=48", "pairs past", 48, (3,), (1, 3, 5), env=NOCHAIN, note="a width between two instantiations")]
for _C in (64, 128):               # a block of both: the fused pairs and the two-launch pair hand the stream over through h16[4 + (n & 1)]
    GEN_CASES += [_gen(f"block C={_C} (1, 25, 26)", "block of both", _C, (3,), (1, 25, 26), env=NOCHAIN),
                  _gen(f"block C={_C} (26, 1, 25)", "block of both", _C, (3,), (26, 1, 25), env=NOCHAIN)]
GEN_CASES += [_gen(f"stage C={_C} (3, 13, 7)", "stage of both", _C, (3, 13, 7), (1, 3, 4), env=NOCHAIN) for _C in (64, 128)]
GEN_CASES += [
    _gen("chain k=3 (25, 25, 25)", "chain", 32, (3,), (25, 25, 25), note="equal"),
    _gen("chain k=7 (10, 10, 9)", "chain", 32, (7,), (10, 10, 9), lens=(575, 576, 577, 1153, 1, 2, 60), note="2H = 192, 576 stored rows"),
    _gen("chain k=11 (1, 6, 6)", "chain", 32, (11,), (1, 6, 6)),
    _gen("chain k=3 (32, 25, 25)", "chain", 32, (3,), (32, 25, 25)),
    _gen("chain refused k=7 (10, 10, 10)", "chain refused", 32, (7,), (10, 10, 10)),
    _gen("chain refused k=11 (1, 3, 7)", "chain refused", 32, (11,), (1, 3, 7)),
    _gen("chain refused k=3 (33, 1, 1)", "chain refused", 32, (3,), (33, 1, 1)),
    _gen("chain refused k=13", "chain refused", 32, (13,), (1, 1, 1)),
    _gen("chain refused k=1", "chain refused", 32, (1,), (1, 3, 5)),
    _gen("chain refused C=64", "chain refused", 64, (3,), (1, 3, 5)),
    _gen("chain refused num_dil=2", "chain refused", 32, (3,), (1, 3)),
    _gen("chain refused num_dil=4", "chain refused", 32, (3,), (1, 3, 5, 7)),
]
GEN_CASES += [
    _gen("ups stream u=2 k=4 Cin=64", "upsamplers", 32, *ONE, u=2, ku=4, lens=UPS_LIN),
    _gen("ups stream u=2 k=4 Cin=128", "upsamplers", 64, *ONE, u=2, ku=4, lens=UPS_LIN),
    _gen("ups u=4 k=8 Cin=64", "upsamplers", 32, *ONE, u=4, ku=8, lens=UPS_LIN, note="N = 128: neither the stream kernel (u) nor the TC kernel (N)"),
    _gen("ups u=2 k=2 Cin=128", "upsamplers", 64, *ONE, u=2, ku=2, lens=UPS_LIN, note="one tap"),
    _gen("ups u=2 k=6 Cin=128", "upsamplers", 64, *ONE, u=2, ku=6, lens=UPS_LIN, note="three taps"),
    _gen("ups u=3 k=5 Cin=128", "upsamplers", 64, *ONE, u=3, ku=5, lens=UPS_LIN, note="k no multiple of u"),
    _gen("ups u=3 k=7 Cin=128", "upsamplers", 64, *ONE, u=3, ku=7, lens=UPS_LIN, note="k no multiple of u, three taps"),
    _gen("ups u=2 k=4 Cin=32", "upsamplers", 16, *ONE, u=2, ku=4, lens=UPS_LIN, note="N == Cin, narrower than the stream kernel's"),
    _gen("ups u=2 k=4 Cin=256", "upsamplers", 128, *ONE, u=2, ku=4, lens=UPS_LIN, note="N == Cin = 256: the TC kernel's smallest"),
    _gen("ups TC u=8 k=16 Cin=64", "upsamplers", 32, *ONE, u=8, ku=16, lens=UPS_LIN, note="N = 256, Cin = 64: one column tile, one k-step per tap"),
    _gen("ups TC u=6 k=12 256->128", "upsamplers", 128, *ONE, u=6, ku=12, lens=UPS_LIN, note="N = 768: three column tiles"),
    _gen("ups TC u=3 k=5 512->256", "upsamplers", 256, *ONE, u=3, ku=5, lens=UPS_LIN, note="N = 768: three column tiles; k no multiple of u (u = 3, k = 6 does not load: odd difference)"),
    _gen("ups u=3 k=5 256->128", "upsamplers", 128, *ONE, u=3, ku=5, lens=UPS_LIN, note="N = 384: refused by N % 256 alone"),
    _gen("ups u=16 k=32 96->48", "upsamplers", 48, *ONE, u=16, ku=32, lens=(1, 2, 15, 16, 17), note="N = 768, Cin = 96: refused by Cin % 64 alone"),
    _gen("ups u=4 k=4 Cin=128", "upsamplers", 64, *ONE, u=4, ku=4, lens=UPS_LIN, note="N = 256, one tap: refused by ntaps alone"),
]
GEN = {c.name: c for c in GEN_CASES}
assert len(GEN) == len(GEN_CASES)


def gen_arch(case):
    from tests.cases import _arch
    return _arch(case.C, u=case.u, k=case.ku, resblock_kernel_sizes=case.ks, resblock_dilation_sizes=case.dils)


def _padded(C):
    return 32 if 4 <= C < 32 else C


def reaches_generator(varch, env=None):
    """{family: launches} of the fp16 stream's dedicated kernels for one chunk of `varch` by the rules above, with "tapgemm_f16" the
    count of tap-GEMM launches (conv_pre, the upsamplers and pairs no dedicated kernel covers: two launches per pair)."""
    env = env or {}
    chain_on = env.get("SI_VOC_CHAIN", "1") != "0"
    fuse = env.get("SI_VOC_FUSE", "1") != "0"
    tc_on = env.get("SI_VOC_UPSGEMM", "1") != "0"
    out = collections.Counter({"tapgemm_f16": 1})
    nk = len(varch.resblock_kernel_sizes)
    Cin = varch.upsample_initial_channel
    for i, (u, ku) in enumerate(zip(varch.upsample_rates, varch.upsample_kernel_sizes)):
        C = _padded(Cin // 2)
        s = dict(u=u, k=ku, Cin=Cin)
        if fuse and holds("upsample_stream", s):
            out[f"upsample_f16_c{Cin}"] += 1
        elif tc_on and holds("gemmcu_tc", s):
            out["gemmcu_f16"] += 1
        else:
            out["tapgemm_f16"] += 1
        for j, (k, dils) in enumerate(zip(varch.resblock_kernel_sizes, varch.resblock_dilation_sizes)):
            acc = "_acc" if j > 0 else ""
            if str(varch.resblock) == "2":
                out["tapgemm_f16"] += len(dils)
                continue
            # (a stage that feeds a TC upsampler stores its sum activated, which the chain kernel does not do: api.hip, whole.slope16)
            nxt = dict(u=varch.upsample_rates[i + 1], k=varch.upsample_kernel_sizes[i + 1], Cin=Cin // 2) if i + 1 < len(varch.upsample_rates) else None
            act_next = nxt is not None and tc_on and holds("gemmcu_tc", nxt) and not (fuse and holds("upsample_stream", nxt))
            if fuse and chain_on and not (act_next and j == nk - 1) and holds("reschain", dict(C=C, k=k, dils=dils)):
                out[f"reschain_f16_c32{acc}"] += 1
                continue
            for n, d in enumerate(dils):
                if fuse and holds("respair", dict(C=C, k=k, d=d)):
                    out[f"respair_f16_c{C}" + (acc if n == len(dils) - 1 else "")] += 1
                else:
                    out["tapgemm_f16"] += 2
        Cin //= 2
    return {k: v for k, v in out.items() if v}


def profiled_generator(prof):
    """A profile {kernel: launches} folded to reaches_generator's keys."""
    out = collections.Counter()
    for n, v in prof.items():
        if n.startswith("tapgemm_f16_"):
            out["tapgemm_f16"] += v
        elif n.startswith("gemmcu_f16_"):
            out["gemmcu_f16"] += v
        elif n.startswith(("respair_", "reschain_", "upsample_f16_")):
            out[n] += v
    return dict(out)


# ------------------------------------------------------------------------------------------------------------ encoder cases
Enc = collections.namedtuple("Enc", "name group kw note")


def _enc(name, group, note="", **kw):
    return Enc(name, group, kw, note)


def _heads(H):
    return dict(hidden_size=H, num_attention_heads=H // 64)


ENC_CASES = [
    _enc("E1", "widths", "K of one k-step", intermediate_size=16, num_conv_pos_embedding_groups=1, **_heads(64)),
    _enc("E1b", "widths", "FFN1 on lingemm at K = 64: one k-step, fewer than a ring has stages", intermediate_size=128, num_conv_pos_embedding_groups=1, **_heads(64)),
    _enc("E1c", "widths", "the projection at K = 64", conv_dim=(32,) * 6 + (64,), **_heads(128)),
    _enc("E2", "widths", "N % 128 != 0: every GEMM on the tap-GEMM", intermediate_size=768, num_conv_pos_embedding_groups=4, **_heads(192)),
    _enc("E3", "widths", "three 128-column tiles, QKV N = 1152", intermediate_size=1536, num_conv_pos_embedding_groups=8, **_heads(384)),
    _enc("E4a", "widths", "FFN2's K not covered: the tap-GEMM reads rows I + pad apart", intermediate_size=272, num_conv_pos_embedding_groups=4, **_heads(256)),
    _enc("E4b", "widths", "FFN1 on the tap-GEMM writes the padded rows, FFN2 on lingemm at 5 k-steps", intermediate_size=320, num_conv_pos_embedding_groups=4, **_heads(256)),
    _enc("E5", "widths", "LayerNorm's widest row", intermediate_size=64, num_conv_pos_embedding_groups=32, **_heads(2048)),
    _enc("E6", "conv stack", "seven widths", conv_dim=(64, 64, 128, 128, 256, 256, 512), **_heads(128)),
    _enc("E6b", "conv stack", "two convs", conv_dim=(64, 128), conv_kernel=(10, 3), conv_stride=(5, 2), **_heads(128)),
    _enc("E7", "conv stack", "layer flavour, LayerNorm lanes partly active", conv_dim=(16, 1040, 32, 32, 32, 32, 32), feat_extract_norm="layer", conv_bias=True,
         do_stable_layer_norm=True, **_heads(128)),
]
# positional conv: (H, groups, kernel) -> Cg = H / groups
PC_CASES = [
    _enc("P48k64", "posconv", "", num_conv_pos_embeddings=64, num_conv_pos_embedding_groups=4, **_heads(192)),
    _enc("P48k8", "posconv", "(ntaps Cg) = 384: the smallest multiple of 128 at Cg = 48", num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4, **_heads(192)),
    _enc("P64k2", "posconv", "(ntaps Cg) = 128", num_conv_pos_embeddings=2, num_conv_pos_embedding_groups=4, **_heads(256)),
    _enc("P64k128", "posconv", "ntaps = 128, pad = 64", num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=4, **_heads(256)),
    _enc("P48k4", "posconv past", "(ntaps Cg) = 192", num_conv_pos_embeddings=4, num_conv_pos_embedding_groups=4, **_heads(192)),
    _enc("P64k127", "posconv past", "odd: no row trimmed; 127 x 64 is no multiple of 128", num_conv_pos_embeddings=127, num_conv_pos_embedding_groups=4, **_heads(256)),
    _enc("P64k129", "posconv past", "ntaps > 128", num_conv_pos_embeddings=129, num_conv_pos_embedding_groups=4, **_heads(256)),
    _enc("P64k130", "posconv past", "ntaps > 128 alone", num_conv_pos_embeddings=130, num_conv_pos_embedding_groups=4, **_heads(256)),
    _enc("P32", "posconv past", "Cg = 32", num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=8, **_heads(256)),
    _enc("P80", "posconv past", "Cg = 80", num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, **_heads(320)),
]
ENC = {c.name: c for c in ENC_CASES + PC_CASES}
assert len(ENC) == len(ENC_CASES) + len(PC_CASES)


def enc_arch(case):
    from speech_inpainting_amd.arch import HubertArch
    kw = dict(num_hidden_layers=1, intermediate_size=256, conv_dim=(32,) * 7, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, codebook_dim=80)
    kw.update(case.kw)
    return HubertArch(**kw)


def enc_gemms(harch, ffn_pad=64):
    """The bf16 encoder's Linear layers as lingemm's shape dicts: name -> dict(N, K, lda, ldo)."""
    H, I, CF = harch.hidden_size, harch.intermediate_size, harch.conv_dim[-1]
    return {"projection": dict(N=H, K=CF, lda=CF, ldo=H), "QKV": dict(N=3 * H, K=H, lda=H, ldo=3 * H), "out-proj": dict(N=H, K=H, lda=H, ldo=H),
            "FFN1": dict(N=I, K=H, lda=H, ldo=I + ffn_pad), "FFN2": dict(N=H, K=I, lda=I + ffn_pad, ldo=H)}


def reaches_encoder(harch, captures=True, env=None):
    """{op: family prefix} of the bf16 encoder's GEMMs, the positional conv and the LayerNorm residuals by the rules above.  A GEMM that
    lingemm's rule covers runs on "gemmcu_bf16|lingemm_bf16" (which of the two is the cost rule's business: test_gpu_encoder_ops.py's
    _linear_kernel), the others on "tapgemm_bf16"."""
    env = env or {}
    out = {}
    ded = env.get("SI_ENC_LINGEMM", "1") != "0"
    proj16 = harch.feat_proj_layer_norm                                 # (without its LayerNorm the projection reads fp32 features: tap-GEMM)
    for name, s in enc_gemms(harch).items():
        ok = ded and holds("lingemm", s) and (name != "projection" or proj16)
        out[name] = "gemmcu_bf16|lingemm_bf16" if ok else "tapgemm_bf16"
    cg = harch.hidden_size // harch.num_conv_pos_embedding_groups
    pc = env.get("SI_ENC_POSCONV", "1") != "0" and holds("posconv", dict(Cg=cg, k=harch.num_conv_pos_embeddings))
    out["pos_conv"] = f"posconv_bf16_c{cg}" if pc else "tapgemm_bf16"
    fuse = (ded and env.get("SI_ENC_LNFUSE", "1") != "0" and not harch.do_stable_layer_norm
            and holds("ln_fuse", dict(H=harch.hidden_size, I=harch.intermediate_size, captures=captures)))
    out["ln_residual"] = "fused" if fuse else "written"
    return out


def reaches(case, **kw):
    """The kernel family each op of a case must take by the rules of this module."""
    if isinstance(case, Gen):
        return reaches_generator(gen_arch(case), case.env)
    return reaches_encoder(enc_arch(case), **kw)


# ------------------------------------------------------------------------------------------------------------ coverage: the shapes a case puts before a rule
def gen_shapes(case):
    """[(rule, shape dict)] of every launcher decision in a generator case (stage 0 only: a second stage repeats the blocks at 128)."""
    C = _padded(case.C)
    out = [("upsample_stream", dict(u=case.u, k=case.ku, Cin=2 * case.C)), ("gemmcu_tc", dict(u=case.u, k=case.ku, Cin=2 * case.C))]
    for k, dils in zip(case.ks, case.dils):
        out.append(("reschain", dict(C=C, k=k, dils=dils)))
        out += [("respair", dict(C=C, k=k, d=d)) for d in dils]
    return out


def enc_shapes(case, captures=False):
    harch = enc_arch(case)
    out = [("lingemm", dict(s, op=n)) for n, s in enc_gemms(harch).items()]
    out.append(("posconv", dict(Cg=harch.hidden_size // harch.num_conv_pos_embedding_groups, k=harch.num_conv_pos_embeddings)))
    if not harch.do_stable_layer_norm:
        out.append(("ln_fuse", dict(H=harch.hidden_size, I=harch.intermediate_size, captures=captures)))
    return out


def coverage():
    """{(rule, term): {"limit": [case names], "past": [case names]}}: `limit` holds the cases whose shape satisfies the whole rule with
    this term at its last accepted value, `past` those that break this term and no other of the rule."""
    cov = {(r, t): {"limit": [], "past": []} for r, rule in RULES.items() for t in rule}
    shapes = [(c.name, rs) for c in GEN_CASES for rs in gen_shapes(c)]
    shapes += [(c.name + (" tapped" if cap else ""), rs) for c in ENC_CASES + PC_CASES for cap in (False, True) for rs in enc_shapes(c, cap)]
    for name, (rule, shape) in shapes:
        if rule == "reschain" and "SI_VOC_CHAIN" in GEN[name].env:
            continue                                                    # (the chain is switched off there: the case says nothing about its rule)
        bad = broken(rule, shape)
        if not bad:
            for t in at_limit(rule, shape):
                cov[(rule, t)]["limit"].append(name)
        elif len(bad) == 1:
            cov[(rule, bad[0])]["past"].append(name)
    return cov
