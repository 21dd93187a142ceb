"""tests/shape_rules.py on the CPU: its constants are the ones the launchers in csrc/*.hip are written with (read out of the source, the way
test_poison_host.py reads the si_prof_begin calls), its case tables stand on both sides of every term of every rule, and the references
the GPU cases are held to still reject a seeded mistake at the new shapes (on a CPU emulation, as in test_vocoder_ref.py)."""
import os
import re

import torch

from tests import encoder_ref as E
from tests import shape_rules as S
from tests import vocoder_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_inpainting_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------ constants out of the source
def _one(text, pattern, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, f"{what}: {len(m)} matches of {pattern!r}"
    return m[0]


def source_constants(csrc=CSRC):
    """{name: value} of every constant of the rule table as csrc/* states it; a rule that is written differently no longer matches."""
    src = {f: open(os.path.join(csrc, f)).read() for f in ("respair.hip", "respair_wide.hip", "reschain.hip", "upsample.hip", "gemmcu.hip", "lingemm.hip",
                                                           "posconv.hip", "encoder_kernels.hip", "vocoder_kernels.hip", "api.hip", "weights_host.cpp", "weights_host.h")}
    c = {}
    rp = src["respair.hip"]
    c["RPN_HALO"] = int(_one(rp, r"constexpr int RPN_HALO = (\d+);", "respair.hip"))
    c["RPW_HALO"] = int(_one(src["respair_wide.hip"], r"constexpr int RPW_HALO = (\d+);", "respair_wide.hip"))
    rule = _one(rp, r"if \(\(C != (\d+) && C != (\d+) && C != (\d+) && C != (\d+)\) \|\| k < (\d+) \|\| k > (\d+) \|\| \(k & 1\) == 0 \|\| \(k - 1\) \* dil > (\d+) \|\|", "si_launch_respair")
    c["PAIR_C"] = tuple(int(v) for v in rule[:4])
    c["PAIR_KMIN"], c["PAIR_KMAX"], c["PAIR_HALO"] = int(rule[4]), int(rule[5]), int(rule[6])
    rc = src["reschain.hip"]
    nw, rt = int(_one(rc, r"[ ,]RC_NW = (\d+)[,;]", "RC_NW")), int(_one(rc, r"constexpr int RC_RT = (\d+)", "RC_RT"))
    _one(rc, r"constexpr int RC_R = RC_NW \* RC_RT \* 16;", "RC_R")
    c["RC_R"] = nw * rt * 16
    c["RC_C"] = int(_one(rc, r"constexpr int RC_C = (\d+)", "RC_C"))
    c["RC_MARG"] = int(_one(rc, r"constexpr int RC_MARG = (\d+);", "RC_MARG"))
    c["RC_KMAX"] = int(_one(rc, r"constexpr int RC_KMAX = (\d+);", "RC_KMAX"))
    _one(rc, r"if \(C != RC_C \|\| p\.k < 3 \|\| p\.k > RC_KMAX \|\| \(p\.k & 1\) == 0 \|\|", "si_launch_reschain: k")
    _one(rc, r"\(p\.k - 1\) / 2 \* p\.dil\[i\] > RC_MARG", "si_launch_reschain: margin")
    _one(rc, r"const int H = \(p\.k - 1\) / 2 \* \(p\.dil\[0\] \+ p\.dil\[1\] \+ p\.dil\[2\] \+ 3\);", "si_launch_reschain: H")
    c["RC_FRACTION"] = int(_one(rc, r"if \(2 \* H > RC_R / (\d+)\) return 1;", "si_launch_reschain: 2 H"))
    _one(src["api.hip"], r"ctx->opt_voc_chain && d\.num_dil == 3 &&", "api.hip: num_dil == 3")
    up = src["upsample.hip"]
    c["UP_TAPS"] = int(_one(up, r"constexpr int UP_TAPS = (\d+);", "UP_TAPS"))
    _one(up, r"if \(p\.taps != UP_TAPS \|\| p\.N != p\.Cin \|\|", "si_launch_upsample_stream")
    c["UP_CIN"] = tuple(sorted(int(v) for v in re.findall(r"if \(p\.Cin == (\d+)\) return upsample_launch<", up)))
    _one(src["api.hip"], r"d\.up_rates\[i\] == 2 && d\.up_kernels\[i\] == 4 &&", "api.hip: the stream kernel's (u, k)")
    gc = src["gemmcu.hip"]
    c["C_BK"] = int(_one(gc, r"constexpr int C_BK = (\d+),", "C_BK"))
    tc = _one(gc, r"p\.dil != -1 \|\| p\.ntaps != (\d+) \|\|", "gemmcu_tc_pick: taps")
    c["TC_TAPS"] = int(tc)
    c["TC_BN"] = int(_one(gc, r"if \(p\.Cin % C_BK \|\| p\.N % (\d+) \|\| p\.ldo % 8 \|\|", "gemmcu_tc_pick: N"))
    c["GEMMCU_N"] = int(_one(gc, r"p\.lda % 8 \|\| p\.M <= 0 \|\| p\.nseg <= 0 \|\| p\.N % (\d+)\) return 1;", "si_launch_gemmcu: N"))
    lg = src["lingemm.hip"]
    bn, bk = _one(lg, r"constexpr int LG_BN = (\d+), LG_BK = (\d+),", "LG_BN, LG_BK")
    c["LG_BN"], c["LG_BK"] = int(bn), int(bk)
    c["LG_LDO"], c["LG_LDA"] = (int(v) for v in _one(lg, r"if \(p\.N % LG_BN \|\| p\.Cin % LG_BK \|\| p\.K % LG_BK \|\| p\.K != p\.ntaps \* p\.Cin \|\| p\.ldo % (\d+) \|\| p\.lda % (\d+) \|\|",
                                                     "si_launch_lingemm"))
    h, i = _one(src["api.hip"], r"ctx->dbg_capture\.empty\(\) && H % (\d+) == 0 && I % (\d+) == 0 &&", "api.hip: ln_fuse")
    c["LNFUSE_H"], c["LNFUSE_I"] = int(h), int(i)
    pc = src["posconv.hip"]
    c["PC_KC"] = int(_one(pc, r"constexpr int PC_KC = (\d+);", "PC_KC"))
    r = _one(pc, r"if \(\(CG != (\d+) && CG != (\d+)\) \|\| \(ntaps \* CG\) % \(32 \* PC_KC\) \|\| pad < 0 \|\| pad > (\d+) \|\| ntaps > (\d+) \|\|", "si_launch_posconv")
    c["PC_CG"], c["PC_PAD_MAX"], c["PC_TAPS_MAX"] = (int(r[0]), int(r[1])), int(r[2]), int(r[3])
    ek = src["encoder_kernels.hip"]
    c["LN_MAX"] = int(_one(ek, r"if \(C % 4 != 0 \|\| C > (\d+)\) return si_fail\(ctx, SI_EINVAL, \"layernorm width", "si_launch_layernorm"))
    c["SI_LN_MAX_WIDTH"] = int(_one(src["weights_host.h"], r"#define SI_LN_MAX_WIDTH (\d+)", "SI_LN_MAX_WIDTH"))
    c["CONV0_K"] = int(_one(ek, r"if \(p\.K != (\d+)\) return si_fail", "conv0_check: K"))
    tpr = int(_one(ek, r"if \(p\.C % 4 != 0 \|\| tpr > (\d+) \|\| \(256 % tpr\) != 0\)", "conv0_check: C"))
    c["CONV0_CMAX"] = 4 * tpr
    wh = src["weights_host.cpp"]
    c["DESC_CONV0_K"] = int(_one(wh, r"if \(d->conv_kernel\[0\] != (\d+)\)", "check_desc: conv_kernel[0]"))
    c["DESC_CONV0_CMAX"] = int(_one(wh, r"if \(d->conv_dim\[0\] > (\d+) \|\|", "check_desc: conv_dim[0]"))
    lds = int(_one(src["weights_host.h"], r"#define SI_POST_MAX_LDS \((\d+) \* 1024\)", "SI_POST_MAX_LDS")) * 1024
    _one(wh, r"\(\(size_t\)\(256 \+ 6\) \* \(c \+ 4\) \+ \(size_t\)7 \* c\) \* 4 > SI_POST_MAX_LDS", "check_desc: conv_post")
    c["POST_CMAX"] = max(C for C in range(4, 4096, 4) if (262 * (C + 4) + 7 * C) * 4 <= lds)
    # ... and the launcher's own form of it: conv_post_kernel's LDS, its cap, and the 7 taps api.hip calls it with
    vk = src["vocoder_kernels.hip"]
    _one(vk, r"const size_t lds = \(\(size_t\)\(256 \+ k - 1\) \* \(C \+ 4\) \+ \(size_t\)k \* C\) \* sizeof\(float\);", "si_launch_conv_post: LDS")
    cap = int(_one(vk, r"if \(lds > (\d+) \* 1024\) return si_fail\(ctx, SI_EINVAL, \"conv_post:", "si_launch_conv_post: cap")) * 1024
    k = int(_one(src["api.hip"], r"return si_launch_conv_post\(ctx, x, wf\(ctx, Ly\.post_w\), wf\(ctx, Ly\.post_b\), Bc, \(int\)Lc, c, (\d+), wav_out", "api.hip: conv_post's taps"))
    c["POST_CMAX_LAUNCHER"] = max(C for C in range(4, 4096, 4) if ((256 + k - 1) * (C + 4) + k * C) * 4 <= cap)
    # ln_fuse's terms beyond the two moduli and the captures (shape_rules.LNFUSE's comment)
    _one(src["api.hip"], r"const bool ln_fuse = e16 && ctx->opt_ln_fuse && ctx->opt_enc_lingemm && !d\.stable_layer_norm && ctx->dbg_capture\.empty\(\) &&", "api.hip: ln_fuse's switches")
    c["LNFUSE_BYTES"] = float(_one(src["api.hip"], r"\(double\)\(BT \+ 128\) \* \(I \+ 128\) \* 2\.0 < ([0-9.e]+);", "api.hip: ln_fuse's workspace bound"))
    return c


WANT = dict(RPN_HALO=S.PAIR_HALO, RPW_HALO=S.PAIR_HALO, PAIR_HALO=S.PAIR_HALO, PAIR_C=S.PAIR_C, PAIR_KMIN=S.PAIR_KMIN, PAIR_KMAX=S.PAIR_KMAX,
            RC_R=S.RC_R, RC_C=S.RC_C, RC_MARG=S.RC_MARG, RC_KMAX=S.RC_KMAX, RC_FRACTION=4, UP_TAPS=S.UP_TAPS, UP_CIN=S.UP_CIN, C_BK=S.C_BK,
            TC_TAPS=S.TC_TAPS, TC_BN=S.TC_BN, GEMMCU_N=S.LG_BN, LG_BN=S.LG_BN, LG_BK=S.LG_BK, LG_LDO=4, LG_LDA=8, LNFUSE_H=S.LNFUSE_H,
            LNFUSE_I=S.LNFUSE_I, PC_KC=S.PC_KC, PC_CG=S.PC_CG, PC_PAD_MAX=S.PC_PAD_MAX, PC_TAPS_MAX=S.PC_TAPS_MAX, LN_MAX=S.LN_MAX,
            SI_LN_MAX_WIDTH=S.LN_MAX, CONV0_K=S.CONV0_K, CONV0_CMAX=S.CONV0_CMAX, DESC_CONV0_K=S.CONV0_K, DESC_CONV0_CMAX=S.CONV0_CMAX,
            POST_CMAX=S.POST_CMAX, POST_CMAX_LAUNCHER=S.POST_CMAX, LNFUSE_BYTES=S.LNFUSE_BYTES)


def mismatches(consts):
    return sorted((k, consts.get(k), v) for k, v in WANT.items() if consts.get(k) != v)


def test_the_restated_constants_are_the_sources():
    """Every constant of the rule table, as the launchers are written today, equals its restatement: a changed rule fails here until the
    restatement -- and with it the cases at and past the limit -- moves too."""
    consts = source_constants()
    assert set(consts) == set(WANT)
    assert mismatches(consts) == []
    # ln_fuse's moduli are what makes its two residual GEMMs (N = H; K = H and I) shapes the dedicated kernels cover
    assert S.LNFUSE_H % S.LG_BN == 0 and S.LNFUSE_I % S.LG_BK == 0 and S.LNFUSE_I % S.C_BK == 0
    # the narrow-stage padding of the fp16 stream lands on the chain's width
    assert S._padded(16) == S.RC_C and S._padded(4) == 32 and S._padded(32) == 32 and S._padded(48) == 48


# ------------------------------------------------------------------------------------------------------------ coverage
def test_every_term_of_every_rule_has_a_case_at_its_limit_and_one_past_it():
    """Per term: a case whose shape satisfies the whole rule with that term at its last accepted value, and a case that breaks exactly that
    term.  The terms no descriptor can break alone, and those whose limit none reaches, are listed with the reason
    (shape_rules.NOT_BREAKABLE_ALONE, LIMIT_NOT_REACHABLE) and must then have no such case."""
    cov = S.coverage()
    assert set(cov) == {(r, t) for r, rule in S.RULES.items() for t in rule}
    for (rule, term), c in sorted(cov.items()):
        print(f"{rule:16s} {term:32s} at the limit: {sorted(set(c['limit']))[:4]}  past: {sorted(set(c['past']))[:4]}")
        if (rule, term) in S.LIMIT_NOT_REACHABLE:
            assert not c["limit"]
        else:
            assert c["limit"], f"{rule}: no case at the limit of '{term}'"
        if (rule, term) in S.NOT_BREAKABLE_ALONE:
            assert not c["past"]
        else:
            assert c["past"], f"{rule}: no case that breaks '{term}' and nothing else"


def test_the_case_tables_hold_what_they_were_asked_to():
    """The cases by name: the (k, d) inside and one step past the pair rule at every width, the mixed block and stage, the chain at each
    limit and refused by each term, the upsamplers, the encoder widths E1 .. E7 and the positional conv shapes."""
    g = S.GEN
    for C in S.PAIR_C:
        assert g[f"pairs C={C} k=5"].dils == ((2, 4, 6),) and g[f"pairs C={C} k=9"].dils == ((1, 2, 6),) and g[f"pairs C={C} k=3 d=25"].dils == ((1, 12, 25),)
        for n in (f"pairs C={C} k=5", f"pairs C={C} k=9", f"pairs C={C} k=3 d=25"):
            fam = S.reaches(g[n])
            assert fam[f"respair_f16_c{C}"] == 3 and not any(k.startswith("reschain") for k in fam), (n, fam)
    for C in (64, 128):
        for n in (f"past C={C} k=3 d=26", f"past C={C} k=11 d=6", f"past C={C} k=13", f"past C={C} k=1"):
            assert set(S.reaches(g[n])) == {"tapgemm_f16"}, n
        assert S.reaches(g[f"block C={C} (1, 25, 26)"]) == {"tapgemm_f16": 4, f"respair_f16_c{C}": 2}
        assert S.reaches(g[f"block C={C} (26, 1, 25)"]) == {"tapgemm_f16": 4, f"respair_f16_c{C}": 2}
        assert S.reaches(g[f"stage C={C} (3, 13, 7)"]) == {"tapgemm_f16": 2 + 6, f"respair_f16_c{C}": 5, f"respair_f16_c{C}_acc": 1}
    for n in ("chain k=3 (25, 25, 25)", "chain k=7 (10, 10, 9)", "chain k=11 (1, 6, 6)", "chain k=3 (32, 25, 25)"):
        assert S.reaches(g[n]) == {"tapgemm_f16": 2, "reschain_f16_c32": 1}, n
    assert set(g["chain k=7 (10, 10, 9)"].lens) >= {575, 576, 577, 1153}
    assert S.RC_R - 6 * (10 + 10 + 9 + 3) == 576                                   # stored rows at the 2 H limit
    for n in [c.name for c in S.GEN_CASES if c.group == "chain refused"]:
        assert not any(k.startswith("reschain") for k in S.reaches(g[n])), n
    assert S.reaches(g["ups stream u=2 k=4 Cin=64"])["upsample_f16_c64"] == 1 and S.reaches(g["ups stream u=2 k=4 Cin=128"])["upsample_f16_c128"] == 1
    for n in ("ups u=4 k=8 Cin=64", "ups u=2 k=2 Cin=128", "ups u=2 k=6 Cin=128", "ups u=3 k=5 Cin=128", "ups u=3 k=7 Cin=128", "ups u=3 k=5 256->128",
              "ups u=16 k=32 96->48", "ups u=4 k=4 Cin=128", "ups u=2 k=4 Cin=32"):
        fam = S.reaches(g[n])
        assert not any(k.startswith(("upsample", "gemmcu")) for k in fam), (n, fam)
    for n in ("ups TC u=6 k=12 256->128", "ups TC u=3 k=5 512->256", "ups TC u=8 k=16 Cin=64", "ups u=2 k=4 Cin=256"):
        assert S.reaches(g[n])["gemmcu_f16"] == 1, n
    for c in S.GEN_CASES:
        assert all(k % 2 == 1 for k in c.ks) and (c.ku - c.u) % 2 == 0 and c.ku >= c.u, c.name      # what the loader admits
    e = {n: S.enc_arch(c) for n, c in S.ENC.items()}
    assert (e["E1"].hidden_size, e["E1"].num_attention_heads, e["E1"].intermediate_size) == (64, 1, 16)
    assert (e["E2"].hidden_size, e["E2"].intermediate_size) == (192, 768) and (e["E3"].hidden_size, e["E3"].intermediate_size) == (384, 1536)
    assert (e["E4a"].hidden_size, e["E4a"].intermediate_size) == (256, 272) and (e["E4b"].hidden_size, e["E4b"].intermediate_size) == (256, 320)
    assert (e["E5"].hidden_size, e["E5"].intermediate_size) == (2048, 64)
    assert e["E6"].conv_dim == (64, 64, 128, 128, 256, 256, 512) and len(e["E6b"].conv_dim) == 2
    assert e["E7"].feat_extract_norm == "layer" and {16, 1040} <= set(e["E7"].conv_dim)
    assert all(a.hidden_size == 64 * a.num_attention_heads and a.num_hidden_layers == 1 for a in e.values())
    r = {n: S.reaches(c) for n, c in S.ENC.items()}
    assert set(r["E2"][op] for op in ("projection", "QKV", "out-proj", "FFN2")) == {"tapgemm_bf16"}
    assert r["E1b"]["FFN1"].startswith("gemmcu") and r["E1c"]["projection"].startswith("gemmcu")
    assert r["E4a"]["FFN2"] == "tapgemm_bf16" and r["E4a"]["FFN1"] == "tapgemm_bf16" and r["E4b"]["FFN1"] == "tapgemm_bf16" and r["E4b"]["FFN2"].startswith("gemmcu")
    assert S.reaches(S.ENC["E3"], captures=False)["ln_residual"] == "fused" and S.reaches(S.ENC["E4b"], captures=False)["ln_residual"] == "fused"
    assert S.reaches(S.ENC["E4a"], captures=False)["ln_residual"] == "written" and S.reaches(S.ENC["E2"], captures=False)["ln_residual"] == "written"
    for n in ("P48k64", "P48k8", "P64k2", "P64k128"):
        assert r[n]["pos_conv"].startswith("posconv_bf16_c"), n
    for n in ("P48k4", "P64k127", "P64k129", "P64k130", "P32", "P80"):
        assert r[n]["pos_conv"] == "tapgemm_bf16", n


# ------------------------------------------------------------------------------------------------------------ seeded mistakes
def _pair_tiled(y, w1, b1, w2, b2, k, d, stored, short=0):
    """A pair kernel emulated tile by tile in float64 with t and the output rounded to fp16: a tile stores `stored` rows and stages the
    y rows its two convolutions reach, (k - 1)(d + 1) / 2 to each side, zeros outside the clip.  short: rows missing at the far end of
    the staged window (the mistake: a halo sized for a smaller (k - 1) d)."""
    L, C = y.shape
    p1, p2 = d * (k - 1) // 2, (k - 1) // 2
    a = V.lrelu16(y).double()
    out = torch.zeros(L, C, dtype=torch.float64)
    for g0 in range(0, L, stored):
        lo, hi = g0 - p1 - p2, min(g0 + stored, L) + p1 + p2
        win = torch.zeros(hi - lo, C, dtype=torch.float64)
        s0, s1 = max(lo, 0), min(hi, L)
        win[s0 - lo:s1 - lo] = a[s0:s1]
        if short:
            win[-short:] = 0
        z1 = torch.nn.functional.conv1d(win.t()[None], w1, dilation=d)[0].t() + b1.double()            # rows g0 - p2 .. of t
        t = V.rne_f16(V.lrelu(z1, V.SLOPE32).clamp(-V.F16_MAX, V.F16_MAX))
        rows = torch.arange(g0 - p2, g0 - p2 + t.shape[0])
        t[(rows < 0) | (rows >= L)] = 0                                                                 # conv 2's zero padding applies to t
        z2 = torch.nn.functional.conv1d(t.t()[None], w2)[0].t() + b2.double()
        n = min(g0 + stored, L) - g0
        out[g0:g0 + n] = z2[:n] + y[g0:g0 + n].double()
    return V.rne_f16(out.clamp(-V.F16_MAX, V.F16_MAX))


def _pair_operands(C, L, k, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(L, C, generator=g).to(torch.float16)
    w = lambda: V.h16(torch.randn(C, C, k, generator=g) / (C * k) ** 0.5)       # noqa: E731
    b = lambda: torch.randn(C, generator=g) * 0.05                              # noqa: E731
    return y, w(), b(), w(), b()


def test_pair_ref_rejects_a_halo_one_row_short_at_d_25():
    """k = 3, d = 25 at C = 32 (254 stored rows, two tiles and a row): the tiled emulation passes pair_ref's bound; with the staged window
    one row short -- a halo sized for (k - 1) d = 49 -- rows at the tile seam fall outside it."""
    C, k, d, stored = 32, 3, 25, 256 - 2
    y, w1, b1, w2, b2 = _pair_operands(C, 2 * stored + 1, k, 5)
    ref, Eb = V.pair_ref(V.lrelu16(y).double(), y.double(), w1, b1, w2, b2, d)
    good = V.check_f16(_pair_tiled(y, w1, b1, w2, b2, k, d, stored), ref, Eb)
    assert good["bad"] == 0, good["bad"]
    r = V.check_f16(_pair_tiled(y, w1, b1, w2, b2, k, d, stored, short=1), ref, Eb)
    assert r["bad"] > 0
    bad_rows = set((~r["ok"]).any(dim=1).nonzero().flatten().tolist())
    assert bad_rows <= {stored - 1, 2 * stored - 1}, sorted(bad_rows)                 # the last stored row of each whole tile reads the missing row


def test_linear_ref_rejects_a_dropped_last_k_step_at_K_64():
    """K = 64 is two MFMA k-steps of 32: an fp32 evaluation passes linear_ref's bound, one that stops after the first k-step does not."""
    g = torch.Generator().manual_seed(6)
    a = E.bf16(torch.randn(140, 64, generator=g))
    w = torch.randn(128, 64, generator=g) / 8
    b = torch.randn(128, generator=g) * 0.05
    ref, bound = E.linear_ref(a, w, b)
    wb = w.to(torch.bfloat16).float()
    good = a.float() @ wb.t() + b
    assert E.check_f32(good, ref, bound)["bad"] == 0
    dropped = a.float()[:, :32] @ wb[:, :32].t() + b
    assert E.check_f32(dropped, ref, bound)["bad"] > 0.9 * ref.numel()


def test_pair_ref_rejects_a_swapped_hand_off_buffer_in_a_mixed_block():
    """The block (1, 25, 26): x1 = pair(x0) lands in one hand-off buffer, x2 = pair(x1) in the other, and the third pair -- on the tap-GEMM,
    d = 26 -- reads x2.  The GPU test holds its output to pair_ref on the TAPPED x2; a third pair that read the other buffer (x1) fails it."""
    C, k, L = 64, 3, 300
    y, w1, b1, w2, b2 = _pair_operands(C, L, k, 7)
    step = lambda x, d: V.rne_f16(V.pair_ref(V.lrelu16(x.to(torch.float16)).double(), x.double(), w1, b1, w2, b2, d, round_t=True)[0].clamp(-V.F16_MAX, V.F16_MAX))   # noqa: E731
    x1 = step(y, 1)
    x2 = step(x1, 25)
    ref, Eb = V.pair_ref(V.lrelu16(x2.to(torch.float16)).double(), x2, w1, b1, w2, b2, 26)
    assert V.check_f16(step(x2, 26), ref, Eb)["bad"] == 0
    assert V.check_f16(step(x1, 26), ref, Eb)["bad"] > 0.5 * ref.numel()
