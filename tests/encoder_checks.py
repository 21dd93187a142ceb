"""The bf16 encoder's tapped run and its checks of every op against tests/encoder_ref.py, for tests/test_gpu_encoder_ops.py (the real
widths) and tests/test_gpu_shape_rules.py (the widths on both sides of every launcher's shape rule).  What is checked and why:
test_gpu_encoder_ops.py's docstring.  A plain module: no fixture; importing it needs no GPU."""
import torch

from tests import encoder_ref as E
from tests import vocoder_ref as V
from tests.cases import _config, _sel_rows
from tests.cases import _enc_state as _state
from tests.harness import build_engine, tapped_run

GEMMCU_BM = {10: 320, 11: 256, 12: 160, 13: 224, 14: 128, 15: 208}
GEMMCU_BN = {10: 256, 11: 256, 12: 128, 13: 128, 14: 128, 15: 256}
# Fraction of a launch's bf16 outputs that differ from rne(float64 result), the bf16 value nearest to the exact one: twice the
# worst measured over this file's runs on MI355X (GEMM / conv 0.395 %, conv0 + GroupNorm 0.051 %, LayerNorm + GELU 0.032 %,
# attention_kernel with a bf16 output 0.0061 %; the projection LayerNorm's C = 512 operand, "features.ln.bf16", measured at most
# 0.0059 % against the float64 reference over 24 runs, so it is held to "ln" and has no key of its own).  The bf16-input
# attention kernels round P to bf16 before P V, so about one output in five lands on the other neighbour of the exact value
# (measured up to 18.6 %, at T = 31); their limit is the same twice-measured guard, the error bound above being the check on
# their arithmetic.
MISMATCH_LIMIT = {"gemm": 0.0079, "conv0": 0.00103, "ln": 0.00064, "attention": 0.00012, "attention_p16": 0.372}


def _engine(harch, env=None, key=None):
    """bf16 encoder; `env` knobs are read when the context is created."""
    from speech_inpainting_amd.arch import VocoderArch
    return build_engine(harch, VocoderArch.tiny(), 50, "bf16", "fp32", env=env, state=(_state(harch), None, None), key=key)


def _run(eng, harch, wave, lens=None, valid_len=None, profile=False):
    """One encoder forward with every per-op tap registered (and "features", "projected", the projection's two ends) -> (taps
    {name: cpu tensor} of the taps the path produced, rows of the transformer, kernel names if profiled)."""
    B, N = wave.shape
    R = sum(harch.num_frames(n) for n in lens) if lens is not None else B * harch.num_frames(N)
    cap = E.tap_capacities(harch, B, N, R)
    cap["features"], cap["projected"] = R * harch.conv_dim[-1], R * harch.hidden_size
    got, out, prof = tapped_run(eng.ctx, cap, lambda: eng.encode_ragged(wave, lens) if lens is not None
                                else eng.encode(wave, valid_len=valid_len, normalize=False), profile=profile)
    assert bool(torch.isfinite(out).all())
    return got, R, set(prof)


def _f64(t):
    return t.double()


def _check(tag, kind, got, ref, bound, limit_key="gemm", limits=None, notes=None):
    """A stored tensor against (ref, bound) over all its elements; a bf16 tensor also against the share of outputs that may differ from
    rne(ref): MISMATCH_LIMIT[limit_key], or the caller's `limits` {key: share, or None for "recorded only"}.  notes: a list that
    receives (tag, kind, limit key, mismatch share, max err / bound) of the check, for the caller's own limits and summary."""
    r = E.check_bf16(got, ref, bound) if kind == "bf16" else E.check_f32(got, ref, bound)
    print("   " + E.fmt(tag, r))
    assert r["bad"] == 0, E.fmt(tag, r)
    if notes is not None:
        notes.append((tag, kind, limit_key, r.get("mismatch"), r["worst"]))
    limit = (MISMATCH_LIMIT if limits is None else limits)[limit_key]
    if kind == "bf16" and limit is not None:
        assert r["mismatch"] <= limit, E.fmt(tag, r)
    return r


def _tap(got, name):
    """(tensor, 'bf16' | 'f32') of whichever form of the tap the path stored."""
    if name + ".bf16" in got:
        return got[name + ".bf16"], "bf16"
    return got[name], "f32"


def _check_layers(got, harch, R, tag, rows=None, **ck):
    """Every GEMM of every captured layer against linear_ref on its captured operands."""
    sd = _state(harch)
    H = harch.hidden_size
    rows = torch.arange(R) if rows is None else rows
    for l in range(harch.num_hidden_layers):
        p = f"base_model.encoder.layers.{l}."
        pre = harch.do_stable_layer_norm
        hin = got[f"layer{l}.h"].view(R, H)[rows]
        if f"layer{l}.h.bf16" in got:
            a_qkv = got[f"layer{l}.h.bf16"].view(R, H)[rows]
        else:                                                              # fp32 operand, rounded by the GEMM's staging
            a_qkv = E.bf16(got[f"layer{l}.ln1"].view(R, H)[rows] if pre else hin)
        wqkv = torch.cat([sd[p + f"attention.{n}_proj.weight"] for n in "qkv"])
        bqkv = torch.cat([sd[p + f"attention.{n}_proj.bias"] for n in "qkv"])
        qkv, kq = _tap(got, f"layer{l}.qkv")
        _check(f"{tag} layer{l} QKV", kq, qkv.view(R, 3 * H)[rows], *E.linear_ref(_f64(a_qkv), wqkv, bqkv), **ck)
        att, ka = _tap(got, f"layer{l}.att")
        a_out = _f64(att.view(R, H)[rows]) if ka == "bf16" else E.bf16(att.view(R, H)[rows])
        _check(f"{tag} layer{l} out-proj + residual", "f32", got[f"layer{l}.att_res"].view(R, H)[rows],
               *E.linear_ref(a_out, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"], res=hin), **ck)
        if pre:
            a_ffn = got[f"layer{l}.ln2.bf16"].view(R, H)[rows] if f"layer{l}.ln2.bf16" in got else E.bf16(got[f"layer{l}.ln2"].view(R, H)[rows])
            res2 = got[f"layer{l}.att_res"].view(R, H)[rows]
        else:
            a_ffn = got[f"layer{l}.ln1.bf16"].view(R, H)[rows] if f"layer{l}.ln1.bf16" in got else E.bf16(got[f"layer{l}.ln1"].view(R, H)[rows])
            res2 = got[f"layer{l}.ln1"].view(R, H)[rows]
        I = harch.intermediate_size
        ffn, kf = _tap(got, f"layer{l}.ffn")
        _check(f"{tag} layer{l} FFN1 + GELU", kf, ffn.view(R, I)[rows],
               *E.linear_ref(_f64(a_ffn), sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"], act="gelu"), **ck)
        a2 = _f64(ffn.view(R, I)[rows]) if kf == "bf16" else E.bf16(ffn.view(R, I)[rows])
        _check(f"{tag} layer{l} FFN2 + residual", "f32", got[f"layer{l}.ffn_res"].view(R, H)[rows],
               *E.linear_ref(a2, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"], res=res2), **ck)


GEMMCU_CFGS = ((320, 256), (256, 256), (160, 128), (224, 128), (128, 128), (208, 256))     # gemmcu.hip, k_cfgs: (BM, BN) of instantiation c


def _linear_kernel(M, N, K, env=None, x16=True):
    """The profile name of one Linear of the bf16 encoder (one tap, one flat segment of M rows), restating the launchers'
    rules: si_launch_tapgemm hands an operand-ready (bf16) input to si_launch_lingemm unless SI_ENC_LINGEMM=0; that tries
    si_launch_gemmcu first (SI_ENC_GEMMCU: 0 never, 10 + c instantiation c wherever BN divides N, 1 the whole-rounds rule over the
    device's CUs), then picks its own tile height by rounds x (BM + 24) over two workgroup slots per CU; everything else runs
    launch_math's bf16 branch: eight light waves on a 128 x 128 tile for an operand-ready input of M > 256 rows ("w8"), else four."""
    env = env or {}
    if N < 128:                                                        # a 64- or 32-column tile: launch_math's narrow branch, as cases._config restates it
        return _config("bf16", N, M, 1, 1, K)[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    opt = int(env.get("SI_ENC_GEMMCU", "1"))
    if x16 and env.get("SI_ENC_LINGEMM", "1") != "0" and N % 128 == 0 and K % 64 == 0:
        pick = -1
        if opt >= 10:
            pick = opt - 10 if N % GEMMCU_CFGS[opt - 10][1] == 0 else -1
        elif opt > 0:
            best, fills_256 = 1e30, False
            for c, (bm, bn) in enumerate(GEMMCU_CFGS):
                if N % bn:
                    continue
                rb = -(-M // bm)
                tiles = rb * (N // bn)
                rounds = -(-tiles // cus)
                fill = tiles / (rounds * cus)
                if c == 1:
                    fills_256 = K >= 128 and fill * M / (rb * bm) >= 0.72
                if opt == 1 and (fill < (0.6 if rounds == 1 else 0.75) or M < 0.75 * rb * bm):
                    continue
                if rounds * (bm + bn) < best:
                    best, pick = rounds * (bm + bn), c
            if pick < 0 and opt == 1 and fills_256:
                pick = 1
        if pick >= 0:
            return "gemmcu_bf16_%dx%d" % GEMMCU_CFGS[pick]
        best, height = 1e30, 128
        for cand in (128, 96, 64):
            tiles = -(-M // cand) * (N // 128)
            cost = -(-tiles // (2 * cus)) * (cand + 24)
            if cost < best * 0.97:
                best, height = cost, cand
        return f"lingemm_bf16_{height}x128"
    return "tapgemm_bf16_128x128w8" if x16 and M > 256 and K % 32 == 0 else "tapgemm_bf16_128x128"      # (the light waves need BK = 32)


def _check_projection(got, harch, R, tag, names, env=None, rows=None, **ck):
    """The feature projection, op by op: its LayerNorm(512) from "features" to "features.ln.bf16" (the rows are stored as the GEMM's
    bf16 operand only) against layernorm_ref, then Linear(512 -> H) -- the encoder's only GEMM with K = 512 -- from that operand to
    "projected" against linear_ref.  Without the LayerNorm the GEMM's staging rounds the fp32 features.  `names`: the run's profile,
    which must hold the kernel the launchers' rule gives this GEMM."""
    sd = _state(harch)
    p = "base_model.feature_projection."
    CF, H = harch.conv_dim[-1], harch.hidden_size
    rows = torch.arange(R) if rows is None else rows
    feats = got["features"].view(R, CF)[rows]
    if harch.feat_proj_layer_norm:
        assert "features.ln.bf16" in got and "features.ln" not in got, sorted(got)
        op = got["features.ln.bf16"].view(R, CF)[rows]
        ref, bound = E.layernorm_ref(feats, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], harch.layer_norm_eps)
        _check(f"{tag} projection LayerNorm (C = {CF}) bf16 operand", "bf16", op, ref, bound, "ln", **ck)
        a = _f64(op)
        kern = _linear_kernel(R, H, CF, env)
    else:
        assert "features.ln.bf16" not in got and "features.ln" not in got, sorted(got)
        a = E.bf16(feats)                                              # fp32 operand, rounded by the GEMM's staging
        kern = _linear_kernel(R, H, CF, env, x16=False)
    ref, bound = E.linear_ref(a, sd[p + "projection.weight"], sd[p + "projection.bias"])
    y = got["projected"].view(R, H)[rows]
    _check(f"{tag} projection (K = {CF}) [{kern}]", "f32", y, ref, bound, **ck)
    ratio = ((y.double() - ref).abs() / bound).amax(1)
    bm = int(kern.split("_")[2].split("x")[0])                         # the kernel's tile height
    last = rows >= (R - 1) // bm * bm                                  # rows of the last (partial) row tile | the rest
    print(f"   [{kern}] max err/E last tile {float(ratio[last].max()):.2e}, the rest {float(ratio[~last].max()) if bool((~last).any()) else 0.0:.2e}")
    assert kern in names, (kern, sorted(names))


def _check_convs(got, harch, B, N, tag, clip_lens=None, **ck):
    """Strided convs 1..n-1 of every clip against linear_ref on their captured inputs (rows: _sel_rows of the clip's own length)."""
    sd = _state(harch)
    Ls = harch.feat_lengths(N)
    layer = harch.feat_extract_norm == "layer"
    pre = "base_model.feature_extractor.conv_layers."
    for i in range(1, len(harch.conv_dim)):
        Cin, C, k, s = harch.conv_dim[i - 1], harch.conv_dim[i], harch.conv_kernel[i], harch.conv_stride[i]
        xin, kin = _tap(got, f"conv{i - 1}.ln" if layer else f"conv{i - 1}")
        y, ky = _tap(got, f"conv{i}")
        xin = xin.view(B, Ls[i], Cin)
        y = y.view(B, Ls[i + 1], C)
        w = E.conv_weight(sd[pre + f"{i}.conv.weight"])
        bias = sd[pre + f"{i}.conv.bias"] if harch.conv_bias else None
        for b in sorted({0, 1, B - 1}) if B > 3 and clip_lens is None else range(B):
            Lb = harch.feat_lengths(clip_lens[b])[i + 1] if clip_lens is not None else Ls[i + 1]
            rows = _sel_rows(Lb, seed=b)
            xb = _f64(xin[b]) if kin == "bf16" else E.bf16(xin[b])
            ref, bound = E.linear_ref(E.conv_rows(xb, k, s, rows), w, bias, act=None if layer else "gelu")
            _check(f"{tag} conv{i} clip {b} (L = {Lb})", ky, y[b][rows], ref, bound, **ck)


# ------------------------------------------------------------------------------------------------------------ attention
def _check_attention(got, harch, clips, tag, kind_out=None, p_bf16=True, **ck):
    """clips: [(first packed row, T, Tk)]; every query row of every clip, padded ones included."""
    H, heads = harch.hidden_size, harch.num_attention_heads
    qkv, kq = _tap(got, "layer0.qkv")
    att, ka = _tap(got, "layer0.att")
    R = att.numel() // H
    qkv, att = qkv.view(R, 3 * H), att.view(R, H)
    if kind_out is not None:
        assert ka == kind_out, (ka, kind_out)
    for r0, T, Tk in clips:
        q = _f64(qkv[r0:r0 + T]) if kq == "bf16" or not p_bf16 else E.bf16(qkv[r0:r0 + T])
        ref, bound = E.attention_ref(q, heads, Tk=Tk, p_bf16=p_bf16)
        _check(f"{tag} T={T} keys={Tk}", ka, att[r0:r0 + T], ref, bound, "attention_p16" if p_bf16 else "attention", **ck)


# ------------------------------------------------------------------------------------------------------- positional conv
PC_HALF = 256                                          # posconv.hip, PC_HALF_ROWS: output rows per half of a workgroup's tile
PC_KERNELS = {"posconv": {}, "tapgemm": {"SI_ENC_POSCONV": "0"}}


def _pc_both(harch, wave, lens=None, valid_len=None, key=None, covered=True):
    """The same batch through posconv.hip and through the SI_ENC_POSCONV=0 fallback -> {kernel: (taps, profile name of the conv's
    kernel)}.  The profile must name the one and none of the other; "projected", the conv's input, must be equal in both runs.
    covered=False: a shape si_launch_posconv refuses -- the default engine must take the fallback by itself, with the same bits."""
    cg = harch.hidden_size // harch.num_conv_pos_embedding_groups
    runs = {}
    for kernel in PC_KERNELS:
        eng = _engine(harch, PC_KERNELS[kernel], key=None if key is None else key + (kernel,))
        got, R, names = _run(eng, harch, wave, lens=lens, valid_len=valid_len, profile=True)
        ran = {n for n in names if n.startswith("posconv_")}
        if kernel == "posconv" and covered:
            name = f"posconv_bf16_c{cg}"
            assert ran == {name}, names
        else:                                                          # the grouped tap-GEMM on the fp32 rows: N = Cg in its own Npad
            name = _config("bf16", cg, harch.num_frames(wave.shape[1]), harch.num_conv_pos_embeddings, 1, cg)[0]
            assert not ran and name in names and name.startswith("tapgemm_bf16_"), names
        runs[kernel] = (got, name)
    assert torch.equal(runs["posconv"][0]["projected"], runs["tapgemm"][0]["projected"])
    if not covered:
        assert torch.equal(runs["posconv"][0]["pos_conv"], runs["tapgemm"][0]["pos_conv"]), "the fallback taken by the rule differs from the one asked for"
    return runs


def _check_posconv(runs, harch, clips, tag, valid=None):
    """Every row and channel of every clip at the "pos_conv" tap, of both kernels, against ONE float64 reference per clip on the
    captured "projected" rows.  clips: [(first packed row, T)]; valid: the clips' valid frame counts in a padded batch ("projected"
    is tapped before the padded frames are zeroed, so the reference zeroes them itself).  -> the largest err / E."""
    sd = _state(harch)
    H, G, k = harch.hidden_size, harch.num_conv_pos_embedding_groups, harch.num_conv_pos_embeddings
    cg = H // G
    w, bias = E.pos_conv_weight(sd), sd["base_model.encoder.pos_conv_embed.conv.bias"]
    geom = E.pos_conv_geom(k, G)
    proj = runs["posconv"][0]["projected"]
    R = proj.numel() // H
    worst = 0.0
    for i, (r0, T) in enumerate(clips):
        h = proj.view(R, H)[r0:r0 + T]
        if valid is not None:
            h = h.clone()
            h[valid[i]:] = 0
        r = V.tapgemm_ref(h, w, bias, "bf16", geom, k * cg, act="gelu", res=h)
        for kernel, (got, name) in runs.items():
            c = V.check_f32(got["pos_conv"].view(R, H)[r0:r0 + T], r.ref, r.E)
            line, near, rest = V.report(tag, name, i, c, T, PC_HALF, 64)
            print(f"   {line} ({near:.2e} | {rest:.2e})")
            assert c["finite"] and c["bad"] == 0, line
            worst = max(worst, near, rest)
    return worst


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _check_layernorms(got, harch, B, N, R, tag, **ck):
    """Every LayerNorm of the run against layernorm_ref on its captured input: the transformer's two per layer (post-LN: fp32 rows and
    their bf16 operand, bit-equal to rne of the rows; pre-LN: the bf16 operand only) and, in the layer flavour, LayerNorm + GELU behind
    every conv (bf16 only, the last one fp32)."""
    sd = _state(harch)
    H = harch.hidden_size
    p = "base_model.encoder.layers.0."
    if not harch.do_stable_layer_norm:
        for ln, x, key in (("ln1", "att_res", "layer_norm"), ("ln2", "ffn_res", "final_layer_norm")):
            rows = got[f"layer0.{ln}"].view(R, H)
            ref, bound = E.layernorm_ref(got[f"layer0.{x}"].view(R, H), sd[p + key + ".weight"], sd[p + key + ".bias"], harch.layer_norm_eps)
            _check(f"{tag} {ln} (C = {H}) fp32 rows", "f32", rows, ref, bound, **ck)
            op = got[f"layer0.{ln}.bf16"].view(R, H)
            assert torch.equal(op, rows.to(torch.bfloat16)), f"{ln}: the bf16 operand is not rne of the fp32 rows"
    else:
        h = got["layer0.h"].view(R, H)
        ref, bound = E.layernorm_ref(h, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], harch.layer_norm_eps)
        _check(f"{tag} ln1 (C = {H}) bf16 operand", "bf16", got["layer0.ln1.bf16"].view(R, H), ref, bound, "ln", **ck)
        ref, bound = E.layernorm_ref(got["layer0.att_res"].view(R, H), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], harch.layer_norm_eps)
        _check(f"{tag} ln2 (C = {H}) bf16 operand", "bf16", got["layer0.ln2.bf16"].view(R, H), ref, bound, "ln", **ck)
    if harch.feat_extract_norm == "layer":
        pre = "base_model.feature_extractor.conv_layers."
        Ls = harch.feat_lengths(N)
        for i in range(len(harch.conv_dim)):
            C = harch.conv_dim[i]
            x = got[f"conv{i}"].view(B, Ls[i + 1], C)
            y, ky = _tap(got, f"conv{i}.ln")
            y = y.view(B, Ls[i + 1], C)
            for b in range(B):
                rows = _sel_rows(Ls[i + 1], seed=b)
                ref, bound = E.layernorm_ref(x[b][rows], sd[pre + f"{i}.layer_norm.weight"], sd[pre + f"{i}.layer_norm.bias"], 1e-5, act="gelu")
                _check(f"conv{i} LayerNorm + GELU (C = {C}) clip {b}", ky, y[b][rows], ref, bound, "ln", **ck)
