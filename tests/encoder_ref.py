"""Float64 references of the bf16 encoder's kernels, op by op, each with an explicit per-element error bound.

Every reference takes the kernel's OWN operands (the activations as the previous kernel stored them, captured through the
encoder's per-op taps) and computes in float64.  GEMM weights are rounded to bf16 the way the packer rounds them (round to
nearest, ties to even: `torch.Tensor.to(torch.bfloat16)` of the fp32 weight); biases, residuals and LayerNorm parameters
stay fp32.  The bounds are derived in the docstrings from the kernels' arithmetic; none is fitted to a measurement.

Notation.  u = 2^-24 is the unit roundoff of an fp32 operation that rounds to nearest.  MFMA accumulation is bounded with
U_ACC = 2^-23, which also covers an accumulator whose internal adds truncate instead of rounding.  gamma(n) = n U / (1 - n U)
bounds the relative error of any order of summing n products into an fp32 accumulator (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., Lemma 3.1 and eq. 3.5), whichever tree the hardware uses.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
U_ACC = 2.0 ** -23
# |erf error| of Abramowitz-Stegun 7.1.26 (the GEMM epilogues' si_gelu_fast) plus its fp32 evaluation: one rcp, one exp2 and
# five fma / mul steps, each within 2 ulp of a quantity <= 1 -> 16 u of slack on an erf in [-1, 1]
ERF_FAST = 1.5e-7 + 16 * U
# max |d/dx erf-GELU(x)| over the reals (at x = 2.4: 1.1289...)
GELU_LIP = 1.13


def gamma(n, u=U_ACC):
    return n * u / (1.0 - n * u)


def bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 -> float64: the packer's rounding of a weight, and a kernel's rounding of an fp32 value it stores as bf16."""
    return x.float().to(torch.bfloat16).double()


def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even) in ONE rounding, as float64 (no detour through fp32)."""
    x = x.double()
    return torch.round(x / ulp_bf16(x)) * ulp_bf16(x)


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of the bf16 values around |x| (8 significant bits): 2^(e - 8) for |x| in [2^(e-1), 2^e)."""
    _, e = torch.frexp(x.double().abs())
    e = torch.where(x == 0, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 8).clamp(min=-133))


def ulp_f32(x: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(x.double().abs())
    e = torch.where(x == 0, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 24).clamp(min=-149))


def gelu(x: torch.Tensor) -> torch.Tensor:
    return F.gelu(x.double())


def gelu_fast_err(z: torch.Tensor) -> torch.Tensor:
    """|si_gelu_fast(z) - gelu(z)| in fp32: 0.5 x (1 + erf) with erf off by <= ERF_FAST, (1 + erf) and the two products rounded
    (<= 3 u |gelu|).  The libm erff form (gelu_erf) is within the same bound."""
    z = z.double()
    return 0.5 * z.abs() * ERF_FAST + 3 * U * gelu(z).abs()


# ----------------------------------------------------------------------------------------------------------- GEMM / conv
def linear_ref(a, w, b=None, res=None, act=None, round_w=True, fp32_products=False):
    """out = epi(a W^T + b) [+ res] in float64, and a bound E on |fp32 out - ref| (before any bf16 rounding of the store).

    a (M, K): the kernel's operand as stored (bf16 values, or fp32 for the tap-GEMM's fp32-input path); w (N, K) fp32, rounded
    to bf16 when round_w; b (N,) and res (M, N) fp32; act None or "gelu".

    The MFMA multiplies bf16 pairs exactly and accumulates in fp32: with S = sum_k |a_k||w_k| + |b|, the pre-activation
    z = acc + b satisfies |fl(z) - z| <= gamma(K + 1) S (K products and the bias into one sum).  A residual adds one more
    term to the same sum: |out - ref| <= gamma(K + 2) (S + |res|).  With act = "gelu" the output is GELU(z): |GELU'| <= GELU_LIP
    carries the sum error, and the epilogue's own erf adds gelu_fast_err(z), so E = GELU_LIP gamma(K + 1) S + gelu_fast_err(z).

    fp32_products (the tap-GEMM's exact-fp32 path, round_w=False: operands and weights are the fp32 values themselves): a
    product of two fp32 values is not exact in fp32.  v_mfma_f32_32x32x2_f32 either rounds it before adding it (relative U) or
    fuses it; the bound holds for both: U (1 + gamma) sum |a||w| on top of gamma on S, i.e. gamma -> gamma + U (1 + gamma).
    """
    a = a.double()
    wd = bf16(w) if round_w else w.double()
    K = a.shape[-1]
    z = a @ wd.t()
    S = a.abs() @ wd.abs().t()
    if b is not None:
        z = z + b.double()
        S = S + b.double().abs()
    g1, g2 = gamma(K + 1), gamma(K + 2)
    if fp32_products:
        g1, g2 = g1 + U * (1 + g1), g2 + U * (1 + g2)
    if act == "gelu":
        return gelu(z), GELU_LIP * g1 * S + gelu_fast_err(z)
    if res is not None:
        return z + res.double(), g2 * (S + res.double().abs())
    return z, g1 * S


def layernorm_of_bounded(x, Ex, g, b, eps):
    """LayerNorm of an fp32 row x~ known only as |x~ - x| <= Ex per element: (ref, E) with ref = LN(x) in float64 and E = the
    kernel's own error on x~ (layernorm_ref's bound evaluated at x and scaled by 1 + 2 e / sigma: between x and x~ it changes by second-order terms U e only)
    plus the passage of Ex through the normalisation.  With e = max_c Ex of the row: the mean moves by <= e, every x - mu by
    <= 2 e, sigma = sqrt(var + eps) by <= e (the RMS of delta - mean(delta) is at most that of delta, and sqrt(. + eps) is
    1-Lipschitz in the RMS); so z = (x - mu) / sigma moves by |dn sigma - n dsigma| / (sigma (sigma + dsigma)) <= (2 + |z|) e / (sigma - e),
    times |g|."""
    ref, E = layernorm_ref(x, g, b, eps)
    x = x.double()
    e = Ex.double().amax(-1, keepdim=True)
    mu = x.mean(-1, keepdim=True)
    sigma = torch.sqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps)
    z = (x - mu) / sigma
    assert bool((sigma > 2 * e).all())
    return ref, E * (1 + 2 * e / sigma) + g.double().abs() * (2 + z.abs()) * e / (sigma - e)


def conv_rows(x, k, stride, rows):
    """(L, Cin) input of one clip -> (len(rows), k * Cin) im2col rows [tap][ci] of the given output rows."""
    idx = rows[:, None] * stride + torch.arange(k)[None, :]
    return x[idx].reshape(len(rows), -1)


def conv_weight(w):
    """Conv1d weight (N, Cin, k) -> (N, k * Cin) with the im2col's [tap][ci] order."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1)


# ----------------------------------------------------------------------------------------------------------- attention
def attention_ref(qkv, heads, Tk=None, p_bf16=True):
    """One clip's self-attention, head_dim 64, in float64, and a bound E on |fp32 out - ref| before the store's rounding.

    qkv (T, 3H) holds the kernel's operands as float64 (bf16 values for the bf16 kernels; fp32 for attention_kernel).  The query
    is scaled by 2^-3 (exact), keys >= Tk are excluded for every query row.  p_bf16: P is rounded to bf16 before P V (the bf16
    MFMA kernels) but the normaliser sums the fp32 P.

    With p^_k = softmax weights, o = sum p^_k v_k and m the row max of the scores:
      * score s_k = q . k_k is a 64-term fp32 sum: |ds_k| <= gamma(65) sum_d |q_d||k_kd|; exp(s_k - m') with the running max
        m' <= m, so the perturbation of p_k is a factor within exp(|ds_k|), i.e. a relative eta_k = expm1(|ds_k|), and
        __expf adds a relative 3 u (v_exp_f32 and the scaling by log2 e) + 2 u |s_k - m| (the rounded argument).  A shift of
        the max is common to numerator and denominator and cancels.
      * numerator: P rounded to bf16 (relative beta = 2^-8, the unit roundoff of an 8-significant-bit format: a p just above a
        power of two moves by up to half of its 2^-7 relative spacing; numerator only) and an fp32 sum of Tk + ceil(Tk / 32) terms
        (gamma(n) sum p^|v|); denominator: the same sum of P, gamma(n).
      * N~/D~ - o = [sum p^ eta (v - o) + sum p^ (1 + eta) beta v + e_N - o e_D] / D~ with D~ >= 1 - eta_max - gamma(n)(1 + eta_max):
        E_core = [sum p^ eta |v - o| + beta sum p^ (1 + eta) |v| + gamma(n)(1 + eta_max)((1 + beta) sum p^ |v| + |o|)] / D~_min
      * the online rescale (one fp32 multiply per key tile on o and on l) and the final 1 / l and product: (2 + 2 tiles) u.
    Returns (ref (T, H), E (T, H)).
    """
    qkv = qkv.double()
    T, H3 = qkv.shape
    H = H3 // 3
    Tk = T if Tk is None else max(1, min(int(Tk), T))
    q = (qkv[:, :H] * 0.125).reshape(T, heads, 64).transpose(0, 1)          # (h, T, 64)
    k = qkv[:Tk, H:2 * H].reshape(Tk, heads, 64).transpose(0, 1)
    v = qkv[:Tk, 2 * H:].reshape(Tk, heads, 64).transpose(0, 1)
    s = q @ k.transpose(1, 2)                                                  # (h, T, Tk)
    ds = gamma(65) * (q.abs() @ k.abs().transpose(1, 2))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    ph = p / p.sum(-1, keepdim=True)
    o = ph @ v                                                                 # (h, T, 64)
    eta = torch.expm1(ds) + 3 * U + 2 * U * (s - m).abs()
    eta_max = eta.amax(-1, keepdim=True)
    beta = 2.0 ** -8 if p_bf16 else 0.0
    n = Tk + (Tk + 31) // 32
    g = gamma(n)
    pv = ph @ v.abs()
    w = ph * eta
    dev = torch.empty_like(o)
    for r0 in range(0, T, 64):                                                 # sum_k w_k |v_k - o| in row blocks (bounded memory)
        r1 = min(T, r0 + 64)
        dev[:, r0:r1] = (w[:, r0:r1, :, None] * (v[:, None, :, :] - o[:, r0:r1, None, :]).abs()).sum(2)
    num = dev + beta * ((ph * (1 + eta)) @ v.abs()) + g * (1 + eta_max) * ((1 + beta) * pv + o.abs())
    core = num / (1 - eta_max - g * (1 + eta_max))
    tiles = (Tk + 31) // 32
    E = core + (2 + 2 * tiles) * U * (o.abs() + core)
    return o.transpose(0, 1).reshape(T, H), E.transpose(0, 1).reshape(T, H)


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm_ref(x, g, b, eps, act=None):
    """LayerNorm over the last dim (biased variance, as F.layer_norm) in float64 [+ erf-GELU], and a bound E on the fp32 rows.

    The kernel (layernorm_kernel): mu = (C-term fp32 sum) / C, d = x - mu, var = (C-term fp32 sum of d^2) / C,
    rstd = rsqrtf(var + eps), y = fma(d * rstd, g, b).  With u-rounded VALU steps:
      * |dmu| <= gamma(C, u) mean|x| + u |mu|;
      * the variance sums (d - dmu)^2 = d^2 - 2 d dmu + dmu^2 (the middle term sums to 0): relative gamma(C + 2, u) on the sum
        plus C dmu^2 / sum d^2, and u for / C and for + eps;  rsqrtf: 2 u;  rstd therefore within
        rho = (gamma(C + 2, u) + C dmu^2 / sum d^2 + 2 u) var / (2 (var + eps)) + 2 u relative;
      * y: |g| rstd (|dmu| + |d| (rho + 2 u)) (the subtraction, the product) + u |y| (the fma), the second-order terms
        (dmu rho) being covered by a factor 1 + 2^-10.
    act = "gelu": GELU_LIP E + gelu_fast_err(y).  Returns (ref, E).
    """
    x = x.double()
    g = g.double()
    b = b.double()
    C = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    ssq = d.pow(2).sum(-1, keepdim=True)
    var = ssq / C
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd * g + b
    dmu = gamma(C, U) * x.abs().mean(-1, keepdim=True) + U * mu.abs()
    rel_var = gamma(C + 2, U) + C * dmu.pow(2) / ssq.clamp_min(1e-300) + 2 * U
    rho = rel_var * var / (2 * (var + eps)) + 2 * U
    E = (g.abs() * rstd * (dmu + d.abs() * (rho + 2 * U)) + U * y.abs()) * (1 + 2.0 ** -10)
    if act == "gelu":
        return gelu(y), GELU_LIP * E + gelu_fast_err(y)
    return y, E


def ln_linear_ref(x, ln_g, ln_b, eps, w, b):
    """LayerNorm + Linear on the exact-fp32 tap-GEMM when the LayerNorm's rows are not stored apart (the head; the feature
    projection): ref = LN(x) W^T + b in float64.  The LayerNorm's own bound Ey (layernorm_ref) passes through the Linear as
    sum |w| Ey, and the Linear's bound (linear_ref, fp32_products) is taken at the operand magnitude |y| + Ey.  ln_g None: the
    Linear alone."""
    if ln_g is None:
        return linear_ref(x, w, b, round_w=False, fp32_products=True)
    y, Ey = layernorm_ref(x, ln_g, ln_b, eps)
    ref, _ = linear_ref(y, w, b, round_w=False, fp32_products=True)
    _, bound = linear_ref(y.abs() + Ey, w.abs(), b.abs(), round_w=False, fp32_products=True)
    return ref, bound + Ey @ w.double().abs().t()


def pos_conv_weight(sd, prefix="base_model.encoder.pos_conv_embed.conv."):
    """The packer's fold of the positional conv (Packer::folded with norm_dim = 2: weight-norm over every dim but the taps'): squares
    summed in double, the root rounded to fp32 once, w = v * (g / norm) in fp32.  -> (H, H / groups, k) fp32."""
    if prefix + "weight" in sd:
        return sd[prefix + "weight"].float()
    new = prefix + "parametrizations.weight.original0" in sd
    g = sd[prefix + ("parametrizations.weight.original0" if new else "weight_g")].float()
    v = sd[prefix + ("parametrizations.weight.original1" if new else "weight_v")].float()
    nrm = v.double().pow(2).sum(dim=(0, 1), keepdim=True).sqrt().float()
    return v * (g.reshape(nrm.shape) / nrm)


def pos_conv_geom(k, groups):
    """The positional conv's geometry as a float64 contraction for vocoder_ref.tapgemm_ref: a (T, H), w (H, H / groups, k) -> (T, H);
    zero padding k / 2 per side, the extra last row of an even kernel dropped (the launch computes M = T rows)."""
    def f(a, w):
        return F.conv1d(a.t()[None], w, padding=k // 2, groups=groups)[0].t()[:a.shape[0]]
    return f


# ----------------------------------------------------------------------------------------------------------- conv0 + GroupNorm
def conv0_groupnorm_ref(x, w, gn_g, gn_b, eps=1e-5, bias=None):
    """conv0 (one input channel, fp32 weights, kernel k, stride s taken from w / the caller) + GroupNorm(C groups: per channel
    over time) + erf-GELU of ONE clip, as the oracle's float64 form, and a bound E.

    x (L_out, k) are the im2col rows of the clip's wave (exact fp32 samples); w (C, k).  The kernel computes the conv in fp32
    (|dy| <= gamma(k + 1, u) sum |w||x| =: D_t per element), the channel statistics in double from those fp32 values, then
    gelu(fma(a, y, sh)) with a = g rstd, sh = b - mu a.  Moving every y_t by at most D = max_t D_t moves the mean by <= D and the
    standard deviation by <= D (the RMS of y - mu is a norm), so the normalised value moves by <= (|y - mu| / sigma + 1) D / sigma,
    times |g|; the affine coefficients and the fma are fp32: 4 u (|a y| + |sh|).  Then GELU as for a GEMM.  Returns (ref (L_out, C), E).
    """
    x = x.double()
    wd = w.double()
    y = x @ wd.t()
    if bias is not None:
        y = y + bias.double()
    Dt = gamma(x.shape[-1] + 1, U) * (x.abs() @ wd.abs().t())
    D = Dt.amax(0, keepdim=True)
    mu = y.mean(0, keepdim=True)
    var = (y - mu).pow(2).mean(0, keepdim=True)
    sigma = torch.sqrt(var + eps)
    zh = (y - mu) / sigma
    g, b = gn_g.double(), gn_b.double()
    pre = zh * g + b
    a = g / sigma
    sh = b - mu * a
    Epre = g.abs() * (zh.abs() + 1) * D / sigma + 4 * U * ((a * y).abs() + sh.abs())
    return gelu(pre), GELU_LIP * Epre + gelu_fast_err(pre)


# ----------------------------------------------------------------------------------------------------------- taps
def tap_capacities(harch, B, N, R):
    """{name: elements} of every per-op tap of the encoder (include/si_hip.h) for B clips of N samples and R transformer rows."""
    Ls = harch.feat_lengths(N)
    H, I = harch.hidden_size, harch.intermediate_size
    cap = {}
    for i, C in enumerate(harch.conv_dim):
        for nm in (f"conv{i}", f"conv{i}.ln"):
            cap[nm] = cap[nm + ".bf16"] = B * Ls[i + 1] * C
    cap["features.ln"] = cap["features.ln.bf16"] = R * harch.conv_dim[-1]
    cap["pos_conv"] = R * H
    for l in range(harch.num_hidden_layers):
        for t, w in (("h", H), ("qkv", 3 * H), ("att", H), ("ln1", H), ("ffn", I), ("ln2", H)):
            cap[f"layer{l}.{t}"] = cap[f"layer{l}.{t}.bf16"] = R * w
        cap[f"layer{l}.att_res"] = cap[f"layer{l}.ffn_res"] = R * H
    return cap


# ----------------------------------------------------------------------------------------------------------- checks
def check_f32(got, ref, E):
    """fp32 output: |got - ref| <= E elementwise.  -> dict(max, rms, worst = max |got - ref| / E, bad = count over)."""
    err = (got.double() - ref).abs()
    return dict(max=float(err.max()), rms=float(err.pow(2).mean().sqrt()), worst=float((err / E.clamp_min(1e-300)).max()),
                bad=int((err > E).sum()), n=err.numel())


def check_bf16(got, ref, E):
    """bf16 output of an fp32 value y with |y - ref| <= E: got = rne(y), so |got - ref| <= E + 1/2 ulp_bf16(|ref| + E) (the ulp
    at |y|'s binade or above).  Also counts the outputs that differ from rne(ref), the bf16 value nearest to ref.
    -> dict(max, rms, worst, bad, n, mismatch = fraction != rne(ref))."""
    got = got.double()
    err = (got - ref).abs()
    bound = E + 0.5 * ulp_bf16(ref.abs() + E)
    mism = float((got != rne_bf16(ref)).double().mean())
    return dict(max=float(err.max()), rms=float(err.pow(2).mean().sqrt()), worst=float((err / bound).max()),
                bad=int((err > bound).sum()), n=err.numel(), mismatch=mism)


def fmt(name, r):
    s = f"{name}: max err {r['max']:.3e}, rms {r['rms']:.3e}, worst err/bound {r['worst']:.3f} ({r['bad']} of {r['n']} over)"
    if "mismatch" in r:
        s += f", != rne(ref) {100 * r['mismatch']:.4f} %"
    return s
