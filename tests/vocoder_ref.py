"""Float64 references of the fp16 vocoder's kernels (the fp16 activation stream that bench.py times), op by op, each with an
explicit per-element error bound.

Every reference takes the kernel's OWN operands: the fp16 tensor the previous kernel stored (captured through the ".f16" taps
of include/si_hip.h), the weights folded as the packer folds them (`fold`: v * (g / norm) in fp32, torch._weight_norm's order)
and rounded once to fp16 (`h16`), the biases in fp32.  It returns (ref, E): the exact result in float64 and a bound on
|stored fp16 value - ref| per element, derived in the docstring from the kernel's arithmetic and fitted to no measurement.
Tensors are channels-last, one clip at a time: (rows, channels).  The last section (`tapgemm_ref`) does the same for the tap-GEMM on an
fp32 activation stream -- the fp32, bf16x3 and bf16 vocoders and the fp32 encoder's convolutions -- with fp32 outputs.

The staged operand.  Every kernel of the stream applies its leaky-ReLU to the packed fp16 halves while staging, so the product
with the slope ROUNDS TO fp16 and the slope is the fp16 constant (fp16(0.1) = 0.0999755859375, fp16(0.01) = 0.0100021362...):
    respair.hip:155, respair_wide.hip:196, reschain.hip:256 and :360, upsample.hip:102   max(h, h * (_Float16)0.1f)
    gemmcu.hip:203 (TC mode)                                                              max(h, h * (_Float16)tc_slope)
    tapgemm.hip:198-201 (a 16-bit input with pro_slope != 1)                              h > 0 ? h : h * (_Float16)slope
    vocoder_kernels.hip:189 (conv_post_mfma_kernel)                                       max(h, h * (_Float16)0.01f)
The select and the max give the same bits for every non-NaN h (0.1 h >= h exactly when h <= 0).  `lrelu16` emulates the step
bit-exactly with torch.float16 CPU arithmetic (a product of two fp16 values is exact in fp32 and is rounded once); the error
bounds start BEHIND it.  Two kernels stage differently: the tap-GEMM's fp32-input path (tapgemm.hip:213-221: conv_pre's
stretched mel) applies the slope in fp32, clamps to +-65504 and rounds -- with pro_slope = 1 that is `h16(clamp(x))`; and
conv_post_kernel (vocoder_kernels.hip:112) converts fp16 -> fp32 and applies 0.01f in fp32, unrounded (`conv_post_ref`, mfma=False).

Notation (shared with tests/encoder_ref.py): U = 2^-24, the unit roundoff of an fp32 operation; gamma(n) = n U_ACC / (1 - n U_ACC)
with U_ACC = 2^-23 bounds any order of summing n products in an fp32 MFMA accumulator.  U16 = 2^-11 is fp16's unit roundoff,
SUB16 = 2^-25 half the spacing of the fp16 subnormals (the absolute rounding error below 2^-14).  F16_MAX = 65504.

Saturation.  The fused kernels set MODE.FP16_OVFL (a conversion that overflows gives +-65504), the tap-GEMM clamps before it
rounds: either way the stored value is rne_f16(clamp(v, +-65504)) of the fp32 v.  `check_f16` applies: where |ref| - E > 65504 the
stored value must be exactly +-65504; where |ref| + E < 65504 the ordinary bound holds; in between either is accepted.  The
ResBlock intermediate t saturates the same way; the references clamp it (a clamp is 1-Lipschitz: the bound on t is unchanged).
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.encoder_ref import U, U_ACC, gamma  # noqa: F401  (re-exported: one set of constants for both reference modules)

U16 = 2.0 ** -11
SUB16 = 2.0 ** -25
F16_MAX = 65504.0
SLOPE32 = float(np.float32(0.1))                # the fp32 epilogues' 0.1f
SLOPE_POST32 = float(np.float32(0.01))          # conv_post_kernel's 0.01f
# tanhf of the device library: the OpenCL C accuracy the library is built to (tanh: <= 5 ulp), as a relative error of the result
TANH_ULPS = 5


def alpha32(nk):
    """The launchers' `1.0f / nk` as the fp32 value the kernel multiplies by."""
    return float(np.float32(1.0) / np.float32(nk))


def h16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> fp16 -> float64: the packer's rounding of a weight (round to nearest, ties to even)."""
    return x.float().to(torch.float16).double()


def ulp_f16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of the fp16 values around |x| (11 significant bits): 2^(e - 11) for |x| in [2^(e-1), 2^e), 2^-24 below 2^-14."""
    _, e = torch.frexp(x.double().abs())
    e = torch.where(x == 0, torch.full_like(e, -30), e)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 11).clamp(min=-24))


def rne_f16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest fp16 value (ties to even) in ONE rounding, as float64; no saturation."""
    x = x.double()
    return torch.round(x / ulp_f16(x)) * ulp_f16(x)


def next_f16(x: torch.Tensor, away_from: torch.Tensor) -> torch.Tensor:
    """The first fp16 value strictly beyond float64 x, on the side away from `away_from` (for the bound-rejection tests)."""
    up = x >= away_from
    q = ulp_f16(x)
    lo = torch.floor(x / q) * q
    cand = torch.where(up, lo + q, torch.where(lo < x, lo, lo - q))
    cand = torch.where(up & (cand <= x), cand + ulp_f16(cand), cand)
    return cand


def lrelu16(h: torch.Tensor, slope=0.1) -> torch.Tensor:
    """The packed-halves leaky-ReLU, bit-exact: max(h, h * fp16(slope)) in fp16 arithmetic.  h: torch.float16 -> torch.float16."""
    assert h.dtype == torch.float16
    return torch.maximum(h, h * torch.tensor(slope, dtype=torch.float32).to(torch.float16))


def lrelu(x: torch.Tensor, slope: float) -> torch.Tensor:
    return torch.where(x > 0, x, x * slope)


def fold(sd, name, round16=True, norm="packer") -> torch.Tensor:
    """The folded weight of module `name` as the packer computes it (api.hip, Packer::folded): w = v * (g / nrm) in fp32 --
    torch._weight_norm's order of operations -- then rounded once to fp16 (round16) -> float64.  The norm runs over every dim
    but 0.  The packer sums the squares in double and rounds the square root to fp32 once (norm="packer": the correctly rounded
    norm); torch sums in fp32 (norm="torch": the norm torch._weight_norm_interface returns), which on about a third of the rows is the neighbouring
    fp32 value and moves a few fp16 weights in 10^5 to their neighbour.  The kernels' operands are the packer's.  A state dict
    that already holds `.weight` is taken as is."""
    if name + ".weight" in sd:
        w = sd[name + ".weight"].float()
    else:
        g, v = sd[name + ".weight_g"].float(), sd[name + ".weight_v"].float()
        if norm == "packer":
            nrm = v.double().pow(2).sum(dim=tuple(range(1, v.dim())), keepdim=True).sqrt().float()
        else:
            nrm = torch._weight_norm_interface(v, g, 0)[1]
        w = v * (g.reshape(nrm.shape) / nrm)
    return h16(w) if round16 else w.double()


# ----------------------------------------------------------------------------------------------------------- convolutions
def _conv(a, w, dil=1):
    """a (L, Cin), w (Cout, Cin, k) float64 -> (L, Cout): the same-length convolution, zero padding dil (k - 1) / 2 per side."""
    k = w.shape[2]
    return F.conv1d(a.t()[None], w, dilation=dil, padding=dil * (k - 1) // 2)[0].t()


def _conv_sum(a, w, b, dil=1):
    """z = conv(a, w) + b and S = sum |a||w| + |b| (the magnitude the accumulation error scales with)."""
    z = _conv(a, w, dil) + b.double()
    S = _conv(a.abs(), w.abs(), dil) + b.double().abs()
    return z, S


def _store16(v, Ev):
    """Bound behind the store: |rne_f16(v~) - v| <= Ev + U16 |v~| + SUB16 with |v~| <= |v| + Ev."""
    return Ev + U16 * (v.abs() + Ev) + SUB16


def tapconv_ref(a, w, b, dil=1, out_slope=1.0):
    """A same-length tap convolution whose fp32 result is stored as fp16 (conv_pre on the tap-GEMM): out = fp16(lrelu(conv(a, w) + b,
    out_slope)).  a (L, Cin): the staged operand as float64 (conv_pre: h16(clamp(x)) of the fp32 mel rows); w (Cout, Cin, k) float64
    (already rounded); b fp32.

    K = k Cin fp16 x fp16 products (exact in fp32) and the bias are summed in fp32: |z~ - z| <= gamma(K + 1) S, S = sum |a||w| + |b|.
    out_slope != 1 (the consumer's activation stored by the producer, tapgemm.hip:541): one fp32 multiply, relative U, and
    |lrelu'| <= 1 carries the sum error.  The store rounds once: E = gamma(K + 1) S [+ U |ref|] + U16 |ref| + SUB16 (`_store16`
    also carries the second-order U16 Ev)."""
    K = w.shape[1] * w.shape[2]
    z, S = _conv_sum(a, w, b, dil)
    Ev = gamma(K + 1) * S
    if out_slope != 1.0:
        z = lrelu(z, out_slope)
        Ev = Ev + U * z.abs()
    return z, _store16(z, Ev)


def upsample_ref(a, w, b, u, out_slope=1.0):
    """ConvTranspose1d(Cin -> Cout, k, stride u, padding (k - u) / 2) on the staged operand a (Lin, Cin) -> (u Lin, Cout).
    w (Cin, Cout, k) float64 (rounded), b fp32.  The kernels run it as u phases of a ceil(k / u)-tap convolution (output row
    u m + p - pad reads input rows m, m - 1, ...; rows outside the clip are zero; the pad first and last rows are cropped), which
    is the same sum: K = ceil(k / u) Cin products and the bias per output.  E = gamma(K + 1) S + U16 |ref| + SUB16, S = sum |a||w| + |b|.
    upsample.hip, gemmcu.hip's TC kernels (accumulators + bias in fp32, one rounding on store, FP16_OVFL) and the tap-GEMM share it."""
    k = w.shape[2]
    pad = (k - u) // 2
    K = -(-k // u) * w.shape[0]
    z = F.conv_transpose1d(a.t()[None], w, stride=u, padding=pad)[0].t() + b.double()
    S = F.conv_transpose1d(a.abs().t()[None], w.abs(), stride=u, padding=pad)[0].t() + b.double().abs()
    Ev = gamma(K + 1) * S
    if out_slope != 1.0:
        z = lrelu(z, out_slope)
        Ev = Ev + U * z.abs()
    return z, _store16(z, Ev)


def pair_ref(a, y, w1, b1, w2, b2, dil, alpha=1.0, prev=None, out_slope=1.0, round_t=False, t_slope=SLOPE32):
    """One ResBlock1 pair: out = fp16(lrelu_os(((conv2(t) + b2 + y) * alpha) + prev)), t = fp16(lrelu(conv1(a) + b1, 0.1f)), t = 0
    outside the clip (conv2's zero padding applies to t: respair.hip's `inside` factor).  a (L, C): the staged operand
    lrelu16(y) as float64; y (L, C): the raw residual; w1, w2 (C, C, k) float64 (rounded); alpha the fp32 factor; prev (L, C) the
    running MRF sum read back as fp16 (accumulate) or None; out_slope the wide kernel's consumer activation (0.1f) or 1.

    The reference keeps t UNROUNDED (round_t and t_slope are for the CPU self-tests).  Bound, with K = k C:
      z1 = conv1(a) + b1 (accumulators started from b1): |z1~ - z1| <= E1 = gamma(K + 1) S1, S1 = sum |a||w1| + |b1|
      t  = lrelu(z1, 0.1f): |lrelu'| <= 1, one fp32 multiply (relative U), clamp (1-Lipschitz), one fp16 rounding:
           dt = E1 + (U + U16) |t| + SUB16
      z2 = conv2(t) + b2:  Ez = sum |w2| dt + gamma(K + 1) (sum |w2| (|t| + dt) + |b2|)
      v  = (z2 + y) * alpha + prev, three fp32 operations (an fma contraction has fewer): with A = alpha (|z2| + Ez + |y|) + |prev|,
           Ev = alpha Ez + gamma(3, U) A;  out_slope != 1 adds one multiply: + U |v|
      store: E = Ev + U16 (|v| + Ev) + SUB16."""
    C, _, k = w1.shape
    K = k * C
    z1, S1 = _conv_sum(a, w1, b1, dil)
    t = lrelu(z1, t_slope).clamp(-F16_MAX, F16_MAX)
    dt = gamma(K + 1) * S1 + (U + U16) * t.abs() + SUB16
    if round_t:
        t = rne_f16(t)
    z2 = _conv(t, w2) + b2.double()
    Ez = _conv(dt, w2.abs()) + gamma(K + 1) * (_conv(t.abs() + dt, w2.abs()) + b2.double().abs())
    return _residual_out(z2, Ez, y, alpha, prev, out_slope)


def _residual_out(z, Ez, y, alpha, prev, out_slope):
    v = (z + y) * alpha
    A = alpha * (z.abs() + Ez + y.abs())
    if prev is not None:
        v = v + prev
        A = A + prev.abs()
    Ev = alpha * Ez + gamma(3, U) * A
    if out_slope != 1.0:
        v = lrelu(v, out_slope)
        Ev = Ev + U * v.abs()
    return v, _store16(v, Ev)


def rb2_ref(a, y, w, b, dil, alpha=1.0, prev=None, out_slope=1.0):
    """One ResBlock2 step (v3 architecture) on the tap-GEMM with the residual epilogue (tapgemm.hip:537-541):
    out = fp16(lrelu_os((conv(a) + b + y) * alpha + prev)).  Ez = gamma(K + 1) S, then pair_ref's last two steps."""
    K = w.shape[1] * w.shape[2]
    z, S = _conv_sum(a, w, b, dil)
    return _residual_out(z, gamma(K + 1) * S, y, alpha, prev, out_slope)


def chain_ref(y, pairs, alpha=1.0, prev=None, staged=None, round_x=True, t_slope=SLOPE32):
    """A whole ResBlock1 (three pairs) composed from pair_ref on the reference's own x_i, each rounded to fp16 as reschain.hip keeps
    it in LDS (round_x).  Returns the last pair's (ref, E) only: E bounds the LAST pair given x_2 and carries no flip term.

    The GPU test does not bound the chain kernel through this composition: the internal x_1, x_2 cannot be observed, and a
    composed bound would have to carry a possible flip of each x_i (U16 |x_i| through the next pair's sum |w1| sum |w2|), three
    times looser than the pair bound.  Instead the pairs run one by one (SI_VOC_CHAIN=0), every x_i is tapped and checked against
    pair_ref on its own tapped input, and the chain kernel's output is checked against pair_ref on the TAPPED x_2 (and for
    equality with the pairs' output: the kernel is specified to do the same arithmetic in the same order).  This function pins
    the composition to the oracle on the CPU and serves the chain on inputs where no pairs run exists."""
    staged = staged or (lambda x: lrelu16(x.to(torch.float16)).double())
    x = y
    out = None
    for n, (w1, b1, w2, b2, dil) in enumerate(pairs):
        last = n == len(pairs) - 1
        out = pair_ref(staged(x), x, w1, b1, w2, b2, dil, alpha if last else 1.0, prev if last else None, t_slope=t_slope)
        x = rne_f16(out[0].clamp(-F16_MAX, F16_MAX)) if round_x else out[0]
    return out


def conv_post_ref(x, w, b, mfma, round_w=True, slope=SLOPE_POST32):
    """leaky_relu(0.01) -> Conv1d(C -> 1, k = 7, pad 3) -> tanh, fp32 out.  x (L, C) torch.float16: the stage's stored tensor;
    w (1, C, 7) fp32 folded; b (1,) fp32.  Returns (ref (L,), E).

    mfma (conv_post_mfma_kernel, C = 32): the operand is lrelu16(x, 0.01) bit-exact, the weights are rounded to fp16 IN THE KERNEL
    (vocoder_kernels.hip:160), the 224 products are summed from 0 in the MFMA accumulator and the bias is added in fp32:
        |z~ - z| <= Es = gamma(K + 1) S,  S = sum |a||w| + |b|.
    not mfma (conv_post_kernel): a = lrelu(float(x), 0.01f) in fp32 (relative U per element: da = U |a|), fp32 weights, an fmaf
    chain started from the bias:  Es = sum |w| da + gamma(K + 1) S.
    |tanh'| <= 1 carries Es; tanhf itself is within TANH_ULPS ulp of the exact tanh of its argument, i.e. a relative
    TANH_ULPS 2^-23:  E = Es + TANH_ULPS 2^-23 |ref| + 2^-149.
    The output is fp32, so no store rounding dominates E as it does for the fp16 tensors: E is the worst-case growth of K + 1 fp32
    additions (gamma(225) = 2.7e-5 of S), two orders above what a sum of 224 terms does in practice.  This bound catches a wrong
    row, tap, slope or weight form; it cannot catch a one-ulp mistake (measured err / E <= 0.005 on MI355X)."""
    K = w.shape[1] * w.shape[2]
    if mfma:
        a = lrelu16(x, 0.01).double()
        wd = h16(w) if round_w else w.double()
        da = torch.zeros_like(a)
    else:
        a = lrelu(x.double(), slope)
        wd = w.double()
        da = U * a.abs()
    z, S = _conv_sum(a, wd, b)
    Es = _conv(da, wd.abs()) + gamma(K + 1) * S
    ref = torch.tanh(z)
    return ref[:, 0], (Es + TANH_ULPS * 2.0 ** -23 * ref.abs() + 2.0 ** -149)[:, 0]


# ------------------------------------------------------------------------------- the tap-GEMM on an fp32 activation stream
# (tapgemm.hip with fp32 inputs: the whole fp32 and bf16x3 vocoder, the bf16 vocoder without operand-ready activations, the
# fp32 encoder's Linear layers and convolutions)
FTZ = 2.0 ** -126                               # the smallest normal fp32: what one flushed product or partial sum can lose


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest, ties to even: v_cvt_pk_bf16_f32 and the packer's h_f2bf) -> fp32."""
    return x.float().to(torch.bfloat16).float()


def lrelu32(x: torch.Tensor, slope: float) -> torch.Tensor:
    """tapgemm.hip:215, bit-exact: v > 0 ? v : v * slope with the fp32 slope, one fp32 rounding of the product.  slope = 1: x."""
    x = x.float()
    return x if slope == 1.0 else torch.where(x > 0, x, x * torch.tensor(slope, dtype=torch.float32))


def split_bf16(v: torch.Tensor):
    """The bf16x3 split of an fp32 tensor, bit-exact: hi = bf16(v), lo = bf16(v - hi), the subtraction in fp32 (it is exact: hi
    shares v's leading bits).  Activations: tapgemm.hip:225-229; weights: Packer::put in api.hip -- `hi = h_f2bf(v)` into the w
    plane, `h_f2bf(v - h_bf2f(hi))` into the w_lo plane, h_f2bf being round to nearest, ties to even.  -> (hi, lo) as float64."""
    v = v.float()
    hi = bf16r(v)
    lo = bf16r(v - hi)
    return hi.double(), lo.double()


TapRef = collections.namedtuple("TapRef", "ref E exact E_exact")


def tapgemm_ref(x, w, b, math, contract, K, slope=1.0, act=None, res=None, alpha=1.0, prev=None, drop=()):
    """One tap-GEMM launch with an fp32 output, on the kernel's own fp32 input:
        out = ((act(sum_K pro(x) w + b) + res) * alpha) + prev,    pro(x) = lrelu32(x, slope) staged in the arithmetic `math`.
    x: the fp32 tensor the kernel read; w: the fp32 (folded) weight the packer was given; b fp32 or None; contract(a, w) the
    layer's geometry as a float64 function, linear in both arguments (`conv_geom`, `tconv_geom`, a matmul, a grouped conv), applied to
    operand planes and to their magnitudes; K products per output; res / prev fp32 tensors of the output's shape (residual,
    accumulate); alpha the fp32 scale.  -> TapRef(ref, E, exact, E_exact).

    The operand planes the MFMAs multiply (everything before them is emulated bit-exactly, the bounds start behind it):
      "f32"     v = lrelu32(x) and w themselves.  v_mfma_f32_32x32x2_f32 either rounds each product to fp32 before adding it
                (relative U) or fuses it; the accumulation of K products and the bias add (epilogue: acc + bias, one rounding) are K + 1
                fp32 additions in whatever order: |z~ - z| <= gamma(K + 1) S + U (1 + gamma(K + 1)) S, S = sum |v||w| + |b|.
      "bf16"    bf16(v) (the slope applied in fp32 BEFORE the rounding, tapgemm.hip:215 then :225) and bf16(w), rounded once.
                Products of two bf16 values are exact in fp32: |z~ - z| <= gamma(K + 1) S.
      "bf16x3"  (v_hi, v_lo), (w_hi, w_lo) of `split_bf16`; the kernel sums v_lo w_hi + v_hi w_lo + v_hi w_hi per K step, each
                product exact: ref is THAT sum in float64 and |z~ - z| <= gamma(3 K + 1) S, S = the sum of the three
                magnitude contractions + |b|.  `exact` is the contraction of the fp32 v and w themselves; with v = v_hi + v_lo + r_v,
                w = w_hi + w_lo + r_w:   v w - (three terms) = v_lo w_lo + r_v w + (v_hi + v_lo) r_w, so
                E_exact = E + epilogue-scaled sum (|v_lo||w_lo| + |r_v||w| + |v_hi + v_lo||r_w|), all computed, nothing
                estimated (bf16 keeps 8 significant bits: |v_lo| <= 2^-8 (1 + 2^-8) |v|, |r_v| <= 2^-16 |v|, likewise for w, so the sum is
                <= 3.1 * 2^-16 sum |v||w| in the worst case of every rounding at half an ulp: what the "fp32-equivalent" claim amounts to).
      "f64"     lrelu(x, slope) and w in float64, E = 0: the operation itself, for pinning the references to the oracle.
    Each term may also lose FTZ to a flushed subnormal: + (terms + 1) FTZ.
    Epilogue (tapgemm.hip:598-602, fp32 VALU, relative U each): act = "gelu": |GELU'| <= GELU_LIP carries the sum error and erff
    adds gelu_fast_err; then with n of {+ res, * alpha (alpha != 1), + prev} present and A = alpha (|z| + Ez + |res|) + |prev|:
    E = alpha Ez + gamma(n, U) A.  A fused multiply-add of the compiler's has fewer roundings.
    drop: names of product planes left out ("lo*hi", "hi*lo", "hi*hi") -- the CPU self-tests' emulation of a kernel that forgets one."""
    from tests.encoder_ref import GELU_LIP, gelu, gelu_fast_err
    wf = w.float()
    if math == "f64":
        planes, coef, terms = [("v*w", lrelu(x.double(), slope), w.double())], 0.0, 0
    else:
        v = lrelu32(x, slope)
        if math == "f32":
            planes = [("v*w", v.double(), wf.double())]
            coef, terms = gamma(K + 1) + U * (1 + gamma(K + 1)), K
        elif math == "bf16":
            planes = [("hi*hi", bf16r(v).double(), bf16r(wf).double())]
            coef, terms = gamma(K + 1), K
        elif math == "bf16x3":
            (vh, vl), (wh, wl) = split_bf16(v), split_bf16(wf)
            planes = [("lo*hi", vl, wh), ("hi*lo", vh, wl), ("hi*hi", vh, wh)]
            coef, terms = gamma(3 * K + 1), 3 * K
        else:
            raise ValueError(math)
    planes = [p for p in planes if p[0] not in drop]
    z = sum(contract(a, ww) for _, a, ww in planes)
    S = sum(contract(a.abs(), ww.abs()) for _, a, ww in planes)
    if b is not None:
        z = z + b.double()
        S = S + b.double().abs()
    Ez = coef * S + (terms + 1) * FTZ if math != "f64" else torch.zeros_like(z)
    zx = Dx = None
    if math == "bf16x3":
        vd, wd = v.double(), wf.double()
        zx = contract(vd, wd) + (b.double() if b is not None else 0.0)
        Dx = contract(vl.abs(), wl.abs()) + contract((vd - vh - vl).abs(), wd.abs()) + contract((vh + vl).abs(), (wd - wh - wl).abs())

    def epilogue(z, Ez):
        if act == "gelu":
            Ez = GELU_LIP * Ez + (gelu_fast_err(z) if math != "f64" else 0.0)
            z = gelu(z)
        elif act is not None:
            raise ValueError(act)
        n = (res is not None) + (alpha != 1.0) + (prev is not None)
        A = z.abs() + Ez
        if res is not None:
            z = z + res.double()
            A = A + res.double().abs()
        z, A, Ez = z * alpha, A * abs(alpha), Ez * abs(alpha)
        if prev is not None:
            z = z + prev.double()
            A = A + prev.double().abs()
        return z, (Ez + gamma(n, U) * A if (n and math != "f64") else Ez)

    ref, E = epilogue(z, Ez)
    if zx is None:
        return TapRef(ref, E, ref if math != "bf16" else None, E if math != "bf16" else None)
    exact, Ex = epilogue(zx, Ez + Dx)
    return TapRef(ref, E, exact, Ex)


def conv_geom(dil=1, shift=0):
    """The same-length convolution of `_conv` (zero padding dil (k - 1) / 2 per side) as a contract(a (L, Cin), w (Cout, Cin, k)).
    shift: every tap reads `shift` rows further down (the self-tests' shifted-tap mistake; 0 is the layer)."""
    def f(a, w):
        if shift:
            a = torch.cat([a[shift:], a.new_zeros(shift, a.shape[1])])
        return _conv(a, w, dil)
    return f


def tconv_geom(u):
    """ConvTranspose1d(k, stride u, padding (k - u) / 2) as a contract(a (Lin, Cin), w (Cin, Cout, k)) -> (u Lin, Cout): the sum the
    kernel forms as u phases of a ceil(k / u)-tap convolution with dil = -1 (see `upsample_ref`); K = ceil(k / u) Cin."""
    def f(a, w):
        return F.conv_transpose1d(a.t()[None], w, stride=u, padding=(w.shape[2] - u) // 2)[0].t()
    return f


# ----------------------------------------------------------------------------------------------------------- checking
def real_channels(t, C, what="tensor"):
    """A tensor of the fp16 stream as its C real channels (last dim).  A stage narrower than 32 channels is carried at 32 (api.hip,
    stage_channels): the weights and biases of the extra channels are zero, so every stored value there is EXACTLY zero (a sum of
    exact zero products, + 0 bias, + a zero residual), and the real channels see sixteen more zero products, which round nothing:
    the references of the real width and their bounds apply unchanged.  Any non-zero bit pattern in the padding is a failure."""
    assert t.shape[-1] >= C, (what, tuple(t.shape), C)
    assert not bool((t[..., C:] != 0).any()), f"{what}: the padded channels {C}..{t.shape[-1] - 1} are not exactly zero"
    return t[..., :C]


def check_f16(got, ref, E):
    """A stored fp16 tensor against (ref, E) with the saturation rule of the module docstring, over ALL elements.
    -> dict(bad, ratio (err / E per element, 0 where the saturation rule decided), worst index)."""
    got, ref, E = got.double(), ref.double(), E.double()
    err = (got - ref).abs()
    must_sat = ref.abs() - E > F16_MAX
    may_sat = (~must_sat) & (ref.abs() + E >= F16_MAX)
    sat_ok = got == torch.sign(ref) * F16_MAX
    ok = torch.where(must_sat, sat_ok, (err <= E) | (may_sat & sat_ok))
    ratio = torch.where(must_sat | (may_sat & sat_ok), torch.zeros_like(err), err / E)
    return dict(bad=int((~ok).sum()), ok=ok, ratio=ratio, err=err, saturated=int((must_sat | (may_sat & sat_ok)).sum()),
                finite=bool(torch.isfinite(got).all()))


def check_f32(got, ref, E):
    got, ref, E = got.double(), ref.double(), E.double()
    err = (got - ref).abs()
    ok = err <= E
    return dict(bad=int((~ok).sum()), ok=ok, ratio=err / E, err=err, saturated=0, finite=bool(torch.isfinite(got).all()))


def seam_distance(L, stored):
    """Per row of a clip of L rows: rows to the nearest tile seam (a seam lies between rows j * stored - 1 and j * stored, j >= 1;
    both of those rows are at distance 0; L when the clip is one tile) and to the nearest clip edge."""
    r = torch.arange(L)
    edge = torch.minimum(r, L - 1 - r)
    if not stored or stored >= L:
        return torch.full((L,), L), edge
    b = torch.arange(stored, L, stored)
    d = r[:, None] - b[None, :]
    return torch.where(d >= 0, d, -d - 1).min(dim=1).values, edge


def report(tag, kernel, clip, r, L, stored, halo):
    """One line per check: max err / E over the rows within `halo` of a tile seam or clip edge and over the rest; on a failure the
    worst element with op, kernel, clip, row, channel, distances and ratio."""
    ratio = r["ratio"].reshape(L, -1)
    seam, edge = seam_distance(L, stored)
    near = (seam <= halo) | (edge <= halo)
    row_max = ratio.max(dim=1).values
    m_near = float(row_max[near].max()) if bool(near.any()) else 0.0
    m_rest = float(row_max[~near].max()) if bool((~near).any()) else 0.0
    line = f"{tag} [{kernel}] clip {clip} L={L}: max err/E seam+edge rows {m_near:.3f}, interior {m_rest:.3f}, saturated {r['saturated']}"
    if r["bad"] or not r["finite"]:
        okm = r["ok"].reshape(L, -1)
        bad_ratio = torch.where(okm, torch.zeros_like(ratio), torch.where(ratio > 0, ratio, torch.full_like(ratio, math.inf)))
        row = int(bad_ratio.max(dim=1).values.argmax())
        ch = int(bad_ratio[row].argmax())
        line += (f" -- FAILED: {r['bad']} elements; worst at row {row}, channel {ch}, {'no tile seam in this clip' if int(seam[row]) >= L else str(int(seam[row])) + ' rows from a tile seam'}, "
                 f"{int(edge[row])} from the clip edge, err/E {float(bad_ratio[row, ch]):.3f} (err {float(r['err'].reshape(L, -1)[row, ch]):.3e})")
    return line, m_near, m_rest
