"""The log-mel front-end kernel by kernel against float64 (tests/frontend_ref.py): si_mel_frontend, _varlen and _spans with the taps
"mel_peak", "mel_frames" and "mel_spec" captured, every stage checked on its own captured input with its derived per-element bound --
the peak bit for bit, the folded frames (exact zeros where the layout or a mask says zero), the two DFT GEMMs, and the log-mel as an
interval that needs no near-clamp exclusions -- on the shapes of frontend_ref.cases(): the frame-count boundaries, the peak kernel's
16-byte and scalar loops, five and sixteen spans within one frame's reach (FeFrameSpans' walked loop), spans at the reflection points,
ragged rows filled with 1e30 past each clip, a fully masked, a silent and a subnormal-peak clip, and a misaligned base pointer.
Each case asserts the kernel families that ran.  The last test prints the largest err / E per stage, edge and interior frames apart."""
import numpy as np
import pytest
import torch

from speech_inpainting_amd.arch import HubertArch, VocoderArch
from tests import frontend_ref as FR
from tests.harness import RatioSummary, tapped_run

pytestmark = pytest.mark.gpu

SUMMARY = RatioSummary()
CASES = {c.name: c for c in FR.cases()}


@pytest.fixture(scope="module")
def ctx():
    from speech_inpainting_amd import native
    c = native.NativeContext(native.make_desc(HubertArch.tiny(), VocoderArch.tiny(), 10), torch.device("cuda:0"))
    yield c
    c.close()


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def run(ctx, case, tapped=True, offset=0, entry=None):
    """One batch through the entry point `entry` (default: the case's own) -> (peak, frames, spec, mel as numpy, {kernel: launches}).
    offset: the clips start that many floats into a larger buffer (a contiguous view whose base pointer is not 16-byte aligned)."""
    from speech_inpainting_amd.native import SpanTable
    entry = entry or case.entry
    B, Ns = case.wave.shape
    Tm = FR.mel_frames(Ns)
    buf = torch.zeros(B * Ns + offset, dtype=torch.float32, device="cuda")
    w = buf[offset:].view(B, Ns)
    w.copy_(torch.from_numpy(case.wave))
    assert w.is_contiguous() and (w.data_ptr() % 16 != 0) == bool(offset % 4)
    cap = {"mel_frames": B * Tm * FR.FRAME, "mel_spec": B * Tm * FR.LDSPEC}
    if case.normalize:
        cap["mel_peak"] = B
    spans = case.spans if case.spans is not None else [[] for _ in range(B)]
    ms = me = None
    if case.spans is not None and entry != "spans":
        assert all(len(s) <= 1 for s in spans)
        ms = _i32(s[0][0] if s else 0 for s in spans)
        me = _i32(s[0][0] + s[0][1] if s else 0 for s in spans)

    def forward():
        if entry == "spans":
            return ctx.mel_frontend_spans(w, SpanTable(spans, torch.device("cuda:0")), normalize=case.normalize, sample_len=case.lens)
        if entry == "varlen":
            return ctx.mel_frontend_varlen(w, case.lens, ms, me, normalize=case.normalize)
        assert case.lens is None
        return ctx.mel_frontend(w, ms, me, normalize=case.normalize)

    taps, mel, prof = tapped_run(ctx, cap if tapped else {}, forward, require_all=True, max_launches=64)
    taps = {k: t.numpy() for k, t in taps.items()}
    peak = taps.get("mel_peak")
    frames = taps["mel_frames"].reshape(B, Tm, FR.FRAME) if tapped else None
    spec = taps["mel_spec"].reshape(B, Tm, FR.LDSPEC) if tapped else None
    return peak, frames, spec, mel.cpu().numpy(), prof


def expected_kernels(case, entry=None):
    """The profile families of one call: the table kernels only through si_mel_frontend_spans, the peak only with normalize, two
    launches of the exact-fp32 tap-GEMM, one projection."""
    table = (entry or case.entry) == "spans"
    names = {"mel_frames_spans" if table else "mel_frames": 1, "mel_project": 1}
    if case.normalize:
        names["wave_peak_spans" if table else "wave_peak"] = 1
    return names


def assert_kernels(prof, case, entry=None):
    gemm = {k: v for k, v in prof.items() if k.startswith("tapgemm_")}
    rest = {k: v for k, v in prof.items() if not k.startswith("tapgemm_")}
    assert rest == expected_kernels(case, entry), (case.name, prof)
    assert gemm and all(k.startswith("tapgemm_f32_") for k in gemm) and sum(gemm.values()) == 2, (case.name, prof)


def own(case, b):
    """(samples, frames) of clip b."""
    N = case.wave.shape[1] if case.lens is None else int(case.lens[b])
    return N, FR.mel_frames(N)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def spec_cols(s):
    """A spec tap without its pad columns 513 .. 515 and 1029 .. 1031."""
    return np.concatenate([s[..., :FR.NBIN], s[..., FR.IMOFF:FR.IMOFF + FR.NBIN]], axis=-1)


def check(case, peak, frames, spec, mel, tag=None):
    res = FR.check_batch(case, peak, frames, spec, mel)
    for stage, r in res.items():
        print(f"{tag or case.name} {stage}: {r['bad']} over, max err/E edge frames {r['edge']:.6f}, interior {r['interior']:.6f}")
        SUMMARY.note(stage, r["edge"], r["interior"])
    assert np.isfinite(mel).all()
    assert all(r["bad"] == 0 for r in res.values()), {k: r["bad"] for k, r in res.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_against_float64(ctx, name):
    case = CASES[name]
    peak, frames, spec, mel, prof = run(ctx, case)
    assert_kernels(prof, case)
    check(case, peak, frames, spec, mel)


@pytest.mark.parametrize("name", ["single-1282-norm", "varlen-1282-norm", "single-400-norm"])
def test_one_span_per_clip_through_the_table_is_bit_identical(ctx, name):
    """The table kernels given one span per clip compute what the single-span kernels compute: peak, frames, spec and log-mel."""
    case = CASES[name]
    a = run(ctx, case)
    b = run(ctx, case, entry="spans")
    assert_kernels(a[4], case)
    assert_kernels(b[4], case, "spans")
    assert same_bits(a[0], b[0]) and same_bits(a[3], b[3])
    for c in range(case.wave.shape[0]):
        tm = own(case, c)[1]
        assert same_bits(a[1][c, :tm], b[1][c, :tm]) and same_bits(spec_cols(a[2][c, :tm]), spec_cols(b[2][c, :tm])), (name, c)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.lens is not None])
def test_ragged_clip_equals_the_clip_alone(ctx, name):
    """Every clip of a ragged batch, its row filled with 1e30 past its length, against the same clip run alone at its own length: peak,
    its own frames and spec rows and its log-mel bit for bit; the log-mel past its own frames exactly zero.  Captured frame rows past
    tm_len[b] are not written and are ignored."""
    case = CASES[name]
    peak, frames, spec, mel, _ = run(ctx, case)
    for b in range(case.wave.shape[0]):
        N, tm = own(case, b)
        alone = FR.Case(f"{name}[{b}]", "spans" if case.entry == "spans" else "single", np.ascontiguousarray(case.wave[b:b + 1, :N]), None,
                        None if case.spans is None else [case.spans[b]], case.normalize)
        p1, f1, s1, m1, prof = run(ctx, alone)
        assert_kernels(prof, alone)
        assert peak is None or same_bits(peak[b:b + 1], p1), (name, b)
        assert same_bits(frames[b, :tm], f1[0]) and same_bits(spec_cols(spec[b, :tm]), spec_cols(s1[0])), (name, b)
        assert same_bits(mel[b, :, :tm], m1[0]) and not mel[b, :, tm:].any(), (name, b)


@pytest.mark.parametrize("name", ["single-4100-norm", "single-4100-norm-nomask", "varlen-4100-norm", "spans-a-norm"])
def test_base_pointer_offset_by_one_float(ctx, name):
    """A contiguous view one float into a larger buffer: no clip of the batch starts 16-byte aligned, so the peak kernel takes its scalar
    loop for every sample (rows of 4100 would otherwise take the 16-byte loads); every stage within its bound and every value the bits
    of the aligned run."""
    case = CASES[name]
    a = run(ctx, case)
    b = run(ctx, case, offset=1)
    assert_kernels(b[4], case)
    check(case, *b[:4], tag=name + "+1float")
    assert same_bits(a[0], b[0]) and same_bits(a[3], b[3])
    for c in range(case.wave.shape[0]):
        tm = own(case, c)[1]
        assert same_bits(a[1][c, :tm], b[1][c, :tm]) and same_bits(spec_cols(a[2][c, :tm]), spec_cols(b[2][c, :tm])), (name, c)


def test_subnormal_peak_leaves_the_clip_unscaled(ctx):
    """The clip whose peak is 1e-39 (below the smallest normal float) comes out unscaled, as R.peak_normalize_095 leaves it: the captured
    peak is that subnormal, bit for bit, and the frames are the clip times 0.95 times the window, not zero and not divided."""
    case = CASES["special-1282-norm"]
    peak, frames, spec, mel, _ = run(ctx, case)
    x = case.wave[2]
    assert same_bits(peak[2:3], np.array([FR.peak_ref(x, len(x), [])])) and 0 < float(peak[2]) < FR.TINY
    r = FR.check_frames(frames[2], FR.frames_ref(x, len(x), [], peak[2], True))
    print(f"subnormal-peak clip: frames max err/E {r['ratio'].max():.6f}, largest |frame| {np.abs(frames[2]).max():.3e}")
    assert r["bad"] == 0 and np.abs(frames[2]).max() > 0
    assert peak[0] == 0 and peak[1] == 0 and not frames[0].any() and not frames[1].any()        # fully masked, silent
    assert same_bits(mel[0], mel[1])


@pytest.mark.parametrize("name", ["single-1282-norm", "single-1282-raw-nomask", "varlen-1282-norm", "varlen-1282-raw-nomask", "spans-a-norm",
                                  "spans-a-raw", "spans-ragged-1282-norm"])
def test_taps_change_no_value_and_no_launch(ctx, name):
    """All three entry points, normalize on and off: with and without captures registered the log-mel is bit-identical and the same
    kernels run the same number of times."""
    case = CASES[name]
    _, _, _, plain, prof0 = run(ctx, case, tapped=False)
    _, _, _, tapped, prof1 = run(ctx, case, tapped=True)
    assert same_bits(plain, tapped) and prof0 == prof1, (name, prof0, prof1)
    assert_kernels(prof0, case)


def test_coverage_of_frame_and_span_situations():
    """From the shapes alone: the table kernels see frames with 0, 1, 2, 3+ and 16 spans in reach (FeFrameSpans keeps two in registers
    and walks the rest), and frames without, with head, with tail and with double reflection all occur."""
    cov = FR.coverage()
    assert {0, 1, 2, 16} <= cov["spans"] and any(3 <= n < 16 for n in cov["spans"]), cov
    assert cov["reflect"] == {"none", "head", "tail", "both"}, cov
    entries = {(c.entry, c.normalize, c.lens is not None) for c in FR.cases()}
    assert {("single", True, False), ("single", False, False), ("varlen", True, True), ("varlen", False, True), ("spans", True, False),
            ("spans", False, False), ("spans", True, True)} <= entries


def test_zz_summary_of_ratios():
    """(last in the file) the largest err / E per stage over every check above: edge frames (reflecting, or with a span in reach) |
    interior frames.  The log-mel's figure is the distance from the middle of its interval in half-widths."""
    SUMMARY.report("front-end {key}: max err/E edge frames {near:.6f} | interior frames {rest:.6f}", keys=("frames", "spec", "logmel"))
