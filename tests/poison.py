"""Stale scratch as a test input: fill patterns for the caller-owned workspaces, poisoned `torch.empty`, the three-fill
comparison, and the closed lists of kernel families with and without scratch.
A plain module, imported by name: it registers no fixture and no plugin, and importing it needs no GPU."""
import contextlib

import torch

# Applied byte-wise.  0x00 is the baseline; 0xFF reads as NaN in fp32 / fp16 / bf16 and as -1 in int32; 0x7B is finite and huge
# (fp32 and bf16 ~ 1.3e36, fp16 61280, int32 2071690107), so a stale read that goes through fmaxf / fminf / a clamp -- which launder
# NaN -- still changes bits.
FILLS = (0x00, 0xFF, 0x7B)

# The profile family names (the names si_prof_begin is given).  A family has scratch if it reads or writes a caller-owned workspace,
# library-owned scratch, or a buffer recycled inside a pass.  The kernels that build their name at run time are listed by the prefix
# their source file gives them; tests/test_poison_host.py holds every launcher of csrc/*.hip to exactly one of the two lists.
SCRATCH_FAMILIES = (
    # encoder pass (hubert_run's carve)
    "wave_stats", "wave_stats_spans", "conv0_apply", "conv0_apply_spans", "conv0_lagsums", "conv0_lagsums_spans", "conv0_gn_affine",
    "pack_rows", "unpack_rows", "layernorm", "attention_bf16", "attention_f32", "tapgemm", "lingemm", "gemmcu", "posconv",
    # generator pass (hifigan_run's carve, one set of buffers for every chunk)
    "extend_mel", "respair", "reschain_f16_c32", "reschain_f16_c32_acc", "upsample", "conv_post",
    # mel front-end (mel_run's carve)
    "wave_peak", "wave_peak_spans", "mel_frames", "mel_frames_spans", "mel_project",
    # F0 encoder, layer by layer (three rotating workspace buffers)
    "f0enc_conv1d",
    # library-owned: ctx->km_cnorm and ctx->det_scratch
    "kmeans_assign", "detect_peak", "detect_peak_final", "detect_dead", "detect_bits", "detect_bits_ch", "detect_carry", "detect_count",
    "detect_offsets", "detect_emit",
)
NO_SCRATCH_FAMILIES = (
    "mel_metrics", "sisdr", "cut_rate", "cut_rate_ch", "patch_rate", "patch_rate_ch", "codebook_splice", "codebook_splice_spans",
    "codebook_gather", "codebook_gather_spans", "codebook_metrics", "codebook_metrics_spans", "code_splice", "unit_frontend",
    "f0enc_fused",                                           # the track's activations live in LDS: input and output tensors only
    "resample_poly", "resample_sinc", "pcm16", "gather_windows", "patch_compose", "cut_clips", "patch_regions",
)
PREFIX_FAMILIES = ("tapgemm", "lingemm", "gemmcu", "respair", "posconv", "upsample")   # named at run time: "<prefix>_<math>_<tile or width>"


def family_of(name):
    """The entry of the two lists a profiled launch name belongs to: itself, or the prefix of a name built at run time; None if neither."""
    if name in SCRATCH_FAMILIES or name in NO_SCRATCH_FAMILIES:
        return name
    for p in PREFIX_FAMILIES:
        if name.startswith(p + "_"):
            return p
    return None


def fill_value(byte, dtype):
    """What a buffer filled byte-wise with `byte` reads as in `dtype` (one element, on the CPU)."""
    return torch.full((8,), int(byte), dtype=torch.uint8).view(dtype)[0]


def poison_scratch(ctx, byte):
    """Fill the context's caller-owned workspaces -- the encoder / generator one, the mel front-end's and the one it replaced, where they
    exist -- with `byte`, on the current stream."""
    for name in ("_ws", "_ws_mel", "_ws_mel_old"):
        t = getattr(ctx, name, None)
        if t is not None:
            t.fill_(int(byte))


@contextlib.contextmanager
def poisoned_allocs():
    """Inside the body every `torch.empty` -- native.py's outputs and freshly grown workspaces -- comes back filled (NaN for floating
    types, the largest value for integer types) instead of holding whatever the allocator had.  Both settings have their previous values
    afterwards, also when the body raises."""
    det = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.utils.deterministic.fill_uninitialized_memory = fill
        torch.use_deterministic_algorithms(det, warn_only=warn)


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(run, ctx, outputs=None, finite=False, fills=FILLS):
    """run() once per fill -- 0x00 twice, then the others -- each time behind poison_scratch(ctx, fill) (ctx None: the pass has no
    caller-owned workspace that outlives the call), and the results compared as integers: all must be equal bit for bit.  run() returns
    a tensor, a sequence of tensors or a {name: tensor} dictionary; `outputs` names the entries of a dictionary to compare (default:
    every tensor in it).  The two 0x00 runs must agree before anything else is concluded: a route that differs from run to run is a
    finding of its own.  finite=True: no output holds NaN or inf either.  -> the baseline's outputs on the CPU, {name: tensor}."""
    def once(byte):
        if ctx is not None:
            poison_scratch(ctx, byte)
        out = run()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if torch.is_tensor(out):
            out = {"out": out}
        elif not isinstance(out, dict):
            out = {f"out{i}": t for i, t in enumerate(out)}
        names = outputs if outputs is not None else [k for k, v in out.items() if torch.is_tensor(v)]
        return {k: out[k].cpu() for k in names}

    base = once(fills[0])
    again = once(fills[0])
    for k in base:
        assert base[k].shape == again[k].shape and torch.equal(bits(base[k]), bits(again[k])), \
            f"{k}: two runs on zeroed scratch differ (not deterministic run to run)"
    for byte in fills[1:]:
        got = once(byte)
        for k in base:
            same = base[k].shape == got[k].shape and torch.equal(bits(base[k]), bits(got[k]))
            if not same:
                bad = (bits(base[k]) != bits(got[k])).reshape(-1).nonzero().reshape(-1)
                raise AssertionError(f"{k}: scratch filled with {byte:#04x} changes {bad.numel()} of {base[k].numel()} elements, the first at flat index "
                                     f"{int(bad[0])}: {base[k].reshape(-1)[bad[0]].item()} -> {got[k].reshape(-1)[bad[0]].item()}")
    if finite:
        for k, v in base.items():
            assert not v.is_floating_point() or bool(torch.isfinite(v).all()), f"{k}: NaN or inf in the output"
    return base
