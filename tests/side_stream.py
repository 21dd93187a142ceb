"""The caller's stream as a test input: a pass run on a side stream behind a bounded delay, its inputs real and its
scratch poisoned only behind that delay, against the same pass on the default stream, bit for bit; and the three tables that
tests/test_side_stream_host.py holds against include/si_hip.h and the sources -- the entry points that take a stream and the GPU case
that runs each one behind a delay (COVERED), those that no case runs and why (EXEMPT), and every host-side wait of csrc/ (WAITS).
A plain module, imported by name: it registers no fixture and no plugin, and importing it needs no GPU."""
import contextlib
import time

import torch

from tests import poison as P

DELAY_MS = 100.0                                       # the request front's stream-order tests wait this long too (tests/test_gpu_front.py)
DELAY_CAP_MS = 250.0
VL_SLOTS = 4                                           # si_ctx::VL_SLOTS of csrc/api.hip: pinned slots the ragged passes' length tables rotate through
LOG = []                                               # one row per delayed run: label, host enqueue ms, delay ms, returned under the delay


def _delay_cycles(target_ms=100.0):
    """Cycle count for torch.cuda._sleep that lasts about `target_ms`, from probes timed with two events (the counter's rate is the device's own)."""
    def timed(c):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(int(c))
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    timed(1000)                                                                     # the first launch loads the kernel
    c, ms = 250000, 0.0
    while ms < 5.0 and c < 10 ** 10:                                                # a probe of 5 .. 20 ms: long enough to time
        c *= 4
        ms = timed(c)
        assert ms < 250.0, (c, ms)
    assert ms >= 5.0, (c, ms)
    return int(c * target_ms / ms)


_PER_MS = []


def cycles_for(ms):
    """_delay_cycles, probed once per process."""
    if not _PER_MS:
        _PER_MS.append(_delay_cycles(DELAY_MS) / DELAY_MS)
    return int(_PER_MS[0] * ms)


_SIDE = {}
BLIND = "the probe is blind"


def _canary(dev, wait_ms=5.0):
    """One tiny op on the default stream and an event behind it -> True if it completes within `wait_ms` of host time."""
    c = _SIDE.setdefault(("canary", dev), torch.zeros(64, device=dev))
    ev = torch.cuda.Event()
    with torch.cuda.stream(torch.cuda.default_stream(dev)):
        c.add_(1.0)
        ev.record()
    t0 = time.perf_counter()
    while not ev.query() and (time.perf_counter() - t0) * 1e3 < wait_ms:
        pass
    return ev.query()


def side_stream(dev):
    """A torch side stream UNDER whose pending work the default stream is seen to run.  The runtime maps its streams onto a few
    hardware queues (GPU_MAX_HW_QUEUES, 4 by default): a side stream that shares its queue with stream 0 keeps a stray launch on stream
    0 in order behind its own work, and a delayed run on it sees nothing.  So candidates are probed -- a 20 ms delay on the candidate,
    then a tiny op on the default stream, which must complete while the delay still runs -- and the first that passes serves every
    delayed run of the process (each run repeats the probe under its own delay)."""
    if dev not in _SIDE:
        for _ in range(16):
            cand = torch.cuda.Stream(dev)
            torch.cuda.synchronize()
            e = torch.cuda.Event()
            with torch.cuda.stream(cand):
                torch.cuda._sleep(cycles_for(20.0))
                e.record()
            ok = _canary(dev) and not e.query()
            cand.synchronize()
            if ok:
                _SIDE[dev] = cand
                break
        else:
            raise AssertionError(f"{BLIND}: the default stream ran under none of 16 side streams' pending work")
    return _SIDE[dev]


def as_dict(out):
    """What run() returned as {name: tensor}: a tensor, a sequence of tensors (None entries left out) or a dictionary."""
    if torch.is_tensor(out):
        return {"out": out}
    if isinstance(out, dict):
        return {k: v for k, v in out.items() if torch.is_tensor(v)}
    return {f"out{i}": t for i, t in enumerate(out) if torch.is_tensor(t)}


def default_decoy(t):
    """Same shape and dtype, finite, other values: the tensor's own elements moved on by one place -- an integer tensor keeps its set of
    values, so a code stays inside its table -- and, for sample and feature types, halved and shifted."""
    r = torch.roll(t.reshape(-1), 1).reshape(t.shape)
    if t.is_floating_point():
        r = torch.nan_to_num(r, nan=0.3, posinf=0.7, neginf=-0.7) * 0.5 + 0.125
    elif t.dtype == torch.int16:
        r = torch.div(r, 2, rounding_mode="floor") + 3
    return r.contiguous()


def first_difference(name, want, got, what):
    """None if the two tensors hold the same bits, else poison.same_bits' message with the first differing flat index."""
    if want.shape != got.shape:
        return f"{name}: {what}: shape {tuple(got.shape)}, the default stream gave {tuple(want.shape)}"
    if want.numel() == 0 or torch.equal(P.bits(want), P.bits(got)):
        return None
    diff = P.bits(want) != P.bits(got)
    while diff.dim() > want.dim():                                                  # (a complex or packed view adds a trailing dimension)
        diff = diff.any(-1)
    bad = diff.reshape(-1).nonzero().reshape(-1)
    return (f"{name}: {what} changes {bad.numel()} of {want.numel()} elements, the first at flat index {int(bad[0])}: "
            f"{want.reshape(-1)[bad[0]].item()} -> {got.reshape(-1)[bad[0]].item()}")


def behind_a_delay(run, inputs, ctx=None, decoy=None, no_wait=True, delay_ms=DELAY_MS, owned_scratch=False, baseline=None, label=""):
    """run() on a side stream behind a delay of `delay_ms`, against run() on the default stream.

    1  baseline: run() on the current (default) stream with the real inputs, synchronised -- it also takes every lazy load and every
       growth of a workspace or of library-owned scratch (baseline= hands in an earlier call's result instead);
    2  still there: the `inputs` (data tensors only -- never an index, length or span table) are copied aside and overwritten in place
       with decoy(t) (default_decoy); with owned_scratch the pass runs once more, so that ctx->det_scratch / ctx->km_cnorm hold the
       decoy's results; synchronise;
    3  on a side stream (side_stream: one under whose work stream 0 is seen to run, shown again here by a tiny op on the default
       stream that completes under the delay): torch.cuda._sleep, event E, the real inputs copied back, poison.poison_scratch(ctx, 0xFF), run()
       inside poison.poisoned_allocs() -- whatever makes the inputs real and the scratch poisoned lies BEHIND the delay, so a launch
       that went to another stream works on the decoy or on old scratch during the delay, and what it wrote is poisoned afterwards;
    4  no_wait: E has not happened when run() returns (the host came back under the delay); after the stream is synchronised every
       output equals the baseline bit for bit.
    -> the baseline's outputs on the CPU, {name: tensor}."""
    dev = torch.device("cuda", torch.cuda.current_device())
    inputs = list(inputs.values()) if isinstance(inputs, dict) else list(inputs)
    if baseline is None:
        with P.poisoned_allocs():                                                   # (a word no pass writes is the same fill in both runs)
            baseline = {k: v.cpu() for k, v in as_dict(run()).items()}
        torch.cuda.synchronize()
    assert baseline, (label, "run() returned no tensor")
    staging = [t.clone() for t in inputs]
    for t in inputs:
        d = (decoy or default_decoy)(t)
        assert d.shape == t.shape and d.dtype == t.dtype and not torch.equal(P.bits(d), P.bits(t)), (label, "the decoy is the input")
        assert not d.is_floating_point() or bool(torch.isfinite(d).all()), (label, "the decoy is not finite")
        t.copy_(d)
    if owned_scratch:
        run()
    torch.cuda.synchronize()
    side = side_stream(dev)
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sighted = False
    try:
        with torch.cuda.stream(side):
            a.record()
            torch.cuda._sleep(cycles_for(delay_ms))
            e.record()
            sighted = _canary(dev) and not e.query()
            for t, s in zip(inputs, staging):
                t.copy_(s)
            if ctx is not None:
                P.poison_scratch(ctx, 0xFF)
            with P.poisoned_allocs():
                t0 = time.perf_counter()
                out = run()
                enqueue_ms = (time.perf_counter() - t0) * 1e3
            under = not e.query()
    finally:
        side.synchronize()
        for t, s in zip(inputs, staging):                                           # whatever happened, the next case finds the real inputs
            t.copy_(s)
        torch.cuda.synchronize()
    slept = a.elapsed_time(e)
    LOG.append((label, enqueue_ms, slept, under))
    assert sighted, f"{label}: {BLIND}: an op on the default stream did not complete under the delay queued on the side stream"
    assert slept <= max(DELAY_CAP_MS, 2.5 * delay_ms), (label, f"the delay took {slept:.0f} ms")
    if no_wait:
        assert under, (f"{label}: the call waited for the caller's stream: it returned after the {slept:.0f} ms delay in front of it had "
                       f"run out ({enqueue_ms:.1f} ms on the host)")
    got = {k: v.cpu() for k, v in as_dict(out).items()}
    assert sorted(got) == sorted(baseline), (label, sorted(got), sorted(baseline))
    for k in baseline:
        msg = first_difference(k, baseline[k], got[k], "behind a delay on a side stream")
        if msg:
            raise AssertionError(f"{label}: {msg}")
    return baseline


@contextlib.contextmanager
def calls_recorded(lib):
    """Inside the body every call of an entry point of COVERED through `lib` is noted -> the set of their names."""
    seen, saved = set(), {}
    for name in COVERED:
        fn = getattr(lib, name)
        saved[name] = fn

        def spy(*args, _fn=fn, _name=name):
            seen.add(_name)
            return _fn(*args)
        setattr(lib, name, spy)
    try:
        yield seen
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


# ------------------------------------------------------------------------------------------------------------ the three tables
# Every declaration of include/si_hip.h with a si_stream_t parameter -> the case of tests/test_gpu_side_stream.py that calls it inside
# behind_a_delay (that file's last test holds each pair against the calls it recorded).
COVERED = {
    "si_hubert_forward": "encoder tiny fp32 forward",
    "si_hubert_forward_padded": "encoder tiny fp32 padded",
    "si_hubert_forward_varlen": "encoder tiny fp32 varlen",
    "si_hubert_forward_spans": "encoder tiny fp32 spans",
    "si_hubert_extract_features": "encoder tiny fp32 extract",
    "si_hifigan_forward": "generator v1-fp16 uniform",
    "si_hifigan_forward_varlen": "generator v1-fp16 ragged",
    "si_mel_frontend": "mel uniform 0",
    "si_mel_frontend_spans": "mel uniform 2",
    "si_mel_frontend_varlen": "mel ragged varlen",
    "si_f0_encoder_forward": "f0 encoder T=877",
    "si_codebook_splice": "codebook grid",
    "si_codebook_splice_varlen": "codebook grid",
    "si_codebook_splice_labels": "codebook grid",
    "si_codebook_metrics": "codebook grid",
    "si_codebook_splice_spans": "codebook table",
    "si_codebook_splice_labels_spans": "codebook table",
    "si_codebook_metrics_spans": "codebook table",
    "si_code_splice": "units",
    "si_unit_frontend": "units",
    "si_kmeans_assign": "kmeans mfma",
    "si_mel_metrics": "metrics",
    "si_sisdr": "metrics",
    "si_resample_poly": "resamplers",
    "si_resample_sinc": "resamplers",
    "si_pcm16": "pcm16 and extend_mel",
    "si_extend_mel": "pcm16 and extend_mel",
    "si_wave_peak": "patch mode",
    "si_gather_windows": "patch mode",
    "si_patch_compose": "patch mode",
    "si_cut_clips": "long recordings",
    "si_cut_clips_valid": "long recordings",
    "si_patch_regions": "long recordings",
    "si_quiet_runs": "detector quiet",
    "si_quiet_runs_ch": "detector quiet",
    "si_dead_runs": "detector dead",
    "si_level_runs": "detector level",
    "si_burst_runs": "detector burst",
    "si_invalid_runs": "detector invalid",
    "si_impulse_runs": "detector impulse",
    "si_impulse_residual": "impulse residual",
    "si_mend_runs": "mend runs",
    "si_patch_rate": "patch rate 48000",
    "si_patch_rate_ch": "patch rate 48000",
    "si_cut_rate": "cut rate 48000",
    "si_cut_rate_ch": "cut rate 48000",
    "si_cut_rate_valid": "cut rate 48000",
    "si_cut_pair": "cut pair 48000",
    "si_cut_pair_ch": "cut pair 48000",
    "si_cut_pair_valid": "cut pair 48000",
}
# ... and those that no case runs, each with its reason.
EXEMPT = {}

# Every hipStreamSynchronize, hipEventSynchronize, hipDeviceSynchronize and synchronous hipMemcpy (the symbol copies included) of
# csrc/*.hip and csrc/*.cpp: (file, enclosing function, call, reason).  The reasons: "setup" -- before or outside any pass, or once on a
# context's first pass of its kind; "growth" -- library-owned scratch is replaced by a larger block and the stream must be done with the
# old one; "slot reuse" -- a pinned slot's previous copy must have left it; "profile stop" -- an instrumentation read-out that is
# documented to wait.  A wait that is in the sources and not here fails tests/test_side_stream_host.py until someone classifies it.
WAIT_REASONS = ("setup", "growth", "slot reuse", "profile stop")
WAITS = (
    ("api.hip", "vl_upload", "hipEventSynchronize", "slot reuse"),
    ("api.hip", "si_destroy", "hipEventSynchronize", "setup"),
    ("api.hip", "si_load_weights", "hipMemcpy", "setup"),
    ("api.hip", "si_weights_check", "hipMemcpy", "setup"),
    ("api.hip", "si_kmeans_assign", "hipStreamSynchronize", "growth"),
    ("api.hip", "ensure_frontend", "hipMemcpy", "setup"),
    ("api.hip", "det_scratch_reserve", "hipStreamSynchronize", "growth"),
    ("api.hip", "si_profile_stop", "hipEventSynchronize", "profile stop"),
    # the instrumented builds' read-outs (libsi_hip_timeline.so, libsi_hip_stamps.so): no stream argument, never called by a pass
    ("gemmcu.hip", "si_debug_gcu_timeline", "hipMemcpyFromSymbol", "profile stop"),
    ("gemmcu.hip", "si_debug_gcu_timeline", "hipMemcpyToSymbol", "profile stop"),
    ("reschain.hip", "si_debug_rc_timeline", "hipMemcpyFromSymbol", "profile stop"),
    ("reschain.hip", "si_debug_rc_timeline", "hipMemcpyToSymbol", "profile stop"),
    ("respair_wide.hip", "si_debug_rpw_timeline", "hipMemcpyFromSymbol", "profile stop"),
    ("respair_wide.hip", "si_debug_rpw_timeline", "hipMemcpyToSymbol", "profile stop"),
    ("tapgemm.hip", "si_debug_stamps", "hipMemcpyFromSymbol", "profile stop"),
    ("tapgemm.hip", "si_debug_stamps", "hipMemcpyToSymbol", "profile stop"),
)

# Kernels that share a profile family name with another route: the ledger of tests/test_gpu_side_stream.py marks each as run.
SHARED_FAMILY_ROUTES = {
    "detect_dead": ("dead", "dead_ch", "level", "burst", "impulse", "impulse residual"),
    "detect_bits": ("quiet", "invalid"),
    "detect_bits_ch": ("quiet_ch", "invalid_ch"),
    "cut_rate": ("cut_rate", "cut_pair"),
    "cut_rate_ch": ("cut_rate_ch", "cut_pair_ch"),
    "patch_rate": ("patch_rate", "mend_runs"),
}
