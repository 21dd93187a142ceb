"""What the GPU tests share, once: the scoped environment, the engine builder, the tapped and profiled run, the summary of ratios.
A plain module, imported by name: it registers no fixture and no plugin, and importing it needs no GPU."""
import contextlib
import os

import torch

torch.set_num_threads(16)                              # the float64 references run on the CPU

_ENGINES = {}                                          # build_engine(key=...): engines kept for the session


@contextlib.contextmanager
def scoped_env(env):
    """Set the variables of `env` for the body; afterwards, also when the body raises, each has its previous value or is unset again.
    The library reads most SI_* switches in si_create (wrap the engine's construction), SI_KMEANS_MFMA per call (wrap the call)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build_engine(harch, varch, K, enc="fp32", voc="fp32", *, vocoder_chunk=0, env=None, state=None, key=None):
    """An InpaintingEngine on cuda:0 with its weights loaded.  env: switches set while the context is created.  state: the (HuBERT,
    generator, codebook) triple, an entry None for the synthetic one at synth's default seed.  key: keep the engine under it for the
    session and hand the same one back (begin the key with the file's own name); without a key every call builds a fresh engine."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.engine import InpaintingEngine
    if key is not None and key in _ENGINES:
        return _ENGINES[key]
    hsd, gsd, cb = state or (None, None, None)
    with scoped_env(env or {}):
        eng = InpaintingEngine(harch, varch, K, "cuda:0", enc, voc, vocoder_chunk)
    eng.load_state(hsd if hsd is not None else synth.synth_hubert_state(harch), gsd if gsd is not None else synth.synth_generator_state(varch),
                   cb if cb is not None else synth.synth_codebook(K))
    if key is not None:
        _ENGINES[key] = eng
    return eng


def tapped_run(ctx, capacity, forward, require_all=False, profile=True, max_launches=4000):
    """forward() with the taps {name: element count} registered on the context `ctx` and, if `profile`, its launches counted ->
    (taps {name: flat cpu tensor}, forward's result, {kernel family: launches}).  A tap counts as produced when the pass filled it to
    exactly its capacity; one that was not is left out, or with require_all is an assertion failure.  However the body ends, the
    context is left with no capture registered and with profiling stopped: a kept engine serves the next test."""
    ctx.clear_captures()
    try:
        caps = ctx.capture(list(capacity), capacity=capacity) if capacity else {}
        if profile:
            ctx.profile_start(max_launches)
        try:
            out = forward()
        finally:
            prof = {e["name"]: e["launches"] for e in ctx.profile_stop()} if profile else {}
        torch.cuda.synchronize()
        taps = {}
        for k, t in caps.items():
            produced = ctx.lib.si_debug_size(ctx._h, k.encode()) == capacity[k]
            assert produced or not require_all, (k, "was not produced")
            if produced:
                taps[k] = t.cpu()
    finally:
        ctx.clear_captures()
    return taps, out, prof


class RatioSummary:
    """max err / E per kernel over the checks of one file: rows near a tile seam or clip edge | the rest, and the number of checks.
    With `group` set a key reads "{group} | {kernel}".  The fp16 tap-GEMM's tile shapes follow the layer, so its configurations
    (profile names "tapgemm_f16_<tile>", several joined by "+") share the one line "tapgemm_f16_*"."""
    def __init__(self, digits=4):
        self.group = ""
        self.rows = {}                                 # key -> [near, rest, checks]
        self.line = f"   SUMMARY {{key}}: max err/E seam+edge rows {{near:.{digits}f}}, interior {{rest:.{digits}f}} over {{checks}} checks"

    def note(self, kernel, near, rest):
        if kernel.startswith("tapgemm_f16_"):
            kernel = "tapgemm_f16_*"
        s = self.rows.setdefault(f"{self.group} | {kernel}" if self.group else kernel, [0.0, 0.0, 0])
        s[0], s[1], s[2] = max(s[0], near), max(s[1], rest), s[2] + 1

    def report(self, line=None, keys=None):
        """Print one line per key (sorted, or the given ones that have a note) and assert that no ratio exceeds 1."""
        for k in sorted(self.rows) if keys is None else [k for k in keys if k in self.rows]:
            near, rest, checks = self.rows[k]
            print((line or self.line).format(key=k, near=near, rest=rest, checks=checks))
            assert near <= 1.0 and rest <= 1.0, (k, near, rest)
