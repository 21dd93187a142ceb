"""The request front (speech_inpainting_amd/stream.py) against the unpipelined path, bit for bit: at file rates other
than 22.05 kHz (its own length rule, both resamplers), while every slot buffer grows, with the copy stream ordered behind the compute
stream where a new buffer needs it and nowhere else, across runs that end early or with a refusal, and with a resampler cache whose
size does not follow the lengths it has seen."""
import math
import time

import numpy as np
import pytest
import torch

from tests.front_ref import assert_same, reference_result
from tests.harness import build_engine
from tests.side_stream import _delay_cycles

pytestmark = pytest.mark.gpu

T0 = time.time()
ENGINES = [("fp32", "fp32"), ("bf16", "fp16")]


def _engine(enc="fp32", voc="fp32", fresh=False):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.tiny(), 50, enc, voc, key=None if fresh else f"test_gpu_front:{enc}:{voc}")


def _clips(lens, sr, seed):
    from speech_inpainting_amd import synth
    return [synth.synth_wave(1, int(n), seed + i, sr=sr)[0].numpy() for i, n in enumerate(lens)]


def _slot_ptrs(front):
    return [tuple(None if t is None else (t.data_ptr(), t.numel()) for t in (s.pin_in, s.dev_in, s.pin_out, s.pin_lab, s.pin_tab, s.dev_tab))
            for s in front.slots]


# ------------------------------------------------------------------------------------------------------------ 1: every rate
# per request: seconds per clip -- at 37800 Hz the sample counts instead, with the clips whose 22.05 kHz length the product-first rule
# ceil(n * 22050.0 / 37800) gets one short: 27900 and 25632 lose a mel frame by it, 49164 / 49176 / 49188 one sample of the patched PCM
SECS = dict(uniform=[1.2, 1.2, 1.2], masked=[1.0, 2.3, 1.6, 0.9], blind=[2.0, 1.1, 1.7], gaps=[1.0, 2.3, 1.6, 0.9], patch=[1.5, 1.3, 1.1])
AT_37800 = dict(uniform=[45360] * 3, masked=[37800, 27900, 60480, 25632], blind=[75600, 27900, 25632], gaps=[27900, 86940, 60480, 25632],
                patch=[56700, 49164, 41580])
GAPS = [[(5, 5), (30, 6)], [(2, 3), (40, 10), (80, 7)], [(10, 4), (50, 6)], [(20, 6)]]
PATCH_GAPS = [[(30, 4), (35, 4)], [(10, 6)], [(20, 5)]]


def _rate_requests(sr):
    from speech_inpainting_amd.stream import Request
    n = {k: (AT_37800[k] if sr == 37800 else [int(s * sr) for s in v]) for k, v in SECS.items()}
    pos = lambda k: [8 + 3 * i for i in range(len(n[k]))]
    return [Request(_clips(n["uniform"], sr, 1100), pos("uniform"), 5, tag="uniform"),
            Request(_clips(n["masked"], sr, 1110), pos("masked"), 5, tag="masked"),
            Request(_clips(n["blind"], sr, 1120), pos("blind"), 5, True, tag="blind"),
            Request(_clips(n["gaps"], sr, 1130), gaps=GAPS, tag="gaps"),
            Request(_clips(n["patch"], sr, 1140), gaps=PATCH_GAPS, patch=True, fade=110, tag="patch")]


def test_the_37800_hz_clips_are_the_ones_the_two_length_rules_split():
    """(host arithmetic, kept next to the requests it vouches for) at 37800 -> 22050 the product-first rule gives 27900 and 25632
    samples one mel frame fewer than the resampler's rule, and the patch batch's 49164 one sample fewer."""
    from speech_inpainting_amd import audio
    from speech_inpainting_amd.arch import mel_frames
    old = lambda n: int(math.ceil(n * float(22050) / 37800))
    for n in (27900, 25632):
        assert any(n in AT_37800[k] for k in ("masked", "blind", "gaps"))
        assert mel_frames(old(n)) + 1 == mel_frames(audio.resampled_len(n, 37800, 22050)), n
    assert all(27900 in AT_37800[k] and 25632 in AT_37800[k] for k in ("masked", "blind", "gaps"))
    hit = [n for n in AT_37800["patch"] if n in (49164, 49176, 49188)]
    assert hit and all(old(n) + 1 == audio.resampled_len(n, 37800, 22050) for n in hit)
    for k in SECS:
        assert len(SECS[k]) == len(AT_37800[k]) and (k == "uniform") == (len(set(AT_37800[k])) == 1)


@pytest.mark.parametrize("enc,voc", ENGINES)
@pytest.mark.parametrize("sr", [16000, 8000, 44100, 48000, 37800, 22050])
def test_front_at_every_file_rate_equals_the_unpipelined_path(sr, enc, voc):
    """Five requests (uniform masked, ragged masked, ragged blind, ragged gaps=, ragged patch=True) at the file rate `sr` through
    predict_stream(depth=2): at 16000 the 16 kHz side is the identity and the 22.05 kHz side is up-sampled, at 22050 the reverse, at
    every other rate both resamplers run."""
    from speech_inpainting_amd.stream import predict_stream
    eng = _engine(enc, voc)
    reqs = _rate_requests(sr)
    got = list(predict_stream(eng, reqs, sr_in=sr, depth=2))
    assert [g.tag for g in got] == [r.tag for r in reqs]
    for rq, g in zip(reqs, got):
        assert_same(g, reference_result(eng, rq, sr), (sr, enc, voc, rq.tag))


# ------------------------------------------------------------------------------------------------------------ 2: growth ladder
def _ladder():
    """Eight requests, each larger than the one before in every size a slot buffer is cut from (clips x longest clip, PCM, labels,
    tables), with and without gaps; then a small one."""
    from speech_inpainting_amd.stream import Request
    reqs = []
    for k in range(8):
        B = 2 + k // 2
        lens = [int((0.9 + 0.2 * k - 0.04 * j) * 22050) for j in range(B)]
        clips = _clips(lens, 22050, 1200 + 10 * k)
        if k in (2, 5):
            reqs.append(Request(clips, [4 + j for j in range(B)], 3 + k, tag=k))
        else:
            reqs.append(Request(clips, gaps=[[(2, 2), (10 + j, 1 + k)] for j in range(B)], tag=k))
    reqs.append(Request(_clips([15435, 17640], 22050, 1290), gaps=[[(3, 2)], []], tag=8))
    return reqs


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_front_while_every_slot_buffer_grows(depth):
    from speech_inpainting_amd.stream import RequestFront
    eng = _engine()
    reqs = _ladder()
    front = RequestFront(eng, sr_in=22050, depth=depth)
    sizes = []
    ensure = front._ensure

    def spy(s, B, n_in, n_out, lm, n_tab=0):
        sizes.append((B * n_in, B * n_out, B * max(lm, 1), n_tab))
        return ensure(s, B, n_in, n_out, lm, n_tab)
    front._ensure = spy
    got = list(front.run(reqs))
    assert [g.tag for g in got] == list(range(9)) and len(sizes) == 9
    for a, b in zip(sizes[:7], sizes[1:8]):                                         # every buffer of every slot grows at every reuse
        assert a[0] < b[0] and a[1] < b[1] and a[2] < b[2], (a, b)
    tabs = [s[3] for s in sizes[:8] if s[3]]
    assert len(tabs) == 6 and all(a < b for a, b in zip(tabs, tabs[1:])), tabs
    assert all(x < y for x, y in zip(sizes[8], sizes[0]))                           # and the last request fits what is there
    for rq, g in zip(reqs, got):
        assert_same(g, reference_result(eng, rq, 22050), (depth, rq.tag))


# ------------------------------------------------------------------------------------------------------------ 3: stream order
def _probe(front, rq, numel, dtype, which):
    """A tensor of the compute stream (`numel` of `dtype`: exactly what the slot's device buffer `which` will take) is filled, a
    bounded delay and a copy of it are queued behind, and it is freed ON THE HOST while both are still queued; then the request is
    submitted to a slot without buffers.  The allocator hands the slot that block.  The queued copy must still read the pattern."""
    slot = front.slots[0]
    assert getattr(slot, which) is None
    pattern = 7.25 if dtype == torch.float32 else 0x5A5A5A5A
    cycles = _delay_cycles()
    # blocks of the same size that earlier tests left free would be handed out before the victim's: take them out of the way
    hold = [torch.empty(numel, dtype=dtype, device="cuda:0") for _ in range(256)]
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    victim = torch.empty(numel, dtype=dtype, device="cuda:0")
    victim.fill_(pattern)
    ptr = victim.data_ptr()
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    out = victim.clone()
    del victim
    front._submit(slot, rq)
    torch.cuda.synchronize()
    same_block = getattr(slot, which).data_ptr() == ptr
    intact = bool((out == pattern).all())
    print(f"   {which}: {numel * out.element_size()} bytes, delay {a.elapsed_time(b):.1f} ms, the slot got the freed block: {same_block}, "
          f"the queued copy read the pattern: {intact}")
    assert a.elapsed_time(b) <= 250.0
    assert getattr(slot, which).numel() == numel and getattr(slot, which).dtype == dtype
    assert same_block, "the probe is blind: the allocator did not hand the slot the block that was just freed"
    assert intact, f"the copy stream wrote {which} while the compute stream still read that block"
    del hold
    return front._collect(slot)


def test_first_copy_into_a_new_clip_buffer_waits_for_the_compute_stream():
    from speech_inpainting_amd.stream import Request, RequestFront
    eng = _engine()
    rq = Request(_clips([22050, 22050], 22050, 1300), [8, 11], 5)
    res = _probe(RequestFront(eng, sr_in=22050, depth=1), rq, 2 * 22050, torch.float32, "dev_in")
    assert_same(res, reference_result(eng, rq, 22050))


def test_first_copy_into_a_new_table_buffer_waits_for_the_compute_stream():
    from speech_inpainting_amd.stream import Request, RequestFront
    eng = _engine()
    gaps = [[(3, 4), (20, 6)], [(0, 2), (10, 3), (30, 5)]]
    rq = Request(_clips([22050, 22050], 22050, 1310), gaps=gaps)
    S, F, B = 5, 20, 2
    res = _probe(RequestFront(eng, sr_in=22050, depth=1), rq, 2 * (B + 2 + 2 * S) + 2 * F, torch.int32, "dev_tab")
    assert_same(res, reference_result(eng, rq, 22050))


# ------------------------------------------------------------------------------------------------------------ 4: overlap kept
class _CountingStream(torch.cuda.Stream):
    """A copy stream that counts what it is made to wait for."""
    def __new__(cls, device):
        self = super().__new__(cls, device=device)
        self.stream_waits = self.event_waits = 0
        return self

    def wait_stream(self, stream):
        self.stream_waits += 1
        return super().wait_stream(stream)

    def wait_event(self, event):
        self.event_waits += 1
        return super().wait_event(event)


def test_a_request_that_grows_nothing_makes_the_copy_stream_wait_for_nothing(monkeypatch):
    """Both slots warmed with the shapes of the two requests that follow (clips, and clips with gap tables): the warm-up's allocations
    make the copy stream wait, the second pair -- same shapes, other samples -- not once, whether the wait is asked of the front's own
    stream object or of another handle of the same stream (torch.cuda.current_stream() inside `with torch.cuda.stream(h2d)`)."""
    from speech_inpainting_amd.stream import Request, RequestFront
    eng = _engine()
    front = RequestFront(eng, sr_in=44100, depth=2)
    front.h2d = h2d = _CountingStream(eng.device)
    other = []                                                                      # waits on the same stream through another object
    for name in ("wait_stream", "wait_event"):
        orig = getattr(torch.cuda.Stream, name)

        def spy(self, arg, _orig=orig, _name=name):
            if self is not h2d and self == h2d:
                other.append(_name)
            return _orig(self, arg)
        monkeypatch.setattr(torch.cuda.Stream, name, spy)

    def pair(seed):
        return [Request(_clips([44100, 39000, 52000], 44100, seed), [8, 11, 14], 5, tag=0),
                Request(_clips([48000, 61000], 44100, seed + 5), gaps=[[(3, 4), (20, 6)], [(0, 2), (40, 5)]], tag=1)]
    warm = pair(1400) + pair(1410)[::-1]                                            # slot 0 and slot 1 each see both shapes
    assert len(list(front.run(warm))) == 4
    grew = (h2d.stream_waits, h2d.event_waits, len(other))
    assert grew[0] + grew[1] + grew[2] > 0, "the spy is blind: the warm-up allocated every slot buffer and no wait was counted"
    ptrs = _slot_ptrs(front)
    h2d.stream_waits = h2d.event_waits = 0
    del other[:]
    reqs = pair(1420) + pair(1430)[::-1]
    got = list(front.run(reqs))
    assert [g.tag for g in got] == [0, 1, 1, 0]
    print(f"   waits of the copy stream: warm-up {grew}, steady state {(h2d.stream_waits, h2d.event_waits, len(other))}")
    assert (h2d.stream_waits, h2d.event_waits, other) == (0, 0, [])
    assert _slot_ptrs(front) == ptrs
    for rq, g in zip(reqs, got):
        assert_same(g, reference_result(eng, rq, 44100), rq.tag)


# ------------------------------------------------------------------------------------------------------------ 5: life cycle
def test_a_front_serves_the_next_run_after_an_early_exit_or_a_refusal():
    from speech_inpainting_amd.stream import Request, RequestFront
    eng = _engine()
    front = RequestFront(eng, sr_in=22050, depth=2)
    big_blind = lambda s: Request(_clips([39690] * 4, 22050, s), [0] * 4, 5, True)
    big_gaps = lambda s: Request(_clips([39690] * 4, 22050, s), gaps=[[(2, 3), (20, 10), (60, 12)]] * 4, patch=True, fade=200)
    assert len(list(front.run([big_blind(1500), big_blind(1504), big_gaps(1508), big_gaps(1512)]))) == 4     # each slot: its largest buffers
    ptrs = _slot_ptrs(front)
    assert all(p is not None for slot in ptrs for p in slot)

    def good(seed):
        return Request(_clips([22050, 26460], 22050, seed), [8, 11], 5, tag=seed)
    three = [Request(_clips([26460] * 3, 22050, 1520), [8, 11, 14], 5, tag="uniform"),
             Request(_clips([22050, 35280], 22050, 1530), gaps=[[(5, 5)], [(2, 3), (40, 10)]], tag="gaps"),
             Request(_clips([24255, 19845], 22050, 1540), [0, 0], 5, True, tag="blind")]
    want = [reference_result(eng, rq, 22050) for rq in three]
    clips = _clips([22050, 22050], 22050, 1550)

    def check(case):
        for i, s in enumerate(front.slots):
            assert s.meta is None and s.keep == (), (case, i)
            assert s.ev_d2h.query() and s.ev_done.query() and s.ev_h2d.query(), (case, i)
        got = list(front.run(three))
        assert [g.tag for g in got] == [r.tag for r in three]
        for g, w in zip(got, want):
            assert_same(g, w, (case, g.tag))
        assert _slot_ptrs(front) == ptrs, case
        assert all(s.meta is None and s.keep == () for s in front.slots), case

    # (a) one result of four, then the generator is closed: batch 1 is in flight at that moment, batches 2 and 3 were never submitted
    four = [good(1560 + 10 * i) for i in range(4)]
    gen = front.run(four)
    first = next(gen)
    assert any(s.meta is not None for s in front.slots)
    gen.close()
    assert_same(first, reference_result(eng, four[0], 22050), "a")
    check("closed early")
    # (b) a gap that overlaps another one: refused with the clip and the gap named, while the good batch is in flight
    with pytest.raises(ValueError, match="clip 1: gap 1"):
        list(front.run([good(1600), Request(clips, gaps=[[(3, 4)], [(5, 5), (8, 2)]])]))
    check("bad gaps")
    # (c) blind mode with gaps
    with pytest.raises(ValueError, match="blind"):
        list(front.run([good(1610), Request(clips, blind=True, gaps=[[(3, 4)], []])]))
    check("blind with gaps")


# ------------------------------------------------------------------------------------------------------------ 6: resampler cache
def _device_tensors(obj, seen=None):
    """The distinct device tensors reachable from `obj` through dictionaries, lists and tuples."""
    seen = {} if seen is None else seen
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            seen[obj.data_ptr()] = obj
    elif isinstance(obj, dict):
        for v in obj.values():
            _device_tensors(v, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _device_tensors(v, seen)
    return seen


def test_resampler_cache_does_not_grow_with_the_lengths_it_has_seen():
    """24 ragged requests at 44.1 kHz, every one with another longest clip (in no order: the shared time-register table both grows
    and serves shorter clips), through one front: the engine holds as many device tables after the last as after the first, at most
    three per rate pair (win, dwin, time_reg), and every result is what an engine that has seen nothing else returns."""
    from speech_inpainting_amd.stream import Request, RequestFront
    sr = 44100
    eng = _engine(fresh=True)
    front = RequestFront(eng, sr_in=sr, depth=2)
    order = [(7 * i) % 24 for i in range(24)]                                       # 0, 7, 14, 21, 4, ...: grows and shrinks
    longest = [int(0.9 * sr) + 1111 * j for j in order]
    assert len(set(longest)) == 24 and max(longest) <= int(2.3 * sr)
    reqs = [Request(_clips([n, int(0.7 * sr) + 13 * i], sr, 1700 + 2 * i), [8, 11], 5, tag=i) for i, n in enumerate(longest)]
    try:
        first = list(front.run(reqs[:1]))
        after_first = len(_device_tensors(eng._resamplers))
        keys = list(eng._resamplers)
        got = first + list(front.run(reqs[1:]))
        after_all = len(_device_tensors(eng._resamplers))
        print(f"   device tables of the resampler cache: {after_first} after one request, {after_all} after 24 lengths; entries {list(eng._resamplers)}")
        assert after_all == after_first and list(eng._resamplers) == keys
        assert len(keys) == 2 and after_all <= 3 * len(keys)
        t0 = time.time()
        for rq, g in zip(reqs, got):
            fresh = _engine(fresh=True)
            try:
                assert_same(g, reference_result(fresh, rq, sr), rq.tag)
            finally:
                fresh.ctx.close()
        print(f"   24 fresh engines and their references: {time.time() - t0:.1f} s")
        # the file-rate routes' filters are the same device tables, not copies
        assert eng._feed_filter(sr)["win"].data_ptr() == eng._sinc_tables(sr, 22050)["win"].data_ptr()
        assert len(_device_tensors(eng._resamplers)) == after_all
        # kind="poly" as before: one entry per length, ragged batches refused, and the same samples as an engine that ran nothing else
        x = torch.from_numpy(np.stack(_clips([30000, 30000], sr, 1790))).cuda()
        fresh = _engine(fresh=True)
        try:
            for n in (30000, 20011):
                y = eng.resample(x[:, :n].contiguous(), sr, 16000, kind="poly")
                assert y.shape == (2, -(-n * 160 // 441)) and torch.equal(y, fresh.resample(x[:, :n].contiguous(), sr, 16000, kind="poly")), n
                assert ("poly", sr, 16000, n) in eng._resamplers
        finally:
            fresh.ctx.close()
        with pytest.raises(ValueError, match="kaiser_best"):
            eng.resample(x, sr, 16000, kind="poly", lens=[30000, 20000])
        torch.cuda.synchronize()
    finally:
        eng.ctx.close()


def test_zz_wall_time_of_this_file():
    print(f"   tests/test_gpu_front.py took {time.time() - T0:.1f} s")
