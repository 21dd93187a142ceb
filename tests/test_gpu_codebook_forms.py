"""The codebook kernels' two forms -- the (Lm, B) grid over `frame_pos[b] + j` [with a per-clip `frame_cnt`] and the frame table of
(clip, frame) entries -- are two instantiations of one body each (splice, gather, metrics).  These tests pin the instantiations to
each other, bit for bit, at the edges where the index policy can go wrong: a clip that crosses the mel's end (a label, no column),
the encoder's end (label -1), one that starts before frame 0, a per-clip count, and a table entry outside the batch.  Both sides are
the library: the claim is that they are one body.  Correctness against the reference stays with the oracle tests."""
import pytest
import torch

from tests.common import case_engine, load_case

pytestmark = pytest.mark.gpu

B, T, D, TM, LM = 3, 7, 80, 6, 4
FRAME_POS = [0, 4, -2]      # clip 1 crosses Tm at pos 6 (label, no column) and T at pos 7 (label -1); clip 2: labels -1 at j = 0, 1


@pytest.fixture(scope="module")
def forms():
    c = load_case("tiny_group")
    K = c["meta"]["K"]
    eng = case_engine(c)
    assert eng.harch.codebook_dim == D
    feats = torch.randn(B, T, D, generator=torch.Generator().manual_seed(5)).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    pairs = [(b, FRAME_POS[b] + j) for b in range(B) for j in range(LM)]           # the same 12 (clip, frame) pairs, b-major
    return dict(ctx=eng.ctx, K=K, feats=feats, i32=i32, pos=i32(FRAME_POS), pairs=pairs,
                clip=i32([b for b, _ in pairs]), frame=i32([p for _, p in pairs]))


def _mel():
    return torch.zeros(B, D, TM, device="cuda")


def test_splice_grid_equals_table(forms):
    f = forms
    mel_g, mel_t = _mel(), _mel()
    lab_g = f["ctx"].codebook_splice(f["feats"], f["pos"], LM, mel_g)
    lab_t = f["ctx"].codebook_splice_spans(f["feats"], f["clip"], f["frame"], mel_t)
    assert torch.equal(lab_g.reshape(-1), lab_t) and torch.equal(mel_g, mel_t)
    lab = lab_g.cpu()
    assert (lab[0] >= 0).all() and (lab[1, :3] >= 0).all() and lab[1, 3] == -1          # pos 7 = T
    assert (lab[2, :2] == -1).all() and (lab[2, 2:] >= 0).all()                         # pos -2, -1
    assert mel_g[1, :, 4:6].abs().sum() > 0 and mel_g[2, :, 2:].abs().sum() == 0         # pos 6 = Tm: no column; clip 2 writes 0, 1


def test_given_labels_grid_equals_table(forms):
    f = forms
    given = torch.tensor([[3, -1, 7, f["K"]], [0, 1, 2, 3], [4, 5, f["K"] - 1, -1]], dtype=torch.int64, device="cuda")
    mel_g, mel_t = _mel(), _mel()
    f["ctx"].codebook_splice_labels(given, f["pos"], mel_g)
    f["ctx"].codebook_splice_labels_spans(given.reshape(-1).contiguous(), f["clip"], f["frame"], mel_t)
    assert torch.equal(mel_g, mel_t)
    assert mel_g[0, :, 0].abs().sum() > 0 and mel_g[0, :, 1].abs().sum() == 0 and mel_g[0, :, 3].abs().sum() == 0   # labels -1 and K


def test_metrics_grid_equals_table(forms):
    f = forms
    tgt = torch.tensor([[3, -1, 7, 9], [0, f["K"], 2, 3], [4, 5, 6, 8]], dtype=torch.int64, device="cuda")
    loss_g, terms_g, pred_g, cpt_g = f["ctx"].codebook_metrics(f["feats"], f["pos"], LM, tgt)
    loss_t, terms_t, pred_t, cpt_t = f["ctx"].codebook_metrics_spans(f["feats"], f["clip"], f["frame"], tgt.reshape(-1).contiguous())
    bits = lambda x: x.reshape(-1).view(torch.int32)                                  # bit patterns: the NaNs count
    assert torch.equal(pred_g.reshape(-1), pred_t)
    assert torch.equal(bits(terms_g), bits(terms_t)) and torch.equal(bits(cpt_g), bits(cpt_t))
    assert torch.equal(bits(loss_g), bits(loss_t))
    assert torch.isnan(terms_g[0, 1]) and torch.isnan(terms_g[1, 1]) and torch.isnan(terms_g[1, 3]) and not torch.isnan(terms_g[0, 0])


def test_per_clip_counts_equal_the_table_of_the_counted_entries(forms):
    f = forms
    cnt = [4, 2, 0]
    mel_g, mel_t = _mel(), _mel()
    lab_g = f["ctx"].codebook_splice_varlen(f["feats"], f["pos"], f["i32"](cnt), LM, mel_g)
    kept = [(b, p) for k, (b, p) in enumerate(f["pairs"]) if k % LM < cnt[b]]
    lab_t = f["ctx"].codebook_splice_spans(f["feats"], f["i32"]([b for b, _ in kept]), f["i32"]([p for _, p in kept]), mel_t)
    assert torch.equal(mel_g, mel_t)
    assert torch.equal(torch.cat([lab_g[b, :cnt[b]] for b in range(B)]), lab_t)
    for b in range(B):
        assert (lab_g[b, cnt[b]:] == -1).all()


def test_table_entry_outside_the_batch(forms):
    f = forms
    mel = _mel()
    lab = f["ctx"].codebook_splice_spans(f["feats"], f["i32"]([B]), f["i32"]([1]), mel)
    assert lab.tolist() == [-1] and mel.abs().sum() == 0
