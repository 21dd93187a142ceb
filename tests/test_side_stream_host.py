"""tests/side_stream.py on the CPU: every entry point of include/si_hip.h that takes a stream is in exactly one of its two
tables, every host-side wait of csrc/ is in the third with a reason, and the pieces of the harness that need no GPU do what they say."""
import glob
import os
import re

import pytest
import torch

from tests import side_stream as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_inpainting_amd", "csrc")

DECL = re.compile(r"\b(?:int|size_t|void|const\s+char\s*\*)\s+(si_\w+)\s*\(([^;{}]*?)\)\s*;", re.S)
WAIT = re.compile(r"\b(hipStreamSynchronize|hipEventSynchronize|hipDeviceSynchronize|hipMemcpy|hipMemcpyToSymbol|hipMemcpyFromSymbol|hipMemcpyDtoH|hipMemcpyHtoD)\s*\(")
FUNC = re.compile(r"^(?!\s)(?:[\w:<>\*&,\s]|\"C\")*?\b(\w+)\s*\([^;]*$")
NOT_A_FUNCTION = ("if", "for", "while", "switch", "return", "sizeof", "defined")


def declarations(header):
    """{name: parameter text} of the functions a C header declares, comments removed."""
    return dict(DECL.findall(re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))


def waits(name, text):
    """[(file, enclosing function, call)] of the host-side waits in one source text; the enclosing function is the last definition that
    began in column 0."""
    fn, out = None, []
    for line in text.splitlines():
        m = FUNC.match(line)
        if m and m.group(1) not in NOT_A_FUNCTION:
            fn = m.group(1)
        out += [(name, fn, w.group(1)) for w in WAIT.finditer(line.split("//")[0])]
    return out


def _header():
    with open(os.path.join(ROOT, "include", "si_hip.h")) as f:
        return f.read()


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))


# ------------------------------------------------------------------------------------------------------------ the entry points
def test_every_entry_point_with_a_stream_is_in_exactly_one_table():
    decl = declarations(_header())
    assert len(decl) >= 70 and "si_create" in decl and "si_mend_runs" in decl, len(decl)
    streamed = {n for n, args in decl.items() if "si_stream_t" in args}
    assert len(streamed) >= 50 and "si_create" not in streamed
    both = set(S.COVERED) & set(S.EXEMPT)
    assert not both, f"in both tables: {sorted(both)}"
    listed = set(S.COVERED) | set(S.EXEMPT)
    assert not streamed - listed, f"declared with a si_stream_t and in neither table of tests/side_stream.py: {sorted(streamed - listed)}"
    assert not listed - streamed, f"in a table of tests/side_stream.py and not declared with a si_stream_t: {sorted(listed - streamed)}"
    for name, case in S.COVERED.items():
        assert isinstance(case, str) and case.strip(), name
    for name, reason in S.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 3, (name, "an exemption states its reason")
    assert len(S.EXEMPT) <= 3


def test_the_header_parser_sees_a_declaration_that_spans_lines_and_skips_comments():
    decl = declarations("""/* int si_in_a_comment(si_ctx* c, si_stream_t s); */
int si_one(si_ctx* ctx, const float* x,
           si_stream_t stream);
size_t si_two(const si_f0enc_desc* d);
typedef void* si_stream_t;
""")
    assert set(decl) == {"si_one", "si_two"} and "si_stream_t" in decl["si_one"] and "si_stream_t" not in decl["si_two"]


# ------------------------------------------------------------------------------------------------------------ the waits
def test_every_host_side_wait_is_classified():
    found = []
    for path in _sources():
        with open(path) as f:
            found += waits(os.path.basename(path), f.read())
    assert len(_sources()) >= 15 and found
    table = [w[:3] for w in S.WAITS]
    assert len(set(table)) == len(table), "a wait is listed twice"
    for w in S.WAITS:
        assert len(w) == 4 and w[3] in S.WAIT_REASONS, w
    assert S.WAIT_REASONS == ("setup", "growth", "slot reuse", "profile stop")
    new = sorted(set(found) - set(table))
    assert not new, f"host-side waits that tests/side_stream.py does not classify (file, function, call): {new}"
    gone = sorted(set(table) - set(found))
    assert not gone, f"waits listed in tests/side_stream.py that the sources no longer hold: {gone}"
    # one wait per (function, call): a second one in the same function would hide behind the first
    assert len(found) == len(set(found)), sorted(w for w in set(found) if found.count(w) > 1)
    # the three a pass can meet are the ones the header names
    met = {w[1]: w[3] for w in S.WAITS if w[3] in ("growth", "slot reuse")}
    assert met == {"si_kmeans_assign": "growth", "det_scratch_reserve": "growth", "vl_upload": "slot reuse"}


def test_the_wait_parser_sees_a_new_wait_and_names_its_function():
    text = """static int helper(si_ctx* ctx, hipStream_t st) {
    // hipStreamSynchronize(st) in a comment is no wait
    SI_HIP_CHECK(hipMemcpyAsync(a, b, n, hipMemcpyDeviceToDevice, st));
    if (x) { SI_HIP_CHECK(hipStreamSynchronize(st)); }
    return 0;
}
int si_entry(si_ctx* ctx, const float* x,
             si_stream_t stream) {
    for (int i = 0; i < 3; ++i) (void)hipMemcpy(&v, p, 4, hipMemcpyDeviceToHost);
    hipDeviceSynchronize();
}
"""
    assert waits("f.hip", text) == [("f.hip", "helper", "hipStreamSynchronize"), ("f.hip", "si_entry", "hipMemcpy"), ("f.hip", "si_entry", "hipDeviceSynchronize")]


def test_the_slot_count_is_the_library_s():
    with open(os.path.join(CSRC, "api.hip")) as f:
        m = re.search(r"static constexpr int VL_SLOTS = (\d+);", f.read())
    assert m and int(m.group(1)) == S.VL_SLOTS


def test_the_header_and_the_integration_notes_name_the_waits():
    for path in (os.path.join(ROOT, "include", "si_hip.h"), os.path.join(ROOT, "INTEGRATION.md")):
        with open(path) as f:
            text = " ".join(f.read().split())
        assert "never synchronises it" not in text, path
        for words in ("enqueues all work on the caller's HIP stream", "grow", "pinned slot", "si_profile_stop"):
            assert words in text, (path, words)


# ------------------------------------------------------------------------------------------------------------ the harness, off the device
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int16, torch.uint8, torch.int64])
def test_the_default_decoy_is_finite_differs_and_keeps_an_integer_inside_its_values(dtype):
    g = torch.Generator().manual_seed(3)
    if dtype.is_floating_point:
        t = torch.randn(5, 7, generator=g).to(dtype)
        t[0, 0], t[1, 1], t[2, 2] = float("nan"), float("inf"), float("-inf")
    else:
        t = torch.randint(0, 11, (5, 7), generator=g).to(dtype)
    d = S.default_decoy(t)
    assert d.shape == t.shape and d.dtype == t.dtype and d.is_contiguous() and not torch.equal(d, t)
    if dtype.is_floating_point:
        assert bool(torch.isfinite(d).all())
    elif dtype in (torch.int64, torch.uint8):
        assert sorted(d.reshape(-1).tolist()) == sorted(t.reshape(-1).tolist())


def test_first_difference_names_the_first_flat_index():
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    b = a.clone()
    assert S.first_difference("out", a, b, "x") is None
    b[1, 2], b[2, 3] = -1.0, float("nan")
    msg = S.first_difference("out", a, b, "behind a delay on a side stream")
    assert msg == "out: behind a delay on a side stream changes 2 of 12 elements, the first at flat index 6: 6.0 -> -1.0"
    assert S.first_difference("z", torch.tensor([0.0]), torch.tensor([-0.0]), "x") is not None           # bits, not values
    assert "shape" in S.first_difference("out", a, a[:2], "x")
    assert S.first_difference("e", torch.zeros(0), torch.zeros(0), "x") is None


def test_as_dict_takes_what_a_pass_returns():
    t = torch.zeros(2)
    assert list(S.as_dict(t)) == ["out"]
    assert list(S.as_dict((t, None, t))) == ["out0", "out2"]
    assert list(S.as_dict({"a": t, "n": 3, "rows": [t]})) == ["a"]


def test_shared_family_routes_name_families_of_the_two_lists():
    from tests import poison as P
    for fam, routes in S.SHARED_FAMILY_ROUTES.items():
        assert fam in P.SCRATCH_FAMILIES or fam in P.NO_SCRATCH_FAMILIES, fam
        assert len(routes) >= 2 and len(set(routes)) == len(routes), fam
