"""tests/harness.py's host parts: the scoped environment restores what it found, the summary of ratios keys, collapses and fails as
the GPU files rely on.  No GPU."""
import os

import pytest

from tests.harness import RatioSummary, scoped_env

SET, UNSET = "SI_HARNESS_TEST_SET", "SI_HARNESS_TEST_UNSET"


@pytest.mark.parametrize("raises", [False, True])
def test_scoped_env_restores_a_set_variable_and_removes_an_unset_one(raises, monkeypatch):
    monkeypatch.setenv(SET, "before")
    monkeypatch.delenv(UNSET, raising=False)
    try:
        with scoped_env({SET: "inside", UNSET: "inside"}):
            assert os.environ.get(SET) == "inside" and os.environ.get(UNSET) == "inside"
            if raises:
                raise KeyError("the body fails")
    except KeyError:
        assert raises
    assert os.environ.get(SET) == "before" and UNSET not in os.environ


def test_summary_groups_keys_and_collapses_the_fp16_tap_gemm_family(capsys):
    s = RatioSummary()
    s.note("respair_f16_c32", 0.5, 0.25)
    s.note("respair_f16_c32", 0.25, 0.75)
    s.group = "u=5 k=11 fp16"
    s.note("tapgemm_f16_128x64", 0.125, 0.5)
    s.note("tapgemm_f16_128x64+tapgemm_f16_256x32", 0.75, 0.25)
    s.note("tapgemm_f32_128x64", 0.0625, 0.03125)                 # the fp32 / bf16x3 / bf16 configurations keep a line each
    assert s.rows == {"respair_f16_c32": [0.5, 0.75, 2], "u=5 k=11 fp16 | tapgemm_f16_*": [0.75, 0.5, 2],
                      "u=5 k=11 fp16 | tapgemm_f32_128x64": [0.0625, 0.03125, 1]}
    s.report()
    assert capsys.readouterr().out.splitlines() == [
        "   SUMMARY respair_f16_c32: max err/E seam+edge rows 0.5000, interior 0.7500 over 2 checks",
        "   SUMMARY u=5 k=11 fp16 | tapgemm_f16_*: max err/E seam+edge rows 0.7500, interior 0.5000 over 2 checks",
        "   SUMMARY u=5 k=11 fp16 | tapgemm_f32_128x64: max err/E seam+edge rows 0.0625, interior 0.0312 over 1 checks"]


def test_summary_prints_at_its_own_precision_and_in_a_given_order(capsys):
    s = RatioSummary(digits=3)
    s.note("conv_post", 0.004, 0.005)
    s.report()
    s.note("spec", 0.5, 0.25)
    s.report("{key}: {near:.6f} | {rest:.6f}", keys=("spec", "logmel", "conv_post"))
    assert capsys.readouterr().out.splitlines() == ["   SUMMARY conv_post: max err/E seam+edge rows 0.004, interior 0.005 over 1 checks",
                                                    "spec: 0.500000 | 0.250000", "conv_post: 0.004000 | 0.005000"]


@pytest.mark.parametrize("near,rest", [(1.0000001, 0.5), (0.5, 1.5), (float("inf"), 0.0)])
def test_summary_fails_when_a_ratio_exceeds_one(near, rest):
    s = RatioSummary()
    s.note("respair_f16_c64", 1.0, 1.0)                            # (at the bound: passes)
    s.report()
    s.note("respair_f16_c64_acc", near, rest)
    with pytest.raises(AssertionError):
        s.report()
