"""CPU: the host reference the device sampler is judged against (tests/_sampler_ref.py) -- its Philox reproduces the Random123
known answers, its kept set is HF's warper chain TopK -> TopP -> MinP (and `filter_logits`) wherever no tie sits on a boundary,
and every input of tests/test_gpu_sampler.py keeps its boundaries at least 1e-4 away from the nearest token, so fp32 against
fp64 rounding cannot move a token across them."""
import numpy as np
import pytest
import torch

from tests import _sampler_ref as R

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert " ".join(f"{w:08x}" for w in R.philox4x32_10(ctr, key)) == want


def test_uniform_is_the_top_24_bits_of_the_first_word():
    x0 = R.philox4x32_10((5, 1, 3, 0), (0x89ABCDEF, 0xFEDCBA98))[0]
    u = R.uniform(0xFEDCBA9889ABCDEF, (1 << 32) + 5, 3)
    assert u.dtype == np.float32 and float(u) == (x0 >> 8) / 2.0 ** 24 and 0.0 <= float(u) < 1.0


@pytest.mark.parametrize("V,si", R.CASES)
def test_gpu_case_margins(V, si):
    c = R.case(V, si)
    assert c["margins"], "a case without a boundary"
    for name, gap in c["margins"].items():
        assert gap >= R.MARGIN, (name, gap, "take another seed for this case: _sampler_ref.SEED_OF")
    if c["m"] and not c["min_p"]:
        assert int(c["keep"].sum()) == c["m"]
    assert c["keep"][int(np.argmax(c["z"]))]


@pytest.mark.parametrize("k,m", R.CROWDED)
def test_crowded_case_margins_and_one_first_digit(k, m):
    c = R.crowded_case(k, m)
    assert all(gap >= R.MARGIN for gap in c["margins"].values()) and c["margins"]
    assert int(c["keep"].sum()) == (m or k) and np.array_equal(c["keep"], _hf_keep(c))
    bits = c["z"].view(np.uint32)
    assert len(set((bits >> 24).tolist())) == 1 and c["V"] > 16384       # sign + 7 exponent bits: the kernel's first digit


def _hf_keep(c):
    from transformers.generation.logits_process import (MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    s = torch.from_numpy(c["x"].copy())[None]
    if c["T"] != 1.0:
        s = TemperatureLogitsWarper(c["T"])(None, s)
    assert np.array_equal(s[0].numpy(), c["z"]), "the reference's z is not HF's scaled logit"
    if 0 < c["top_k"] < c["V"]:
        s = TopKLogitsWarper(c["top_k"])(None, s)
    if c["top_p"] < 1.0:
        s = TopPLogitsWarper(c["top_p"])(None, s)
    if c["min_p"] > 0.0:
        s = MinPLogitsWarper(c["min_p"])(None, s)
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("V,si", R.CASES)
def test_kept_set_is_hf_warper_chain(V, si):
    c = R.case(V, si)
    assert np.array_equal(c["keep"], _hf_keep(c))


@pytest.mark.parametrize("V,si", [(V, si) for V, si in R.CASES if V in (1001, 128256)])
def test_filter_logits_keeps_the_same_set(V, si):
    from unsloth_amd.models.decode import filter_logits
    c = R.case(V, si)
    out = filter_logits(torch.from_numpy(c["z"].copy())[None], c["top_k"], c["top_p"], c["min_p"])
    assert np.array_equal(torch.isfinite(out[0]).numpy(), c["keep"])


def test_filter_logits_min_p_default_changes_nothing():
    from unsloth_amd.models.decode import filter_logits
    z = torch.from_numpy(R.case(1000, 3)["z"].copy())[None]
    assert torch.equal(filter_logits(z, 50, 0.9), filter_logits(z, 50, 0.9, 0.0))


def test_ties_stay_or_go_as_a_group():
    z = np.full(40, -3.0, np.float32)
    z[5:15] = 2.0                                    # ten equal values across the top-k boundary
    z[20] = 4.0
    keep = R.kept_set(z, top_k=4)
    assert keep.sum() == 11 and keep[5:15].all() and keep[20]
    # 0.5, then four tokens of 0.1 each, then 0.1 spread thinly: top_p = 0.75 cuts through the tied four; they stay whole
    p = np.array([0.5, 0.1, 0.1, 0.1, 0.1] + [0.01] * 10)
    keep = R.kept_set(np.log(p).astype(np.float32), top_p=0.75)
    assert keep.sum() == 5
    keep = R.kept_set(np.log(p).astype(np.float32), top_p=0.45)
    assert keep.sum() == 1


def test_special_values_are_never_kept():
    z = np.array([1.0, -np.inf, np.nan, 0.5, np.inf], np.float32)
    assert R.kept_set(z).tolist() == [True, False, False, True, False]
    assert not R.kept_set(np.full(4, -np.inf, np.float32)).any()


def test_cdf_intervals_partition_the_unit_interval():
    c = R.case(4099, 3)
    a, b = R.cdf_intervals(c["z"], c["keep"])
    idx = np.nonzero(c["keep"])[0]
    assert a[idx[0]] == 0.0 and b[idx[-1]] == 1.0 and np.abs(a[idx[1:]] - b[idx[:-1]]).max() < 1e-15
    assert np.isnan(a[~c["keep"]]).all()
