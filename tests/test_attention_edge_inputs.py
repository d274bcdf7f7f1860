"""Host checks of the attention mask-edge inputs (tests/_attn_edges.py; the GPU side is tests/test_gpu_attention_edges.py).

The GPU tests hold every kernel output to `row_err <= 4 x the rounding model's row_err` against an fp64 reference. That bound means
something only if a mask that is off by one key moves the outputs by far more than it: here every off-by-one mask (lower / upper
edge, one key out / in) is shown to move o, dq, dk and dv by at least 3 x that bound, on the very inputs the GPU tests use. This is
a condition on the INPUTS -- a case that misses it gets another seed or other lengths, never another factor."""
import math

import pytest
import torch

from tests import _attn_edges as E

BOUND_FACTOR = E.BOUND_FACTOR   # the GPU tests' bound: row_err(kernel) <= BOUND_FACTOR x row_err(model)
assert BOUND_FACTOR == 4
MARGIN = 3              # every mutant sits at least MARGIN x above that bound


@pytest.mark.parametrize("dtype_name", list(E.DTYPES))
@pytest.mark.parametrize("name", list(E.CASES))
def test_rounding_model_is_close_to_the_fp64_reference(name, dtype_name):
    c = E.build_case(name, dtype_name)
    for t in E.TENSORS:
        assert torch.isfinite(c["ref"][t]).all() and torch.isfinite(c["model"][t]).all(), t
        e = c["model_err"][t]
        if e is None:                                  # dQ / dK under window 1: zero in the reference, rounding dust in the model
            assert c["window"] == 1 and t in ("dq", "dk") and float(c["model"][t].abs().max()) <= 1e-3
            continue
        # (how small it has to be is the next test's business: 12 x this value must stay below every mutant's effect)
        assert math.isfinite(e) and e >= 0.0, (t, e)


@pytest.mark.parametrize("dtype_name", list(E.DTYPES))
@pytest.mark.parametrize("name", list(E.CASES))
def test_every_off_by_one_mask_is_visible_above_the_bound(name, dtype_name):
    c = E.build_case(name, dtype_name)
    muts = E.mutants(c["lo"], c["hi"], c["causal"])
    assert muts, "no mutant differs from the true mask"
    names = [n for n, _ in muts]
    # (lo = 0 everywhere leaves nothing below the lower edge; window 1 leaves no edge to pull in)
    assert names == [n for n in ("lo-1", "lo+1", "up+1", "up-1")
                     if not (n == "lo-1" and int(c["lo"].max()) == 0) and not (n in ("lo+1", "up-1") and c["window"] == 1)]
    # window 1: P = 1 on the diagonal, dS = P (dP - Delta) = 0 and with it dQ and dK, identically -- nothing to compare against
    tensors = ("o", "dv") if c["window"] == 1 else ("o", "dq", "dk", "dv")
    seen = {}
    for mname, allowed in muts:
        got = dict(zip(E.TENSORS, E.ref64(c["q"], c["k"], c["v"], c["do"], c["scale"], allowed)))
        for t in tensors:
            seen[(mname, t)] = (E.row_err(got[t], c["ref"][t]), MARGIN * BOUND_FACTOR * c["model_err"][t])
    print({k: (round(a, 4), round(b, 5)) for k, (a, b) in seen.items()})
    for key, (effect, need) in seen.items():
        assert effect >= need, (key, effect, need)


def test_window_one_has_zero_dq_and_dk():
    c = E.build_case("win1", "bf16")
    assert float(c["ref"]["dq"].abs().max()) <= 1e-12 and float(c["ref"]["dk"].abs().max()) <= 1e-12


def test_allowed_from_band_on_hand_written_rows():
    lo = torch.tensor([[0, 0, 1, 3]])
    hi = torch.tensor([[0, 2, 2, 3]])
    causal = E.allowed_from_band(lo, hi, True)[0, 0].int().tolist()
    assert causal == [[1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 0, 1]]
    both = E.allowed_from_band(lo, hi, False)[0, 0].int().tolist()
    assert both == [[1, 0, 0, 0], [1, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 1]]


def test_mutants_on_hand_written_rows():
    lo = torch.tensor([[0, 0, 1, 3]])
    hi = torch.tensor([[0, 2, 2, 3]])
    m = dict(E.mutants(lo, hi, True))
    assert m["lo-1"][0, 0].int().tolist() == [[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0], [0, 0, 1, 1]]
    assert m["lo+1"][0, 0].int().tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]     # empty rows keep the diagonal
    assert m["up+1"][0, 0].int().tolist() == [[1, 1, 0, 0], [1, 1, 1, 0], [0, 1, 1, 1], [0, 0, 0, 1]]     # clamped at T - 1
    assert m["up-1"][0, 0].int().tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]
    one = torch.arange(4)[None]
    assert [n for n, _ in E.mutants(one, one, True)] == ["lo-1", "up+1"]


def test_attention_band_causal_window_packed_on_hand_written_rows():
    """attention_band with documents AND a sliding window AND two batch rows: lengths [3, 4, 5] over 2 x 6 tokens, window 3. The
    second document (flat 3 .. 6) is cut at the row boundary, the third is flat 7 .. 11 = positions 1 .. 5 of row 1."""
    from unsloth_amd.kernels.attention import attention_band
    lo, hi = attention_band(6, batch=2, seq_lengths=[3, 4, 5], sliding_window=3)
    assert lo.tolist() == [[0, 0, 0, 3, 3, 3], [0, 1, 1, 1, 2, 3]]
    assert hi.tolist() == [[2, 2, 2, 5, 5, 5], [0, 3, 4, 5, 5, 5]]
    want = [[1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 1]]
    assert E.allowed_from_band(lo, hi, True)[0, 0].int().tolist() == want
    want = [[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 1, 1, 1, 0, 0], [0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1]]
    assert E.allowed_from_band(lo, hi, True)[1, 0].int().tolist() == want


def test_document_band_on_hand_written_rows():
    from unsloth_amd.kernels.attention import document_band
    lo, hi = document_band(5, batch=2, seq_lengths=[2, 4, 1])                        # the second document is cut after flat 4
    assert lo.tolist() == [[0, 0, 2, 2, 2], [0, 1, 2, 2, 2]] and hi.tolist() == [[1, 1, 4, 4, 4], [0, 1, 4, 4, 4]]
    want = [[1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1]]
    assert E.allowed_from_band(lo, hi, False)[0, 0].int().tolist() == want


@pytest.mark.parametrize("name", list(E.CASES))
def test_band_builders_agree_with_the_helper_on_every_case(name):
    """The GPU tests hand the kernels the product's band and judge them by the helper's dense mask: the two must be the same band."""
    from unsloth_amd.kernels.attention import attention_band, document_band
    B, T, Hq, Hk, D, lengths, window, causal = E.CASES[name]
    lo, hi = E.case_band(B, T, lengths, window, causal)
    if causal:
        plo, phi = attention_band(T, batch=B, seq_lengths=lengths, sliding_window=window)
    else:
        plo, phi = document_band(T, batch=B, seq_lengths=lengths)
    assert torch.equal(plo.long(), lo) and torch.equal(phi.long(), hi)
