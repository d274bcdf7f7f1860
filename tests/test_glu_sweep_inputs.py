"""Host only: the float64 truth and the intervals of tests/_glu_sweep.py, validated by means other than themselves -- the
derivative against a central difference, GeGLU against log_ndtr, finiteness on every finite input, the share of intervals
that are ONE value (what keeps an interval from hiding a failure), the fp32 CPU restatement (oracle/ref_ops.py) inside
everywhere, and wrong variants outside."""
import pytest
import torch

from oracle import ref_ops as R
from tests import _glu_sweep as S

F64 = torch.float64
NAMES = ("bf16", "fp16", "fp32")


@pytest.mark.parametrize("act", S.ACTS)
def test_derivative_agrees_with_a_central_difference(act):
    """D against (F(e + d) - F(e - d)) / 2d in float64, d = 2^-21 max(1, |e|) <= 1.9e-5 on |e| <= 40: the truncation
    d^2 |F'''| / 6 (|F'''| of order 1 for all four) and the cancellation 2^-53 |F| / d are each a few 1e-10; asserted at 1e-8"""
    e = torch.linspace(-40.0, 40.0, 32001, dtype=F64)
    d = 2.0 ** -21 * e.abs().clamp(min=1.0)
    _, D = S.truth(act, e)
    num = (S.truth(act, e + d)[0] - S.truth(act, e - d)[0]) / (2.0 * d)
    assert float((D - num).abs().max()) < 1e-8


def test_geglu_exact_agrees_with_log_ndtr():
    e = torch.cat([S.all_values("fp16")["finite"].double(), S.all_values("bf16")["finite"].double()])
    F, _ = S.truth("geglu_exact", e)
    ln = torch.special.log_ndtr(e)
    other = torch.where(e == 0, e, e * torch.exp(ln))
    # exp() turns the half-ulp of its argument into a relative |ln| 2^-53; a few ulps for erfc, exp and the products; denormals
    ok = (F - other).abs() <= 16 * 2.0 ** -53 * (1.0 + ln.abs()) * other.abs() + 1e-290
    assert bool(ok.all()), S.describe(~ok, e, F, other, other)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act", S.ACTS)
def test_truth_is_finite_on_every_finite_input(act, name):
    e = S.finite_values(name).double()
    F, D = S.truth(act, e)
    assert bool(torch.isfinite(F).all()) and bool(torch.isfinite(D).all())
    uf, ud = S._units(act, e, F)
    assert bool(torch.isfinite(uf).all()) and bool(torch.isfinite(ud).all())


def test_the_sweeps_are_what_they_claim():
    for name, n_finite in (("bf16", 65280), ("fp16", 63488)):
        v = S.all_values(name)
        assert v["finite"].numel() == n_finite and v["inf"].numel() == 2 and v["nan"].numel() == 65536 - n_finite - 2
    f = S.fp32_values()
    assert bool(torch.isfinite(f).all()) and f.numel() == torch.unique(f.view(torch.int32)).numel()
    for name in ("bf16", "fp16"):                        # every 16-bit value is in the fp32 sweep
        assert torch.isin(S.all_values(name)["finite"].float().view(torch.int32), f.view(torch.int32)).all()
    for name in NAMES:                                   # the (g, DW) values are exact in the dtype
        for g, dw in S.pairs(name):
            for x in (g, dw):
                assert float(torch.tensor(x, dtype=F64).to(S.DTYPES[name]).double()) == x and abs(x) <= 2.0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act", S.ACTS)
def test_most_intervals_are_one_value(act, name):
    """On |e| <= 64, with the C in force, at least 0.8 of the intervals admit exactly one value of the dtype (fp32: the interval
    is the tolerance, and one value is not to be expected)."""
    shares = S.single_share(act, name)
    if name == "fp32":
        return
    for out, s in shares.items():
        assert s >= 0.8, (act, name, out, s)


def _oracle_outputs(act, dt, e, g, dw):
    gt, dwt = torch.full_like(e, g), torch.full_like(e, dw)
    if act == "quick_gelu":
        return {"y": R.quick_gelu_forward(e), "dx": R.quick_gelu_backward(dwt, e)}
    h = R.glu_forward(e, gt, act)
    h2, df, de = R.glu_backward(dwt, e, gt, act)
    return {"h": h, "h_bwd": h2, "df": df, "de": de}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act", S.ACTS)
def test_the_fp32_cpu_restatement_lies_inside(act, name):
    e = S.finite_values(name)
    for g, dw in S.pairs(name):
        iv = S.intervals(act, name, e, g, dw)
        for out, got in _oracle_outputs(act, S.DTYPES[name], e, g, dw).items():
            lo, hi = iv["h" if out == "h_bwd" else out]
            assert not bool(torch.isnan(got.float()).any()), (act, name, out, "NaN on a finite input")
            ok = S.inside(got, lo, hi, name)
            assert bool(ok.all()), (act, name, out, g, dw, int((~ok).sum()), S.describe(~ok, e.double(), got.double(), lo, hi))


@pytest.mark.parametrize("name", ("bf16", "fp16"))
@pytest.mark.parametrize("act", S.ACTS)
def test_one_ulp_off_falls_outside_where_the_interval_is_one_value(act, name):
    e = S.finite_values(name)
    iv = S.intervals(act, name, e)
    for out, got in _oracle_outputs(act, S.DTYPES[name], e, 1.0, 1.0).items():
        lo, hi = iv["h" if out == "h_bwd" else out]
        single = (lo == hi) & torch.isfinite(lo)
        for up in (True, False):
            wrong = S.one_ulp_off(got, up)
            moved = single & torch.isfinite(wrong.double()) & (wrong.double() != got.double())
            assert int(moved.sum()) > 0.5 * e.numel()
            assert not bool((S.inside(wrong, lo, hi, name) & moved).any()), (act, name, out, up)


@pytest.mark.parametrize("name", ("bf16", "fp16"))
def test_swiglu_derivative_without_one_minus_se_falls_outside(name):
    e = S.finite_values(name)
    lo, hi = S.intervals("swiglu", name, e)["de"]
    wrong = S.swiglu_d_without_one_minus_se(e.double()).float().to(S.DTYPES[name])
    ok = S.inside(wrong, lo, hi, name)
    # the slip changes D by e se^2: on 1/4 <= |e| <= 4 that is at least 2 % of D, several bf16 ulps (further out on the negative
    # side se falls below the dtype's resolution and the two really round alike)
    a = e.double().abs()
    body = (a >= 0.25) & (a <= 4.0)
    assert float((~ok)[body].double().mean()) > 0.9, float((~ok)[body].double().mean())
