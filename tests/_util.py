"""Shared helpers of the test-suite (not a test module)."""
import torch

EPS = {torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def assert_ulp(actual, expected, dtype, ulps=1.0, atol=None, what="", allow_frac=0.0):
    """|actual - expected| <= ulps * eps(dtype) * |expected| + atol elementwise. `allow_frac` tolerates a
    fraction of elements at 2x the bound (transcendental implementations differ in the last fp32 bit,
    which can flip a rounding to the 16-bit dtype)."""
    a = actual.detach().float().cpu()
    b = expected.detach().float().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    assert torch.isfinite(a).all(), f"{what}: non-finite values in result"
    eps = EPS[dtype]
    if atol is None:
        atol = eps * float(b.abs().mean() + 1e-30) * 0.5
    bound = ulps * eps * b.abs() + atol
    err = (a - b).abs()
    bad = err > bound
    if bad.any():
        worse = err > 2 * bound
        frac = float(bad.float().mean())
        idx = torch.nonzero(bad)[0].tolist()
        msg = (f"{what}: {int(bad.sum())}/{bad.numel()} beyond {ulps} ulp ({frac:.2e}); first at {idx}: "
               f"got {a[tuple(idx)].item()!r} want {b[tuple(idx)].item()!r}; max err {err.max().item():.4e}")
        assert not worse.any() and frac <= allow_frac, msg


def rel_fro(actual, expected):
    a = actual.detach().float().cpu()
    b = expected.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- AdamW: an fp64 reference, the kernels' fp32 arithmetic restated, and the comparison both feed -----------------------
def adamw_ref64(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=1.0):
    """One AdamW step in float64 on fp32 `p, g, m, v` (any shape, any device), as the header of csrc/adamw.hip states it:
    g is scaled by `grad_scale` first, weight decay is decoupled, bc1 = 1 - b1^t, bc2_sqrt = sqrt(1 - b2^t).
    Returns (p, m, v, scale): the new float64 values and `scale`, a dict of the per-element OPERAND scale of each result --
    the magnitudes an fp32 evaluation rounds at: m: |b1 m| + |(1 - b1) g|, v: |b2 v| + |(1 - b2) g^2|,
    p: |p| + |step_size m / denom|. Pinned to torch.optim.AdamW in tests/test_optim_ref_host.py."""
    import math
    b1, b2 = betas
    p, g, m, v = (x.detach().to(torch.float64) for x in (p, g, m, v))
    g = g * grad_scale
    step_size = lr / (1.0 - b1 ** step)
    bc2_sqrt = math.sqrt(1.0 - b2 ** step)
    scale = dict(m=(b1 * m).abs() + ((1.0 - b1) * g).abs(), v=(b2 * v).abs() + ((1.0 - b2) * g * g).abs())
    pd = p - lr * weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    upd = step_size * m / (v.sqrt() / bc2_sqrt + eps)
    scale["p"] = p.abs() + upd.abs()
    return pd - upd, m, v, scale


def adamw_restated_f32(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=1.0):
    """The same step as separate fp32 torch operations in the association of csrc/adamw.hip adamw_one, every scalar formed in
    double and rounded to fp32 once, as the entry points do (lr_wd = float32(lr * wd), step_size = float32(lr / bc1),
    omb = float32(1 - beta)). What the kernels compute up to the rounding of their division and square root; written here,
    not imported from the product. Returns new fp32 (p, m, v)."""
    import math
    b1, b2 = betas
    f = lambda x: torch.tensor(float(x), dtype=torch.float64).to(torch.float32).to(p.device)
    bc1, bc2_sqrt = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    gr = g.to(torch.float32) * f(grad_scale)
    p = p - f(lr * weight_decay) * p
    m = f(b1) * m + f(1.0 - b1) * gr
    v = f(b2) * v + f(1.0 - b2) * gr * gr
    denom = v.sqrt() / f(bc2_sqrt) + f(eps)
    return p - f(lr / bc1) * m / denom, m, v


def adamw_ratio(got, want64, scale):
    """Worst |got - want64| / (2^-24 * scale) over the elements; an element whose scale is 0 must be exact."""
    err = (got.detach().to(torch.float64) - want64).abs().reshape(-1)
    unit = (scale.to(torch.float64) * 2.0 ** -24).reshape(-1)
    r = torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    r = torch.where(torch.isfinite(got.detach().reshape(-1).to(torch.float64)), r, torch.full_like(r, float("inf")))
    return r


def assert_adamw_close(got, want64, scale, ratio_bound, what=""):
    """|got - want64| <= ratio_bound * 2^-24 * scale at every element (an absolute bound at the operands' scale: a moment
    that cancels is not held to its own, smaller, magnitude); reports the worst element."""
    assert got.shape == want64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want64.shape)}"
    r = adamw_ratio(got, want64, scale)
    if r.numel() == 0:
        return 0.0
    worst = float(r.max())
    if not worst <= ratio_bound:
        i = int(r.argmax())
        raise AssertionError(f"{what}: {int((r > ratio_bound).sum())}/{r.numel()} elements beyond {ratio_bound:.3g} x 2^-24 x "
                             f"operand scale; worst at flat index {i}: got {got.reshape(-1)[i].item()!r} want "
                             f"{want64.reshape(-1)[i].item()!r} scale {scale.reshape(-1)[i].item():.6e} ratio {worst:.3f}")
    return worst
