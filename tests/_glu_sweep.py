"""Helpers of the gated-activation sweep (tests/test_glu_sweep_inputs.py on the host, tests/test_gpu_glu_sweep.py on the GPU, which
also writes the measured figures to its report): every 16-bit input of SwiGLU, GeGLU (erf), GeGLU (tanh) and QuickGELU
(csrc/glu.hip act_fwd / act_bwd / fwd_one / bwd_one / quick_gelu_kernel and the two SwiGLU copies of csrc/decode.hip), a float64
truth of each function and of its derivative, and the INTERVAL of values a correct kernel may return. Nothing here runs a
kernel, and the truth imports neither the product nor oracle/ref_ops.

The check. The kernels evaluate f(e) and f'(e) in fp32 and round where the reference rounds (glu.hip's header): f to the
activation dtype T, then h = f * g, df = DW * f and dg = DW * g as products IN T, then de = dg * f'(e) in fp32 rounded once.
Round-to-nearest is monotone, so if the fp32 f is within delta_f of the truth F, rt(f) lies in [rt(F - delta_f), rt(F + delta_f)]
= [flo, fhi]; h lies between rt(flo g) and rt(fhi g) (f g is exact in fp32: two significands of at most 11 bits, or one
rounding for T = fp32), df likewise with DW, dg = rt(DW g) is exact in the model, and de lies between the roundings of
dg (D -+ delta_d). The kernel's output must lie in the closed interval -- no ulp allowance, no share of elements let off. Where
the interval is one value, which is most elements (single_share), the assertion is bit-exact.

delta = C 2^-24 unit(e) + floor. `unit` is how the formula AS WRITTEN in glu.hip amplifies one fp32 rounding (_units), the floor
is the fp32 underflow of the sigmoid, and C is measured on the device (profiles/glu_sweep_report.json) and then fixed at twice
the measured worst rounded up to a power of two (C_IN_FORCE)."""
import math

import torch

F64 = torch.float64
ACTS = ("swiglu", "geglu_exact", "geglu_approx", "quick_gelu")
GLU_ACTS = ACTS[:3]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MANT = {"bf16": 8, "fp16": 11, "fp32": 24}                      # significand bits, the hidden one included
EMIN = {"bf16": -126, "fp16": -14, "fp32": -126}                # exponent of the smallest normal number
MAX32 = float(torch.finfo(torch.float32).max)
TINY32 = 2.0 ** -126
EPS32 = 2.0 ** -24
SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)
QG = 1.702

# C per (activation, kind): kind "f" governs the outputs made of f (h, df; QuickGELU's y), "d" those made of f' (de; dx).
# Measured on an MI355X by tests/test_gpu_glu_sweep.py (the worst over the streaming kernels, bf16 / fp16 / fp32, g = DW = 1);
# in force = twice the measured worst, rounded up to a power of two.                      measured worst
C_IN_FORCE = {
    ("swiglu", "f"): 4.0,            # 1.88  (fp32, e = -0.0043)
    ("swiglu", "d"): 4.0,            # 1.22  (fp32, e = -0.0028)
    ("geglu_exact", "f"): 4.0,       # 1.12  (fp32, e = 1.0039)
    ("geglu_exact", "d"): 4.0,       # 1.37  (fp32, e = 1.3418)
    ("geglu_approx", "f"): 4.0,      # 1.13  (fp32, e = 0.9312)
    ("geglu_approx", "d"): 4.0,      # 1.41  (fp32, e = -5.4219: |u| = 10, where the unit falls to 1)
    ("quick_gelu", "f"): 4.0,        # 1.96  (fp32, e = -0.6865)
    ("quick_gelu", "d"): 4.0,        # 1.11  (fp32, e = 5.1133)
}


# ---------------------------------------------------------------------------------------------------------------- the truth
def _sig(x):
    """sigmoid in float64 without the 1 - s cancellation: callers take _sig(-x) for 1 - sigmoid(x)"""
    return torch.sigmoid(x)


def truth(act, e):
    """(F, D = dF/de) in float64 for float64 e; finite for every finite e. Forms that do not cancel on the negative side:
    Phi(x) = erfc(-x / sqrt 2) / 2, (1 + tanh u) / 2 = sigmoid(2 u), 1 - sigmoid(x) = sigmoid(-x)."""
    e = e.to(F64)
    if act in ("swiglu", "quick_gelu"):
        k = 1.0 if act == "swiglu" else QG
        s, sm = _sig(k * e), _sig(-k * e)
        return e * s, s + (k * e * s) * sm
    if act == "geglu_exact":
        phi_c = 0.5 * torch.special.erfc(-e / math.sqrt(2.0))
        pdf = torch.exp(-0.5 * e * e) / math.sqrt(2.0 * math.pi)
        return e * phi_c, phi_c + e * pdf
    if act == "geglu_approx":
        u2 = 2.0 * SQRT_2_OVER_PI * e * (1.0 + 0.044715 * e * e)
        du2 = 2.0 * SQRT_2_OVER_PI * (1.0 + 3.0 * 0.044715 * e * e)
        s, sm = _sig(u2), _sig(-u2)
        # e * du2 reaches 1e115 in float64 and sm is exactly 0 long before: multiply the bounded factors first
        return e * s, s + (s * sm) * (e * du2)
    raise ValueError(act)


def _units(act, e, F):
    """(unit_f, unit_d): the absolute error of the fp32 formula per 2^-24, up to the constant C.
    SwiGLU, f = e / (1 + __expf(-e)): __expf scales its argument by log2(e) before v_exp_f32, so exp(-e) carries a RELATIVE
      error of |e| 2^-24; the quotient and the product add a few 2^-24 relative: |F| max(1, |e|).
      f' = se (1 + e (1 - se)): 1 - se cancels for e > 0 (absolute error 2^-24) and is multiplied by e: 1 + max(e, 0); for
      e < 0 the relative error |e| 2^-24 of se meets |f'| <= e^-|e| (1 + |e|): below 1.
    GeGLU erf, f = 0.5 e (erf(e / sqrt 2) + 1): the sum carries an ABSOLUTE error 2^-24 (all of it where erf -> -1): |e|.
      f' = Phi + t e __expf(-e^2 / 2): Phi absolute 2^-24; the second term is at most 0.25 with a relative error e^2 / 2 * 2^-24
      that the factor e^-(e^2 / 2) outruns: 1.
    GeGLU tanh, f = 0.5 e (tanh(u) + 1): as above, |e|.
      f' = T2 + P (a + 3 b) with T = 1 + tanh(u), P = -T2 (T - 2): T and T - 2 each carry an absolute 2^-24 and the product
      is multiplied by a + 3 b: 1 + |a + 3 b| -- while tanh is not saturated. From |u| = 10 on, 1 - |tanh u| < 2^-27: a tanhf
      good to an ulp returns +-1 exactly, P is exactly 0 and a + 3 b multiplies no error at all; what is left is the true
      P |a + 3 b| that the kernel drops (below 1e-6): 1 + P |a + 3 b| + [|u| < 10] |a + 3 b|. (With the first form alone the
      interval of de is wider than the function's range from |e| ~ 1e3 on and rejects only NaN.)
    QuickGELU: SwiGLU with 1.702 v in the sigmoid's argument.
    Computed in float64 and clamped to the largest finite fp32 (|F| |e| alone reaches 1e77 for bf16 inputs)."""
    a = e.abs()
    if act in ("swiglu", "quick_gelu"):
        x = e if act == "swiglu" else QG * e
        uf = F.abs() * x.abs().clamp(min=1.0)
        ud = 1.0 + x.clamp(min=0.0)
    elif act == "geglu_exact":
        uf, ud = a.clone(), torch.ones_like(a)
    else:
        aa = SQRT_2_OVER_PI * e
        b = aa * 0.044715 * e * e
        u, w = aa + b, (aa + 3.0 * b).abs()
        p_true = 2.0 * _sig(2.0 * u) * _sig(-2.0 * u)
        w_live = torch.where(u.abs() < 10.0, w, torch.zeros_like(w))
        uf, ud = a.clone(), 1.0 + (p_true * w.clamp(max=MAX32)).clamp(max=MAX32) + w_live
    return uf.clamp(max=MAX32), ud.clamp(max=MAX32)


def _floor(e):
    """fp32 underflow of the sigmoid (v_exp_f32 and v_rcp_f32 flush denormals) times the factor e of f, plus the flush itself"""
    return e.abs() * TINY32 + TINY32


def deltas(act, e, C=None):
    """(F, D, delta_f, delta_d) in float64 for float64 e"""
    F, D = truth(act, e)
    uf, ud = _units(act, e, F)
    cf = (C or C_IN_FORCE)[(act, "f")]
    cd = (C or C_IN_FORCE)[(act, "d")]
    fl = _floor(e)
    return F, D, cf * EPS32 * uf + fl, cd * EPS32 * ud + fl


# --------------------------------------------------------------------------------------------------------------- the inputs
def all_values(name):
    """every bit pattern of bf16 / fp16 as that dtype: dict(finite=, inf=, nan=), ascending bit pattern"""
    dt = DTYPES[name]
    assert dt.itemsize == 2
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    f = v.float()
    return dict(finite=v[torch.isfinite(f)], inf=v[torch.isinf(f)], nan=v[torch.isnan(f)])


def fp32_values():
    """the fp32 sweep: both 16-bit sets widened, plus the fp32 neighbours of those with 2^-4 <= |e| <= 2^7"""
    base = torch.cat([all_values("bf16")["finite"].float(), all_values("fp16")["finite"].float()])
    mid = base[(base.abs() >= 2.0 ** -4) & (base.abs() <= 2.0 ** 7)]
    inf = torch.full_like(mid, float("inf"))
    allv = torch.cat([base, torch.nextafter(mid, inf), torch.nextafter(mid, -inf)])
    bits = torch.unique(allv.view(torch.int32))                 # by bit pattern: keeps -0 beside +0
    return bits.view(torch.float32)


def finite_values(name):
    return fp32_values() if name == "fp32" else all_values(name)["finite"]


def mid_values(name):
    """the finite values with 2^-4 <= |e| <= 2^7 (the tail-only tensors of the position test)"""
    v = finite_values(name)
    a = v.float().abs()
    return v[(a >= 2.0 ** -4) & (a <= 2.0 ** 7)]


def pairs(name):
    """(g, DW) pairs, exact in the dtype, |.| <= 2: 1.0, a negative value, and all mantissa bits set (2 - 2^-(p-1), 1 - 2^-p)"""
    p = MANT[name]
    ones = 2.0 - 2.0 ** -(p - 1)
    return ((1.0, 1.0), (-1.5, 0.625), (ones, -0.5 * ones), (0.75, ones))


# ------------------------------------------------------------------------------------------------------------ the intervals
def rt(x64, name):
    """float64 -> the dtype -> float64. Through fp32 on purpose: the kernel's value IS an fp32 number >= the bound, hence >= the
    bound rounded to fp32 whichever way, so rounding the bound to nearest fp32 first keeps the interval valid."""
    return x64.to(torch.float32).to(DTYPES[name]).to(F64)


def _between(a, b):
    return torch.minimum(a, b), torch.maximum(a, b)


def intervals(act, name, e, g=1.0, dw=1.0, C=None):
    """{output: (lo, hi)} in float64 (members of the dtype, or +-inf) for e (tensor of the dtype), scalars g and DW.
    GLU activations: "h" (forward and backward), "df", "de". QuickGELU: "y" and "dx" (DW = dy)."""
    e64 = e.to(F64)
    F, D, d_f, d_d = deltas(act, e64, C)
    if act == "quick_gelu":
        dlo, dhi = _between(dw * (D - d_d), dw * (D + d_d))
        return {"y": (rt(F - d_f, name), rt(F + d_f, name)), "dx": (rt(dlo, name), rt(dhi, name))}
    flo, fhi = rt(F - d_f, name), rt(F + d_f, name)
    out = {}
    out["h"] = _between(rt(flo * g, name), rt(fhi * g, name))
    out["df"] = _between(rt(flo * dw, name), rt(fhi * dw, name))
    dg = rt(torch.tensor(dw, dtype=F64) * g, name)
    out["de"] = tuple(rt(x, name) for x in _between(dg * (D - d_d), dg * (D + d_d)))
    return out


def inside(got, lo, hi, name):
    """elementwise: got in [lo, hi]. +-0 compare equal; an infinite bound admits the infinity and the largest finite value of the
    dtype (a sum that reaches the overflow threshold may land on either); NaN is inside nothing."""
    big = float(torch.finfo(DTYPES[name]).max)
    g64 = got.to(F64).cpu()
    lo = torch.where(lo == float("inf"), torch.full_like(lo, big), lo)
    hi = torch.where(hi == float("-inf"), torch.full_like(hi, -big), hi)
    return (g64 >= lo) & (g64 <= hi)


def bounds_finite(lo, hi):
    return torch.isfinite(lo) & torch.isfinite(hi)


def single_share(act, name, C=None, limit=64.0):
    """{output: share of the finite inputs with |e| <= limit whose interval is one value}, from the truth alone (g = DW = 1)"""
    e = finite_values(name)
    e = e[e.float().abs() <= limit]
    return {k: float((lo == hi).double().mean()) for k, (lo, hi) in intervals(act, name, e, C=C).items()}


def describe(bad, e, got, lo, hi, limit=5):
    idx = torch.nonzero(bad).flatten()[:limit].tolist()
    return "; ".join(f"e={float(e[i]):.9g} got={float(got[i]):.9g} want [{float(lo[i]):.9g}, {float(hi[i]):.9g}]" for i in idx)


# ------------------------------------------------------------------------------------------------- measuring C from an output
def needed_c(act, kind, name, e, got):
    """For outputs computed with g = DW = 1 (h = df = rt(f), de = rt(f'), y, dx): per element the smallest C that puts `got`
    inside, i.e. (distance from the truth to the set of reals that round to `got`, less the floor) / (2^-24 unit). NaN -> inf."""
    e64 = e.to(F64)
    F, D = truth(act, e64)
    uf, ud = _units(act, e64, F)
    center, unit = (F, uf) if kind == "f" else (D, ud)
    g64 = got.to(F64).cpu()
    p, emin = MANT[name], EMIN[name]
    _, ex = torch.frexp(g64)                                     # |got| = m 2^ex, m in [0.5, 1)
    ex = torch.where(torch.isfinite(g64) & (g64 != 0), ex - 1, torch.full_like(ex, emin)).clamp(min=emin)
    ulp = torch.pow(torch.tensor(2.0, dtype=F64), (ex - (p - 1)).to(F64))
    mag = g64.abs()
    pow2 = (mag == torch.pow(torch.tensor(2.0, dtype=F64), ex.to(F64))) & (ex > emin)
    out_half, in_half = 0.5 * ulp, torch.where(pow2, 0.25 * ulp, 0.5 * ulp)     # half the gap away from / towards zero
    lo = torch.where(g64 >= 0, g64 - in_half, g64 - out_half)
    hi = torch.where(g64 > 0, g64 + out_half, g64 + in_half)
    lo = torch.where(g64 == 0, -0.5 * ulp, lo)
    hi = torch.where(g64 == 0, 0.5 * ulp, hi)
    big = float(torch.finfo(DTYPES[name]).max)
    top = big + 0.5 * 2.0 ** (math.floor(math.log2(big)) - (p - 1))
    lo = torch.where(g64 == float("inf"), torch.full_like(lo, top), lo)
    hi = torch.where(g64 == float("-inf"), torch.full_like(hi, -top), hi)
    dist = torch.maximum(torch.maximum(lo - center, center - hi), torch.zeros_like(center))
    need = (dist - _floor(e64)).clamp(min=0.0) / (EPS32 * unit.clamp(min=TINY32))
    return torch.where(torch.isnan(g64), torch.full_like(need, float("inf")), need)


# ------------------------------------------------------------------------------------------------------------ wrong variants
def one_ulp_off(x, up=True):
    """every finite, non-extreme element moved to the next value of its dtype away from (up) or towards zero"""
    it = torch.int16 if x.dtype.itemsize == 2 else torch.int32
    b = x.clone().view(it)
    return (b + (1 if up else -1)).view(x.dtype)


def swiglu_d_without_one_minus_se(e64):
    """SwiGLU's derivative with (1 - se) dropped: se (1 + e) -- a transcription slip the loose tolerance would let through"""
    s = _sig(e64)
    return s * (1.0 + e64)
