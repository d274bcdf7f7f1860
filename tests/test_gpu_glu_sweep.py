"""-m gpu: the gated activations on EVERY 16-bit input (and the fp32 set around them) against a float64 truth.

The streaming kernels (csrc/glu.hip glu_fwd_kernel / glu_bwd_kernel / quick_gelu_kernel, through the public wrappers) must return,
for every finite e and a few exact (g, DW), a value inside the interval tests/_glu_sweep.py derives from the truth -- one value
for most elements, so a bit-exact assertion there -- and a finite value wherever the interval's bounds are finite. The same sweep is
then run at every lane of the 16-byte vector and through the scalar tail, under every UAMD_TUNE_GLU_VAR / UAMD_TUNE_STREAM_NT
schedule, and every other host of the arithmetic (the fused glu_xa kernels, glu_tn_kernel, the two SwiGLU sites of
csrc/decode.hip) must agree with the streaming kernel bit for bit. tests/test_glu_sweep_inputs.py validates the truth and the
intervals on the host.

The measured figures go to glu_sweep_report.json in the directory UAMD_REPORT_DIR names (default: test_reports/ in the repository
root, git-ignored); profiles/glu_sweep_report.json is a committed copy of one MI355X run: per kernel, activation, dtype and output
the element count, the share of one-value intervals, the worst measured C and the C in force; per activation and dtype the number
of elements whose bits differ between positions / schedules (asserted to be 0); what +-inf returns."""
import json
import os

import pytest
import torch

from tests import _glu_sweep as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {"streaming": {}, "positions": {}, "tail_only": {}, "hosts": {}, "inf": {}}
GLU_VAR, STREAM_NT, GLU_XA = 0, 2, 10
DEFAULT = {GLU_VAR: 2, STREAM_NT: 0, GLU_XA: 3}
NAMES = ("bf16", "fp16", "fp32")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "glu_sweep_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture
def lib():
    from unsloth_amd import _lib
    L = _lib.lib()
    yield L
    for k, v in DEFAULT.items():
        L.uamd_set_tuning(k, v)


def _bits(t):
    return t.view(torch.int16 if t.dtype.itemsize == 2 else torch.int32)


def _ndiff(a, b):
    """number of elements whose bit patterns differ (the sign of a zero included)"""
    return int((_bits(a) != _bits(b)).sum())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and _ndiff(a, b) == 0


def _glu_kernels(act):
    from unsloth_amd.kernels import geglu, swiglu
    return {"swiglu": (swiglu.swiglu_fg_kernel, swiglu.swiglu_DWf_DW_dfg_kernel),
            "geglu_exact": (geglu.geglu_exact_forward_kernel, geglu.geglu_exact_backward_kernel),
            "geglu_approx": (geglu.geglu_approx_forward_kernel, geglu.geglu_approx_backward_kernel)}[act]


def run(act, e, g, dw):
    """{kernel/output: flat device tensor} of the streaming kernels for flat device tensors e, g, dw (left untouched)"""
    n = e.numel()
    if act == "quick_gelu":
        from unsloth_amd.kernels.quick_gelu import fast_quick_gelu
        x = e.clone().requires_grad_(True)
        y = fast_quick_gelu(x)
        y.backward(dw.clone())
        return {"quick_gelu_fwd/y": y.detach(), "quick_gelu_bwd/dx": x.grad}
    fwd, bwd = _glu_kernels(act)
    h = fwd(e.view(1, 1, n), g.view(1, 1, n)).view(-1)
    h2, df, de = bwd(dw.clone().view(1, 1, n), e.clone().view(1, 1, n), g.clone().view(1, 1, n))
    return {"glu_fwd/h": h, "glu_bwd/h": h2.view(-1), "glu_bwd/df": df.view(-1), "glu_bwd/de": de.view(-1)}


def _kind(key):
    return "d" if key.endswith(("/de", "/dx")) else "f"


def _layout(name, vals):
    """the sweep repeated for each (g, DW) pair: flat e, g, DW on the device"""
    dt = S.DTYPES[name]
    P = S.pairs(name)
    n = vals.numel()
    e = vals.repeat(len(P))
    g = torch.tensor([p[0] for p in P], dtype=torch.float64).to(dt).repeat_interleave(n)
    dw = torch.tensor([p[1] for p in P], dtype=torch.float64).to(dt).repeat_interleave(n)
    return e.to(DEV), g.to(DEV), dw.to(DEV)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act", S.ACTS)
def test_streaming_kernels_lie_inside_the_interval_of_the_truth(act, name):
    vals = S.finite_values(name)
    n = vals.numel()
    got = {k: v.cpu() for k, v in run(act, *_layout(name, vals)).items()}
    shares = S.single_share(act, name)
    failures = []
    for pi, (g, dw) in enumerate(S.pairs(name)):
        iv = S.intervals(act, name, vals, g, dw)
        for key, t in got.items():
            out = key.split("/")[1]
            t = t[pi * n:(pi + 1) * n]
            lo, hi = iv[out]
            if pi == 0:                                      # g = DW = 1: the output IS rt(f) resp. rt(f'): measure, then judge
                need = S.needed_c(act, _kind(key), name, vals, t)
                w = int(torch.argmax(need))
                REPORT["streaming"][f"{key}/{act}/{name}"] = dict(
                    elements=n, single_valued_share_to_64=shares[out], worst_ratio=float(need[w]), worst_at_e=float(vals[w]),
                    c_in_force=S.C_IN_FORCE[(act, _kind(key))])
                print(f"{key}/{act}/{name}: worst C {float(need[w]):.4g} at e = {float(vals[w]):.9g}")
            nan = torch.isnan(t.float()) & S.bounds_finite(lo, hi)
            inf = torch.isinf(t.float()) & S.bounds_finite(lo, hi)
            bad = ~S.inside(t, lo, hi, name)
            if bool(nan.any()) or bool(inf.any()) or bool(bad.any()):
                a = vals.double().abs()
                failures.append(f"{key} g={g} DW={dw}: {int(nan.sum())} NaN (|e| from {float(a[nan].min()) if nan.any() else 0:.4g}), "
                                f"{int(inf.sum())} inf, {int(bad.sum())} outside: " + S.describe(bad, vals.double(), t.double(), lo, hi, 3))
    assert not failures, "\n".join(failures)


def _padded(vals, rem=7):
    """the sweep followed by its own first values up to a length of 8 k + rem"""
    extra = (rem - vals.numel()) % 8
    return torch.cat([vals, vals[:extra]])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act", S.ACTS)
def test_position_in_the_vector_and_schedule_do_not_change_a_result(lib, act, name):
    """The sweep (n = 8 k + 7) rotated by 0..7 elements: every value visits every lane of the 16-byte vector and the scalar tail
    loop, under UAMD_TUNE_GLU_VAR 0 / 1 / 2 x UAMD_TUNE_STREAM_NT 0 / 3. Every activation and dtype: the bits of rotation 0
    under the default schedule (fp16 GeGLU too: csrc/glu.hip is built without the mixed-precision fma whose use depended on
    the position, the note in front of fwd_one). The count of differing elements goes to the report before it is asserted."""
    vals = _padded(S.finite_values(name))
    n = vals.numel()
    assert n % 8 == 7
    g, dw = S.pairs(name)[2]
    dt = S.DTYPES[name]
    e0 = vals.to(DEV)
    gt, dwt = torch.full((n,), g, dtype=dt, device=DEV), torch.full((n,), dw, dtype=dt, device=DEV)
    base = run(act, e0, gt, dwt)
    differ = {k: 0 for k in base}
    schedules = [(2, 0)] if act == "quick_gelu" else [(v, nt) for v in (2, 0, 1) for nt in (0, 3)]
    for var, nt in schedules:
        assert lib.uamd_set_tuning(GLU_VAR, var) == 0 and lib.uamd_set_tuning(STREAM_NT, nt) == 0
        for r in range(8):
            got = run(act, torch.roll(e0, r), gt, dwt)
            for k, t in got.items():
                differ[k] = max(differ[k], _ndiff(torch.roll(t, -r), base[k]))
    REPORT["positions"][f"{act}/{name}"] = dict(elements=n, asserted_identical=True,
                                               most_elements_differing_from_rotation_0=differ)
    assert not any(differ.values()), differ


@pytest.mark.parametrize("name", ("bf16", "fp16"))
@pytest.mark.parametrize("act", S.ACTS)
def test_seven_element_tensors_take_the_tail_loop_alone(lib, act, name):
    """nvec = 0: every value with 2^-4 <= |e| <= 2^7 in a 7-element tensor of its own, against the same values in one long tensor
    (default schedule), bit for bit; once under the default schedule and once under UAMD_TUNE_GLU_VAR 0 + UAMD_TUNE_STREAM_NT 3
    (with no whole vector only block 0's tail loop works, whatever the grid: the second pass shows it)."""
    vals = S.mid_values(name)
    vals = torch.cat([vals, vals[:(-vals.numel()) % 7]])
    rows = vals.numel() // 7
    g, dw = S.pairs(name)[1]
    dt = S.DTYPES[name]
    e0 = vals.to(DEV)
    gt, dwt = torch.full_like(e0, g), torch.full_like(e0, dw)
    want = run(act, e0, gt, dwt)
    buf = torch.zeros(rows, 8, dtype=dt, device=DEV)           # rows of 7 on 16-byte boundaries
    buf[:, :7] = e0.view(rows, 7)
    differ = {k: 0 for k in want}
    for var, nt in ((2, 0), (0, 3)):
        assert lib.uamd_set_tuning(GLU_VAR, var) == 0 and lib.uamd_set_tuning(STREAM_NT, nt) == 0
        got = {k: torch.empty_like(e0).view(rows, 7) for k in want}
        for i in range(rows):
            for k, t in run(act, buf[i, :7], gt[:7], dwt[:7]).items():
                got[k][i] = t
        for k, t in got.items():
            differ[k] = max(differ[k], _ndiff(t.reshape(-1), want[k]))
    REPORT["tail_only"][f"{act}/{name}"] = dict(elements=vals.numel(), asserted_identical=True, elements_differing=differ)
    assert not any(differ.values()), differ


# ---------------------------------------------------------------------------------------------- the other hosts of the arithmetic
def _host_pairs(name):
    """(g, DW) with |g|, |DW| <= 1: h and df are finite for every finite e"""
    return ((0.75, -0.625), (-1.0, 1.0 - 2.0 ** -S.MANT[name]))


def _host_inputs(name, K):
    """[M, K] e, g, DW holding the finite sweep once per (g, DW) pair (the last row filled up from the start)"""
    dt = S.DTYPES[name]
    vals = S.finite_values(name)
    P = _host_pairs(name)
    n = vals.numel()
    M = (n * len(P) + K - 1) // K
    idx = torch.arange(M * K) % (n * len(P))
    e = vals.repeat(len(P))[idx]
    g = torch.tensor([p[0] for p in P], dtype=torch.float64).to(dt).repeat_interleave(n)[idx]
    dw = torch.tensor([p[1] for p in P], dtype=torch.float64).to(dt).repeat_interleave(n)[idx]
    return tuple(t.view(M, K).to(DEV) for t in (e, g, dw))


def _proj(n_out, n_in, r, seed, dt):
    gen = torch.Generator().manual_seed(seed)
    W = torch.zeros(n_out, n_in, dtype=dt, device=DEV)
    A = (torch.randn(r, n_in, generator=gen) * 0.02).to(DEV)
    B = (torch.randn(n_out, r, generator=gen) * 0.02).to(DEV)
    return (W, None, A, B, 2.0)


@pytest.fixture
def fused_any_size():
    from unsloth_amd.kernels import utils as U
    keep = U.GLU_FUSED, U.GLU_TN
    U.GLU_FUSED, U.GLU_TN = "all", True
    yield U
    U.GLU_FUSED, U.GLU_TN = keep


@pytest.mark.parametrize("name", ("bf16", "fp16"))
@pytest.mark.parametrize("K", [264, 520, 1024])
def test_fused_activation_kernels_equal_the_streaming_kernel_on_the_sweep(lib, fused_any_size, K, name):
    """glu_xa_kernel (forward and backward, UAMD_TUNE_GLU_XA 0 / 3 / 8) and glu_tn_kernel: h, df, de the bits of the
    streaming kernel. K = 264 and 520 reach the column remainder of the 256-column tile. The rank products are not looked at:
    with |e| up to the largest finite value they overflow by construction (tests/test_gpu_glu_fused.py covers them)."""
    U = fused_any_size
    e, g, dw = _host_inputs(name, K)
    M = e.shape[0]
    want = run("swiglu", e.reshape(-1), g.reshape(-1), dw.reshape(-1))
    assert all(bool(torch.isfinite(t.float()).all()) for t in want.values())
    dt = S.DTYPES[name]
    down, up, gate = _proj(64, K, 8, 1, dt), _proj(K, 64, 8, 2, dt), _proj(K, 64, 8, 3, dt)
    for xv in (0, 3, 8):
        assert lib.uamd_set_tuning(GLU_XA, xv) == 0
        out = U.glu_fwd_xa("swiglu", e, g, down)
        assert out is not None
        assert _same(out[0].reshape(-1), want["glu_fwd/h"]), ("fwd_xa", xv)
        res = U.glu_bwd_terms("swiglu", dw.clone(), e.clone(), g.clone(), up, gate)
        assert res is not None
        for t, k in zip(res[:3], ("glu_bwd/h", "glu_bwd/df", "glu_bwd/de")):
            assert _same(t.reshape(-1), want[k]), ("bwd_xa", xv, k)
    zeros = torch.zeros(M, 8, dtype=torch.float32, device=DEV)
    dw1 = dw.clone()
    res = U.glu_bwd_tn("swiglu", dw1, e.clone(), g.clone(), up, gate, down, zeros, zeros.clone(), zeros.clone())
    assert res is not None
    assert _same(res[0].reshape(-1), want["glu_bwd/df"]) and _same(res[1].reshape(-1), want["glu_bwd/de"])
    assert _same(dw1, dw)
    REPORT["hosts"][f"glu_xa+glu_tn/swiglu/{name}/K={K}"] = dict(elements=e.numel(), identical_to_streaming=True)


def _decode_mismatches(h, want, sign_free):
    """elements whose bits differ, except a zero of the other sign where `sign_free` (the value that travelled through the GEMV
    was a zero: 1 * (-0) + 0 + ... = +0, a sum of zeros keeps no sign)"""
    return int(((_bits(h) != _bits(want)) & ~(sign_free & (h == 0) & (want == 0))).sum())


@pytest.mark.parametrize("name", ("bf16", "fp16"))
def test_decode_swiglu_sites_equal_the_streaming_kernel_on_the_sweep(name):
    """csrc/decode.hip restates SwiGLU twice. Prologue (mode = 1): the token h = SwiGLU(e, g) is formed inside the GEMV; an identity
    weight reads it back (every dot product is 1 * h[n] + zeros). Epilogue (glu = True): e and g are the dot products of a one-hot
    token with weights whose first column holds the sweep and g; h = SwiGLU of the two rounded sums. Both must equal
    uamd_swiglu_fg bit for bit on every finite e, subnormal e and subnormal h included. One allowance: the value that TRAVELS
    through the GEMV's sum (h in the first case, e in the second) loses the sign of a zero there, so where that value is a zero
    the result may be the zero of the other sign."""
    from unsloth_amd.kernels import decode as D
    dt = S.DTYPES[name]
    K1 = 2048
    e, g, _ = _host_inputs(name, K1)
    want = run("swiglu", e.reshape(-1), g.reshape(-1), torch.ones_like(e).reshape(-1))["glu_fwd/h"].view(e.shape)
    assert bool(torch.isfinite(want.float()).all())
    eye = torch.eye(K1, dtype=dt, device=DEV)
    bad1 = 0
    for i in range(e.shape[0]):
        (h,) = D.linear_group(e[i], [(eye, None, None, None, None)], fused=dict(mode=1, x2=g[i]))
        bad1 += _decode_mismatches(h, want[i], want[i] == 0)
    N, K0 = 4096, 64
    e, g, _ = _host_inputs(name, N)
    want = run("swiglu", e.reshape(-1), g.reshape(-1), torch.ones_like(e).reshape(-1))["glu_fwd/h"].view(e.shape)
    x = torch.zeros(K0, dtype=dt, device=DEV)
    x[0] = 1.0
    Wg, Wu = torch.zeros(N, K0, dtype=dt, device=DEV), torch.zeros(N, K0, dtype=dt, device=DEV)
    bad0 = 0
    for i in range(e.shape[0]):
        Wg[:, 0], Wu[:, 0] = e[i], g[i]
        (h,) = D.linear_group(x, [(Wg, None, None, None, None), (Wu, None, None, None, None)], fused=dict(mode=0, glu=True))
        bad0 += _decode_mismatches(h, want[i], e[i] == 0)
    REPORT["hosts"][f"decode/swiglu/{name}"] = dict(elements=e.numel(), prologue_mismatches=bad1, epilogue_mismatches=bad0)
    assert bad1 == 0 and bad0 == 0, (bad1, bad0)


# ------------------------------------------------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act", S.ACTS)
def test_nan_reaches_exactly_the_outputs_that_depend_on_it(act, name):
    """A NaN in e, g or DW: NaN in the outputs made of that operand at that element (h of e, g; df of DW, e; de of all three;
    y of x; dx of x, dy), every other element identical to the run without it. n = 8 k + 7: vector lanes and the tail loop."""
    dt = S.DTYPES[name]
    n = 1031
    mid = S.mid_values(name)
    e = mid[torch.arange(n) * 37 % mid.numel()].to(DEV)
    g, dw = torch.full((n,), -1.5, dtype=dt, device=DEV), torch.full((n,), 0.625, dtype=dt, device=DEV)
    at = torch.tensor([0, 3, 7, 8, 15, 511, 512, 1023, 1024, 1027, 1030], device=DEV)
    clean = run(act, e, g, dw)
    assert not any(bool(torch.isnan(t.float()).any()) for t in clean.values())
    depends = {"h": "eg", "df": "ew", "de": "egw", "y": "e", "dx": "ew"}
    for which in ("e", "g", "w"):
        if act == "quick_gelu" and which == "g":
            continue
        ins = {"e": e.clone(), "g": g.clone(), "w": dw.clone()}
        ins[which][at] = float("nan")
        got = run(act, ins["e"], ins["g"], ins["w"])
        hit = torch.zeros(n, dtype=torch.bool, device=DEV)
        hit[at] = True
        for k, t in got.items():
            expect = hit if which in depends[k.split("/")[1]] else torch.zeros_like(hit)
            assert torch.equal(torch.isnan(t.float()), expect), (k, which)
            assert _same(t[~expect], clean[k][~expect]), (k, which)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act", S.ACTS)
def test_infinite_inputs_are_reported(act, name):
    """what e = +-inf returns (g = DW = 1) goes to the report; nothing is asserted but that its finite neighbours are unchanged"""
    dt = S.DTYPES[name]
    e = torch.ones(15, dtype=dt, device=DEV)
    one = e.clone()
    clean = run(act, e, one, one)
    e[3], e[12] = float("inf"), float("-inf")
    got = run(act, e, one, one)
    keep = torch.ones(15, dtype=torch.bool, device=DEV)
    keep[3] = keep[12] = False
    for k, t in got.items():
        assert _same(t[keep], clean[k][keep]), k
        REPORT["inf"][f"{k}/{act}/{name}"] = {"+inf": str(float(t[3])), "-inf": str(float(t[12]))}
