"""-m gpu: LoRA_MLP / LoRA_QKV / LoRA_W (unsloth_amd/kernels/fast_lora.py) on every dispatch route of the host code under them
(unsloth_amd/kernels/utils.py), slice by slice against an fp64 truth.

tests/test_gpu_lora_blocks.py runs one shape and one rank per block under the module defaults and judges by one Frobenius norm.
Here a table of small cases (tests/_lora_blocks.py CASES) forces each route with the module switches of kernels/utils.py -- the
128-tile GEMM with the LoRA term in its prologue or the 256-tile family with the rank block, NF4 decoded in the GEMM or into
scratch, NT or NN and merged or per-projection dX, the three X @ A^T paths, the three MLP backward routes -- at ranks 4 .. 128,
mixed ranks, every adapter subset and row counts beside the tile and policy edges. Every case states the routes it means to
reach and two spies hold it to them: the library entry points that were launched and which of glu_fwd_xa / glu_bwd_tn /
glu_bwd_terms / lora_tn / _lora_grads took the shape. Every output is judged per token row (activations), rank row (dA) or rank
column (dB): its distance from the fp64 truth may be BOUND_FACTOR = 4 x the distance of a plain fp32 model with the product's
16-bit rounding points (tests/_lora_blocks.py rounding_model) on the same slice. tests/test_lora_block_inputs.py shows on the
host that this yardstick has the size of 16-bit rounding on every slice and that every wrong variant of a block lies beyond 8 x.

The measured ratios go to lora_block_report.json in the directory UAMD_REPORT_DIR names (default: test_reports/ in the
repository root, git-ignored); profiles/lora_block_report.json is a committed copy of one MI355X run: per case and tensor the
kernel's and the model's error on the slice with the worst ratio, and that ratio. The worst ratio per block, route and tensor
in that run (fwd = out or Q / K / V; 128- / 256-tile = GEMM256_MODE "off" / "on"; plain / terms / tn = the MLP backward route):

    mlp  128-tile  plain             fwd 1.24  dX 1.25  dA 1.20  dB 1.12
    mlp  128-tile  terms             fwd 1.21  dX 1.19  dA 1.18  dB 1.19
    mlp  128-tile  tn                fwd 1.18  dX 1.21  dA 1.16  dB 1.11
    mlp  256-tile  plain             fwd 1.28  dX 1.18  dA 1.18  dB 1.14
    mlp  256-tile  terms             fwd 1.25  dX 1.33  dA 1.20  dB 1.13
    mlp  256-tile  tn                fwd 1.24  dX 1.19  dA 1.12  dB 1.14
    qkv  128-tile  merged dX         fwd 1.09  dX 1.01  dA 1.00  dB 1.01
    qkv  128-tile  per-projection dX fwd 1.11  dX 1.89  dA 1.00  dB 1.00
    qkv  256-tile  merged dX         fwd 1.09  dX 1.00  dA 1.00  dB 1.00
    qkv  256-tile  per-projection dX fwd 1.08  dX 1.80  dA 1.07  dB 1.02  dbias 1.00
    w    128-tile                    fwd 1.04  dX 1.01  dA 1.01  dB 1.00
    w    256-tile                    fwd 1.00  dX 1.03  dA 1.01  dB 1.00

Nothing comes near 4, so BOUND_FACTOR stands for every tensor and L.FACTORS is empty. The one figure that stands out has a
cause: the per-projection dX of q|k|v is written in 16 bits by the first GEMM and read, added to and rounded again by the next
two, three roundings where the model (and the merged GEMM: 1.0) has one. The smallest wrong variant on the host side is 18 x.

Routes and a case that reaches each (the table in tests/_lora_blocks.py has them all):
  lora_linear_forward    NF4 in the GEMM, LoRA in its prologue: mlp-r16-plain, qkv-r16, w-r16 | NF4 into scratch, 128-tile:
                         mlp-r16-m129-maxm, qkv-r16-m129-maxm | NF4 into scratch, 256-tile rank block: mlp-r16-256-decode,
                         qkv-r64-256-merged, w-r16-fp16-256-decode | dense, prologue: mlp-r16-tn-dense, qkv-r16-merged-dense |
                         dense, rank block: mlp-r16-256-tn-dense, qkv-r64-256-dense | X A^T handed over by glu_fwd_xa:
                         mlp-r16-tn, with its rank block mlp-r16-256-tn-dense | bias in the epilogue: qkv-r16-bias-frozen
  _rank_plan, forward    (_xa_and_rank_block; tests/test_rank_plan_host.py pins the launch lists) rank block, <= 64 ranks: every
                         r <= 16 case | 65 .. 192 in groups of 64: mlp-r64-256-dense, qkv-r64-256-dense,
                         qkv-r32-m129-256-dense | first-version kernel + padded cast: mlp-r128-256-dense, qkv-r128-256-dense,
                         mlp-r16-xa1-256-dense | no rank block, one launch of 65 .. 192 ranks: mlp-r64-terms, qkv-r64 | past
                         192 in chunks: mlp-r128, qkv-r128-merged
  _rank_plan, backward   (lora_dx_terms) shared P and shared rank block: qkv-r16-merged-scales-256, qkv-r64-256-merged | one
                         adapter's rank block: w-r4-m129-256-dense, qkv-q-only-256-dense | padded cast per term (odd ranks, a
                         missing adapter, r > 64): mlp-r4-256-dense, qkv-r16-8-4-m257-256-dense, qkv-r128-256-dense | no rank
                         block: every 128-tile case | no adapter: mlp-none, qkv-none-merged, w-none
  _dx_gemm               NT, 128-tile prologue: every 128-tile case, odd ranks through the padded LB: mlp-r4, qkv-r4 | NN, rank
                         block: every 256-tile case | 256-tile wanted but no shared rank block, prologue: mlp-r16-xa1-256-dense,
                         qkv-r128-m129-256-merged | NN without an adapter: mlp-none-256-dense
  _lora_linear_dx_merged taken: qkv-r16-merged, qkv-r16-merged-scales-256, qkv-r64-256-merged, df | de in mlp-r16-terms |
                         declined -- dense weights: qkv-r16-merged-dense, mlp-r16-tn-dense; a missing adapter:
                         qkv-q-v-only-merged, qkv-none-merged; no shared P (ranks no multiple of 8): qkv-r16-8-4-merged;
                         differing scales on the prologue: qkv-r16-merged-scales; separate buffers: qkv-r16, mlp-r16-plain;
                         one row: qkv-r8-m1
  mlp_forward            glu_fwd_xa: mlp-r16-tn | plain SwiGLU: mlp-r16-plain | GeGLU: mlp-r16-geglu-exact,
                         mlp-r16-geglu-approx-256-dense | fused route declines the rank: mlp-r4, mlp-r128; no down adapter:
                         mlp-gate-up-only
  mlp_backward           glu_bwd_tn: mlp-r16-tn, mlp-r8-tn | glu_bwd_terms: mlp-r16-terms, mlp-r32-terms, mlp-r64-terms,
                         mlp-r8-16-64, mlp-gate-up-only | plain kernel + lora_dx_terms: mlp-r16-plain, mlp-r4, mlp-r128

Routes no case reaches: the torch `_lora_grads` fallback (lora_tn_supported refuses only a feature width that is no multiple
of 8, which none of the fixed widths is; the spy asserts it never runs), uamd_gemm_nt_256 as a dX GEMM (with H and I multiples
of 8 a dX launch on the 256-tile family that has its rank block is the NN form, and one without keeps the 128-tile prologue),
and GLU_FUSED = "both" / "bwd" (the row threshold of 2048 is a property of the switch, not another kernel)."""
import json
import os
import types

import pytest
import torch

from tests import _lora_blocks as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}

FUNCTION_LEVEL = [n for n, c in L.CASES.items() if not c["bias"]]
# through the autograd Functions: the bias cases (d_bias is formed there), None gradients for absent adapters, both `inplace`
AUTOGRAD = [n for n, c in L.CASES.items() if c["bias"]] + ["mlp-r16-tn", "mlp-gate-up-only", "mlp-none", "qkv-r16-merged",
                                                          "qkv-q-v-only-merged", "qkv-r16-merged-scales-256", "w-r16", "w-none"]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "lora_block_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture
def spy(monkeypatch):
    """entries: the library entry points of L.ENTRIES in launch order (recorded the way the `calls` fixture of
    tests/test_gpu_gemm_views.py does); py: [(name of L.PY_ROUTES, did it take the shape)] as fast_lora.py called them."""
    from unsloth_amd import _lib
    from unsloth_amd.kernels import fast_lora as FL
    lib = _lib.lib()
    seen = types.SimpleNamespace(entries=[], py=[])
    for name in L.ENTRIES:
        def wrapped(*a, _fn=getattr(lib, name), _name=name):
            seen.entries.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)
    for name in L.PY_ROUTES:
        def route(*a, _fn=getattr(FL, name), _name=name, **kw):
            res = _fn(*a, **kw)
            if _name == "lora_tn":
                took = bool(a[0])                                  # (an empty problem list launches nothing)
            elif _name == "_lora_grads":
                took = res[0] is not None
            else:
                took = res is not None                             # the fused GLU routes answer None when they decline
            seen.py.append((_name, took))
            return res
        monkeypatch.setattr(FL, name, route)
    return seen


def _on_gpu(c):
    """The case on the device: X, {output: dY} (column blocks of one buffer when `merged`) and per projection
    (W or packed NF4, quant state, A, B, s, bias) with the factors as fp32 Parameters or plain tensors."""
    X, dYs, projs = L.case_inputs(c["name"])
    dev = {}
    for p, (W, pieces, A, B, s, bias) in projs.items():
        Wd, qs = L.quant_state(pieces, DEV) if pieces is not None else (W.to(DEV), None)
        if A is not None:
            make = (lambda t: torch.nn.Parameter(t.to(DEV))) if c["params"] else (lambda t: t.to(DEV).requires_grad_(True))
            A, B = make(A), make(B)
        if bias is not None:
            bias = bias.to(DEV).requires_grad_(c["bias"] == "train")
        dev[p] = (Wd, qs, A, B, s if A is not None else None, bias)
    outs = L.OUTPUTS[c["block"]]
    if c["merged"]:
        cat = torch.cat([dYs[o] for o in outs], dim=1).to(DEV)
        ends = [0]
        for o in outs:
            ends.append(ends[-1] + dYs[o].shape[1])
        dY = {o: cat[:, a:b] for o, a, b in zip(outs, ends, ends[1:])}
    else:
        dY = {o: dYs[o].to(DEV) for o in outs}
    return X.to(DEV), dY, dev


def _acts(kind):
    import unsloth_amd.kernels as K
    return {"swiglu": (K.swiglu_fg_kernel, K.swiglu_DWf_DW_dfg_kernel),
            "geglu_exact": (K.geglu_exact_forward_kernel, K.geglu_exact_backward_kernel),
            "geglu_approx": (K.geglu_approx_forward_kernel, K.geglu_approx_backward_kernel)}[kind]


def _functions(c, spy):
    """mlp_forward / mlp_backward, qkv_forward / qkv_backward, w_forward / w_backward as the whole-layer Function calls them
    (no autograd). Returns ({tensor: result}, launches of the forward, problems found)."""
    from unsloth_amd.kernels import fast_lora as FL
    X, dY, dev = _on_gpu(c)
    X0 = X.clone()
    P = [dev[p][:5] for p in L.PROJS[c["block"]]]
    bad, got = [], {}
    with torch.no_grad():
        if c["block"] == "mlp":
            fwd, bwd = _acts(c["kind"])
            out, e, g, xas = FL.mlp_forward(X, *P, fwd)
            got["out"] = out.cpu()
            n_fwd = len(spy.entries)
            dX, grads = FL.mlp_backward(dY["out"], X, e, g, xas, *P, bwd, inplace=c["inplace"])
            order = ("gate", "up", "down")
        elif c["block"] == "qkv":
            Q, K, V, xas = FL.qkv_forward(X, *P)
            got.update(Q=Q.cpu(), K=K.cpu(), V=V.cpu())
            n_fwd = len(spy.entries)
            dX, grads = FL.qkv_backward(dY["Q"], dY["K"], dY["V"], X, xas, *P, inplace=c["inplace"])
            order = ("q", "k", "v")
        else:
            out, xa = FL.w_forward(X, P[0])
            got["out"] = out.cpu()
            n_fwd = len(spy.entries)
            dX, grads = FL.w_backward(dY["out"], X, xa, P[0])
            order = ("o",)
        torch.cuda.synchronize()
    inplace = c["inplace"] and c["block"] != "w"                   # (w_backward has no in-place form)
    if inplace and dX.data_ptr() != X.data_ptr():
        bad.append("inplace=True: dX is not in X's buffer")
    if not inplace and (dX.data_ptr() == X.data_ptr() or not torch.equal(X.view(torch.int16), X0.view(torch.int16))):
        bad.append("inplace=False: X was written")
    got["dX"] = dX.cpu()
    for i, p in enumerate(order):
        got[f"dA_{p}"], got[f"dB_{p}"] = grads[2 * i], grads[2 * i + 1]
    return got, n_fwd, bad


def _autograd(c, spy):
    """The same through LoRA_MLP / LoRA_QKV / LoRA_W.apply and torch.autograd.backward."""
    from unsloth_amd.kernels import fast_lora as FL
    X, dY, dev = _on_gpu(c)
    Xg = X.clone().requires_grad_(True)
    Xin = Xg * 1.0                                                 # the saved input: a non-leaf the block may overwrite
    X0 = Xin.detach().clone()
    order = L.PROJS[c["block"]]
    flat = [a for p in order for a in dev[p][:5]]
    bad, got = [], {}
    if c["block"] == "mlp":
        outs = [FL.LoRA_MLP.apply(Xin, *flat, *_acts(c["kind"]), c["inplace"])]
    elif c["block"] == "qkv":
        biases = [dev[p][5] for p in order]
        outs = list(FL.LoRA_QKV.apply(Xin, *flat, c["inplace"], *(biases if c["bias"] else ())))
    else:
        outs = [FL.LoRA_W.apply(Xin, *flat)]
    for o, y in zip(L.OUTPUTS[c["block"]], outs):
        got[o] = y.detach().cpu()
    n_fwd = len(spy.entries)
    torch.autograd.backward(outs, [dY[o] for o in L.OUTPUTS[c["block"]]])
    torch.cuda.synchronize()
    got["dX"] = Xg.grad.cpu()
    if c["inplace"] and c["block"] != "w":
        if not torch.equal(Xin.detach(), Xg.grad):
            bad.append("inplace=True: dX was not written into the saved X")
    elif not torch.equal(Xin.detach().view(torch.int16), X0.view(torch.int16)):
        bad.append("inplace=False: the saved X was written")
    for p in order:
        _, _, A, B, _, bias = dev[p]
        got[f"dA_{p}"] = None if A is None else A.grad
        got[f"dB_{p}"] = None if B is None else B.grad
        if c["bias"] == "train":
            got[f"dbias_{p}"] = bias.grad
        elif bias is not None and bias.grad is not None:
            bad.append(f"a frozen bias of {p} got a gradient")
    return got, n_fwd, bad


def _routes(c, spy, n_fwd):
    """What the spies saw against what the case states; [] when it reached exactly its routes."""
    fwd = {L.GEMM[n] for n in spy.entries[:n_fwd] if n in L.GEMM}
    bwd = [L.GEMM[n] for n in spy.entries[n_fwd:] if n in L.GEMM]
    xa = {L.XA[n] for n in spy.entries if n in L.XA}
    decode = any(n in L.DECODE for n in spy.entries[:n_fwd])
    py = {n for n, took in spy.py if took}
    seen = dict(fwd=fwd, bwd=set(bwd), n_bwd=len(bwd), xa=xa, decode=decode, py=py)
    bad = [f"route {k}: reached {seen[k]}, the case states {c[k]}" for k in seen if seen[k] != c[k]]
    # the two spies agree: a fused GLU route that took the shape launched its kernel, one that declined did not
    for py_name, entry in (("glu_fwd_xa", "uamd_glu_fwd_xa_ws"), ("glu_bwd_terms", "uamd_glu_bwd_xa_ws"),
                           ("glu_bwd_tn", "uamd_glu_bwd_tn_ws"), ("lora_tn", "uamd_lora_tn")):
        if (py_name in py) != (entry in spy.entries):
            bad.append(f"{py_name} took the shape: {py_name in py}, but {entry} launched: {entry in spy.entries}")
    return bad


def _judge(c, how, got):
    dt = L.DTYPES[c["dtype"]]
    bad = []
    assert set(got) == set(c["truth"]), (sorted(got), sorted(c["truth"]))
    for t, ref in c["truth"].items():
        g = got[t]
        if ref is None:
            if g is not None:
                bad.append(f"{t}: an absent adapter must return None")
            continue
        if g is None:
            bad.append(f"{t}: missing")
            continue
        want = torch.float32 if t[:3] in ("dA_", "dB_") else dt
        if g.dtype != want or tuple(g.shape) != tuple(ref.shape):
            bad.append(f"{t}: {g.dtype} {tuple(g.shape)}, expected {want} {tuple(ref.shape)}")
            continue
        if not bool(torch.isfinite(g.float()).all()):
            bad.append(f"{t}: not finite")
            continue
        err, model, ratio, ok = L.judge(c, t, g)
        i = int(torch.where(err == 0, torch.zeros_like(err), err / model).argmax())
        REPORT[f"{c['name']}/{how}/{t}"] = dict(kernel=float(err[i]), model=float(model[i]), ratio=ratio)
        print(f"{c['name']}/{how}/{t}: kernel {float(err[i]):.3e} model {float(model[i]):.3e} ratio {ratio:.2f}")
        if not ok:
            bad.append(f"{t}: slice {i} is {ratio:.2f} x the model's error (kernel {float(err[i]):.3e}, model {float(model[i]):.3e})")
    return bad


def _run(name, how, runner, spy, monkeypatch):
    from unsloth_amd.kernels import utils as U
    c = L.build_case(name)
    for k, v in c["knobs"].items():
        assert hasattr(U, k), k
        monkeypatch.setattr(U, k, v)
    U.invalidate_cast_cache()
    got, n_fwd, bad = runner(c, spy)
    print(f"{name}/{how}: entries {spy.entries} py {spy.py}")
    bad += _routes(c, spy, n_fwd)
    bad += _judge(c, how, got)
    assert not bad, "\n".join([name] + bad)


@pytest.mark.parametrize("name", FUNCTION_LEVEL)
def test_block_functions_on_every_route(name, spy, monkeypatch):
    _run(name, "functions", _functions, spy, monkeypatch)


@pytest.mark.parametrize("name", AUTOGRAD)
def test_autograd_functions_on_every_route(name, spy, monkeypatch):
    _run(name, "autograd", _autograd, spy, monkeypatch)
