"""-m gpu: `unsloth_fused_ce_loss` (unsloth_amd/kernels/cross_entropy_loss.py) on the vocabulary, vector, row-chunk and
dW-scaling edges, row by row against an fp64 truth; and out-of-range labels through the CE kernels.

tests/test_gpu_lora_blocks.py, tests/test_gpu_linear_ce_golden.py and tests/test_gpu_full_finetune.py judge the fused loss by
its scalar and by one Frobenius norm per gradient, at shapes that fit one row chunk. Here a table of small cases
(tests/_linear_ce.py CASES: T = 194 rows in chunks of 64 | 64 | 64 | 2, H = 256) puts it on a padded vocabulary with a scalar
tail (V = 1003, 8197), on the 8191 | 8192 boundary between two blocks of ce_bwd_kernel and two _DW_SCALE_ROWS steps of the
backward (V = 8200, 8197), on both GEMM families, on the NN form of d(hidden) (no W^T), with logit scaling, a soft cap, fp16,
n_items counted / an int / a 0-dim GPU tensor, a mask, and hidden states read in place from a [..., :H] view. The inputs put
0.55 .. 0.73 of a row's softmax on each edge column, on rows on and beside the chunk edges, and make one row pad-sensitive.

  gradients   each case runs with a frozen head and with a trainable one (a Parameter of the activation dtype, no gradient
              sink: dW comes back through autograd). Every token row of d(hidden) and every vocabulary row of dW is held to
              BOUND_FACTOR = 4 x the error of a plain fp64 model with the product's 16-bit rounding points on the same row; a
              row whose truth is zero must be exactly zero. A spy holds the launches to exactly the sequence the case states;
              d(hidden) of the two runs is bitwise equal; the padding columns of the logits chunk are zero before and after the
              CE backward.
  row losses  for every edge row, the pad-sensitive row and two interior rows a forward-only call under no_grad() with a mask
              that keeps that row alone and n_items = 1 is held to b_r, one ulp of every logit (tests/_linear_ce.py); it
              launches no CE backward, no d(hidden) GEMM and no dW GEMM although hidden states and head ask for gradients.
              The full call's scalar loss is held to sum_r b_r / n.
tests/test_linear_ce_inputs.py shows on the host that this yardstick has the size of 16-bit rounding on every row and that
every wrong variant (a dropped last column, padding counted, labels off by one, a lost chunk row, dW overwritten or its tail
unscaled, a missing derivative factor, mask or n_items ignored) is rejected by these same checks.

The measured ratios go to linear_ce_report.json in the directory UAMD_REPORT_DIR names (default: test_reports/ in the
repository root, git-ignored); profiles/linear_ce_report.json is a committed copy of one MI355X run: per case, run and tensor
the kernel's and the model's error on the row with the worst ratio, and that ratio; per case the worst row loss as a fraction
of b_r. The worst ratio per route in that run:

    logits GEMM        d(hidden) GEMM             dtype  cases   d(hidden)  dW (uamd_gemm_tn_256)  row loss / b_r  loss / bound
    uamd_gemm_nt       uamd_gemm_nt over W^T      bf16   5       1.01       1.08                   0.36            0.027
    uamd_gemm_nt       uamd_gemm_nt over W^T      fp16   2       1.05       1.06                   0.38            0.010
    uamd_gemm_nt_256   uamd_gemm_nt over W^T      bf16   3       1.01       1.22                   0.37            0.029
    uamd_gemm_nt_256   uamd_gemm_nn_256 over W    bf16   2       1.00       1.06                   0.16            0.018

Nothing comes near 4, so BOUND_FACTOR stands for both tensors and C.FACTORS is empty. The largest figure, 1.22, is one ordinary
dW row (6198) of v8197-cap-256: kernel 2.0e-7 against the model's 1.7e-7, on a tensor that is rounded four times, once per row
chunk. The row losses use about a third of b_r, which is what the host test measures for the rounding model itself (0.24 ..
0.38): the logits' rounding alone. The weakest rejection of a wrong variant on the host side is 25 x (no_cap_deriv, on
d(hidden) of the soft cap + scaling case).

Not covered here: the gradient-sink branch of _FusedLinearCE.backward (FullGradBuckets, first_write False) stays with
tests/test_gpu_full_finetune.py; the 4 GiB chunking, fp32 activations and a bias on the head are out of scope.

The last test is the kernel-level side of the same work: a label outside [0, V) is treated like -100 by ce_bwd_kernel as it
always was by ce_fwd_kernel (loss / log-prob 0 AND a zero gradient row), through Fast_CrossEntropyLoss and
Fast_LogProbEntropy."""
import json
import os
import types

import pytest
import torch

from tests import _linear_ce as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
ALL = list(C.CASES)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "linear_ce_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture
def spy(monkeypatch):
    """entries: the library entry points of C.ENTRIES in launch order by their short names; gemm: [(short name, lda, accumulate)]
    of the GEMM launches; pad_ok: for each CE backward, were the padding columns of the logits chunk zero before and after."""
    from unsloth_amd import _lib
    from unsloth_amd.kernels import cross_entropy_loss as CE
    lib = _lib.lib()
    seen = types.SimpleNamespace(entries=[], gemm=[], pad_ok=[])
    short = dict(C.GEMM, **C.CE)
    for name in C.ENTRIES:
        def wrapped(*a, _fn=getattr(lib, name), _name=name):
            seen.entries.append(short[_name])
            if _name in C.GEMM:
                seen.gemm.append((short[_name], int(a[1]), int(a[6])))
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)

    def ce_backward(logits2d, *a, _fn=CE._ce_backward_, **kw):
        chunk = logits2d._base if logits2d._base is not None else logits2d
        V = logits2d.shape[1]
        before = not bool(chunk[:, V:].any())
        res = _fn(logits2d, *a, **kw)
        seen.pad_ok.append((tuple(chunk.shape), before and not bool(chunk[:, V:].any())))
        return res
    monkeypatch.setattr(CE, "_ce_backward_", ce_backward)
    return seen


def _call(c, hidden, W, labels, **over):
    from unsloth_amd.kernels import unsloth_fused_ce_loss
    n = c["n_items"]
    if isinstance(n, tuple):
        n = torch.tensor(n[1], device=DEV)
    kw = dict(mask=None, n_items=n, logit_softcapping=c["softcap"], logit_scaling=c["scale"], chunk_rows=c["chunk_rows"])
    kw.update(over)
    return unsloth_fused_ce_loss(None, hidden, W, None, labels, **kw)


def _chunks(c):
    return [min(c["chunk_rows"], C.T - r0) for r0 in range(0, C.T, c["chunk_rows"])]


def _train_run(c, spy, trainable):
    """One training call of the case: (loss, d(hidden) [T, H], dW [V, H] or None, problems found)."""
    h, W, labels, mask = C.case_inputs(c["name"])
    dt = C.DTYPES[c["dtype"]]
    bad = []
    if c["view"]:
        buf = torch.zeros(C.B, C.L, C.H + 8, dtype=dt)
        buf[..., :C.H] = h.view(C.B, C.L, C.H)
        leaf = buf.to(DEV).requires_grad_(True)
        hidden, lda = leaf[..., :C.H], C.H + 8
    else:
        leaf = h.view(C.B, C.L, C.H).to(DEV).requires_grad_(True)
        hidden, lda = leaf, C.H
    Wd = torch.nn.Parameter(W.to(DEV)) if trainable else W.to(DEV)
    del spy.entries[:], spy.gemm[:], spy.pad_ok[:]
    loss = _call(c, hidden, Wd, labels.to(DEV), mask=None if mask is None else mask.to(DEV))
    (loss / 3).backward()
    torch.cuda.synchronize()
    how = "train" if trainable else "frozen"
    print(f"{c['name']}/{how}: entries {spy.entries}")
    per_chunk = [c["logits"], "ce_fwd", "ce_bwd", c["dh"]] + (["tn_256"] if trainable else [])
    if spy.entries != per_chunk * len(_chunks(c)):
        bad.append(f"{how}: launched {spy.entries}, the case states {per_chunk} per chunk")
    if not trainable and "tn_256" in spy.entries:
        bad.append("frozen head: uamd_gemm_tn_256 launched")
    first = [g for g in spy.gemm if g[0] != "tn_256"][::2]          # the logits GEMM of each chunk: hidden states in place
    if any(g[1] != lda for g in first):
        bad.append(f"{how}: the logits GEMM read rows of stride {[g[1] for g in first]}, the hidden states have {lda}")
    acc = [g[2] for g in spy.gemm if g[0] == "tn_256"]
    if trainable and acc != [0] + [1] * (len(_chunks(c)) - 1):
        bad.append(f"train: accumulate flags of the dW launches {acc}")
    if hasattr(Wd, "_uamd_wt") != c["wt"]:
        bad.append(f"{how}: W^T built: {hasattr(Wd, '_uamd_wt')}, the case states {c['wt']}")
    Vp = C.padded(c["V"])
    if [s for s, _ in spy.pad_ok] != [(rows, Vp) for rows in _chunks(c)] or not all(ok for _, ok in spy.pad_ok):
        bad.append(f"{how}: logits chunks / their padding columns stayed zero: {spy.pad_ok}")
    dh = leaf.grad
    if c["view"]:
        if bool(dh[..., C.H:].any()):
            bad.append(f"{how}: gradient in the buffer's columns beyond the view")
        dh = dh[..., :C.H]
    dh = dh.reshape(C.T, C.H)
    dW = Wd.grad if trainable else None
    if not trainable and Wd.grad is not None:
        bad.append("frozen head got a gradient")
    return loss.detach(), dh, dW, bad


def _judge(c, how, tensor, got, bad):
    dt = C.DTYPES[c["dtype"]]
    ref = c["truth"][tensor]
    if got is None or got.dtype != dt or tuple(got.shape) != tuple(ref.shape):
        bad.append(f"{how} {tensor}: {None if got is None else (got.dtype, tuple(got.shape))}, expected {dt} {tuple(ref.shape)}")
        return
    if not bool(torch.isfinite(got.float()).all()):
        bad.append(f"{how} {tensor}: not finite")
        return
    err, model, ratio, ok = C.judge(c, tensor, got)
    i = int(torch.where(err == 0, torch.zeros_like(err), err / model).argmax())
    REPORT[f"{c['name']}/{how}/{tensor}"] = dict(kernel=float(err[i]), model=float(model[i]), ratio=ratio, row=i)
    print(f"{c['name']}/{how}/{tensor}: row {i} kernel {float(err[i]):.3e} model {float(model[i]):.3e} ratio {ratio:.2f}")
    if not ok:
        bad.append(f"{how} {tensor}: row {i} is {ratio:.2f} x the model's error (kernel {float(err[i]):.3e}, model "
                   f"{float(model[i]):.3e})")


@pytest.mark.parametrize("name", ALL)
def test_gradients_row_by_row(name, spy, monkeypatch):
    from unsloth_amd.kernels import utils as U
    c = C.build_case(name)
    monkeypatch.setattr(U, "GEMM256_MODE", c["mode"])
    tr = c["truth"]
    loss_f, dh_f, _, bad = _train_run(c, spy, trainable=False)
    loss_t, dh_t, dW, bad_t = _train_run(c, spy, trainable=True)
    bad += bad_t
    if not torch.equal(dh_f.view(torch.int16), dh_t.view(torch.int16)) or float(loss_f) != float(loss_t):
        bad.append("d(hidden) / the loss differ between the frozen and the trainable head")
    _judge(c, "frozen", "dh", dh_f, bad)
    _judge(c, "train", "dh", dh_t, bad)
    _judge(c, "train", "dW", dW, bad)
    bound = float(tr["b"][tr["live"]].sum()) / tr["n"]
    d = abs(float(loss_f) - float(tr["loss"]))
    REPORT[f"{name}/loss"] = dict(kernel=d, bound=bound, fraction=d / bound)
    print(f"{name}: loss {float(loss_f):.6f} truth {float(tr['loss']):.6f} |d| {d:.3e} bound {bound:.3e}")
    if not d <= bound:
        bad.append(f"loss {float(loss_f)} vs {float(tr['loss'])}: off by {d:.3e}, bound {bound:.3e}")
    assert not bad, "\n".join([name] + bad)


@pytest.mark.parametrize("name", ALL)
def test_row_losses_one_row_at_a_time(name, spy, monkeypatch):
    from unsloth_amd.kernels import utils as U
    c = C.build_case(name)
    monkeypatch.setattr(U, "GEMM256_MODE", c["mode"])
    tr = c["truth"]
    h, W, labels, _ = C.case_inputs(name)
    hidden = h.view(C.B, C.L, C.H).to(DEV).requires_grad_(True)      # both ask for gradients: no_grad() alone must decide
    Wd = torch.nn.Parameter(W.to(DEV))
    lab = labels.to(DEV)
    want = [c["logits"], "ce_fwd"] * len(_chunks(c))
    bad, worst = [], 0.0
    for r in C.checked_rows(name):
        assert bool(tr["live_unmasked"][r])
        mask = torch.zeros(C.T, dtype=torch.bool)
        mask[r] = True
        del spy.entries[:]
        with torch.no_grad():
            loss = _call(c, hidden, Wd, lab, mask=mask.view(C.B, C.L).to(DEV), n_items=1)
        got, ref, b = float(loss), float(tr["row_loss_unmasked"][r]), float(tr["b"][r])
        worst = max(worst, abs(got - ref) / b)
        print(f"{name} row {r}: loss {got:.6f} truth {ref:.6f} |d| {abs(got - ref):.3e} b_r {b:.3e}")
        if not abs(got - ref) <= b:
            bad.append(f"row {r}: loss {got} vs {ref}, off by {abs(got - ref):.3e} = {abs(got - ref) / b:.2f} b_r")
        if spy.entries != want:
            bad.append(f"row {r}: a forward-only call launched {spy.entries}")
        if loss.requires_grad or hidden.grad is not None or Wd.grad is not None:
            bad.append(f"row {r}: a forward-only call left a graph or a gradient")
    REPORT[f"{name}/row_loss"] = dict(worst_fraction_of_b=worst, rows=len(C.checked_rows(name)))
    assert not bad, "\n".join([name] + bad)


# ---- out-of-range labels through the CE kernels ------------------------------------------------------------------------------
# |got - ref| <= REL x |ref| + ATOL per gradient entry: the logits are given in the dtype (no input rounding), the kernel works
# in fp32 -- its logsumexp is within LOSS_FP32 = 2e-5 of the truth (test_cross_entropy's figure), which is a relative 2e-5 on
# every exp(x - lse), and __expf adds a few fp32 ulps of an argument up to ~40: 4e-5 together -- and rounds once to the dtype:
# half an ulp, 2^-8 / 2^-11 relative, or half a subnormal step of fp16 (2^-25) where the entry is that small.
OOR_REL = {torch.bfloat16: 2.0 ** -8 + 4e-5, torch.float16: 2.0 ** -11 + 4e-5, torch.float32: 4e-5}
OOR_ATOL = {torch.bfloat16: 1e-30, torch.float16: 2.0 ** -25, torch.float32: 1e-30}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("softcap,scale", [(0, 0), (30.0, 0.5)])
@pytest.mark.parametrize("fn", ["ce", "logprob"])
def test_out_of_range_labels_are_ignored_rows(fn, softcap, scale, dtype):
    from unsloth_amd.kernels.cross_entropy_loss import Fast_CrossEntropyLoss, Fast_LogProbEntropy
    V, rows = 1001, 12
    g = torch.Generator().manual_seed(1001)
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    labels = torch.randint(0, V, (rows,), generator=g)
    dead = {1: V, 4: V + 7, 6: -1, 9: -100}                        # each between two rows with valid labels
    for r, lab in dead.items():
        labels[r] = lab
    labels[0], labels[5], labels[10] = V - 1, 0, V - 1             # neighbours on the first / last column
    live = torch.tensor([r not in dead for r in range(rows)])
    dl = torch.rand(rows, generator=g) + 0.5
    # fp64 truth
    z = logits.double().requires_grad_(True)
    t = z * scale if scale else z
    t = softcap * torch.tanh(t / softcap) if softcap else t
    ce = torch.nn.functional.cross_entropy(t[live], labels[live], reduction="none")
    sign = 1.0 if fn == "ce" else -1.0
    (sign * ce * dl[live].double()).sum().backward()
    want = z.grad

    lg = logits.to(DEV).requires_grad_(True)
    xin = lg * 1.0
    if fn == "ce":
        out = Fast_CrossEntropyLoss.apply(xin, labels.to(DEV), softcap, scale)
    else:
        out, _ = Fast_LogProbEntropy.apply(xin, labels.to(DEV), softcap, scale)
    out.backward(dl.to(DEV))
    out, grad = out.detach().cpu().double(), lg.grad.cpu()
    for r in dead:
        assert float(out[r]) == 0.0, (r, float(out[r]))
        assert not bool(grad[r].any()), f"row {r} (label {dead[r]}) must have an exactly zero gradient"
    assert float((out[live] - sign * ce.detach()).abs().max()) <= C.LOSS_FP32 * (1 + float(ce.detach().max()))
    err = (grad.double() - want).abs()
    assert bool((err <= OOR_REL[dtype] * want.abs() + OOR_ATOL[dtype]).all()), float((err / (want.abs() + 1e-30)).max())
