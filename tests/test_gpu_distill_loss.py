"""-m gpu: the full-vocabulary distillation loss (csrc/distill_loss.hip: uamd_distill_loss_forward / _backward) through
`_distill_forward` / `_distill_backward_`, `fast_generalized_jsd_loss` and `chunked_hidden_states_distillation_loss`.

Reference, written here: fp64 on the CPU from the same 16-bit (or fp32) inputs, the definition of TRL's generalized_jsd_loss
summed over the vocabulary -- log_softmax of both logits / tau, KL sums with the terms of weight 0 left out, the mixture
through logsumexp -- and its gradient by autograd.

Bounds. Loss: 1e-3 (ln V + 1), the entropy sibling's (tests/test_gpu_logprob_entropy.py). Gradient, per row: the worst
|dz - dz_ref| over the row against the worst error of dz_ref ROUNDED ONCE to the dtype over the same row; the kernel does its
arithmetic in fp32 and rounds once, so the ratio is 1 plus what the fp32 arithmetic adds. Measured on an MI355X over every
case below (each prints its own): 1.000 (bf16) and 1.002 (fp16) on every row but one, 72.4 at worst in fp32 (where "rounded
once" is 2^-25 relative and every fp32 operation of the formula adds as much). The one row: the student one-hot-dominated
(q = 1 - 2e-6 on one column) under the reverse KL, whose largest gradient element is q ((log q - log p) - RKL) with the
bracket cancelling to 1 - q of its terms -- an fp32 ulp of those terms (1e-6) against a gradient of 1e-5: 37.1 (bf16), 28.1
(fp16), an absolute error of 1e-6 |dloss|. GRAD_MARGIN / CANCELLING_ROW_MARGIN are set from those figures (DESIGN.md section 9,
"Distillation loss")."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32

GRAD_MARGIN = {BF: 1.25, HF: 1.25, F32: 128.0}
CANCELLING_ROW_MARGIN = 64.0            # row 5 of `_inputs`, 16-bit cases
#        name: (V, layout, dtype, rows, label dtype)     V <= 4096: a wave per row; above: a block per row / per chunk
SHAPES = {
    "v1000": (1000, "dense", BF, 3, torch.int64),                # fewer vectors than lanes take two trips
    "v1001": (1001, "dense", BF, 65, torch.int32),               # scalar tail; 65 rows: a last block with one live wave
    "v6496": (6496, "dense", BF, 65, torch.int64),               # block per row: two-vector trips + remainder, partial chunk
    "v70000": (70000, "dense", BF, 3, torch.int32),              # > 65536; full backward chunks and a ragged last one
    "v1001_stride1008": (1001, "padded", HF, 65, torch.int64),   # row stride != vocab
    "v1000_offset1": (1000, "offset", BF, 65, torch.int64),      # not 16-byte aligned: the scalar instantiation, wave per row
    "v6496_offset1": (6496, "offset", HF, 3, torch.int32),       # ... block per row
    "v1001_fp32": (1001, "dense", F32, 1, None),                 # one row, no labels
    "v6496_fp32_stride6500": (6496, "padded", F32, 3, torch.int64),
}
PAD = {1001: 1008, 6496: 6500}


def ref_rows(z64, t64, beta, tau):
    """fp64 per-row divergence; a term whose weight is 0 is left out of its sum."""
    lq, lp = torch.log_softmax(z64 / tau, -1), torch.log_softmax(t64 / tau, -1)

    def kl(la, lb):
        w = la > -math.inf
        la0, lb0 = torch.where(w, la, 0.0), torch.where(w, lb, 0.0)
        return torch.where(w, la0.exp() * (la0 - lb0), 0.0).sum(-1)

    if beta == 0:
        return kl(lp, lq)
    if beta == 1:
        return kl(lq, lp)
    lm = torch.logsumexp(torch.stack([lp + math.log(beta), lq + math.log1p(-beta)]), 0)
    return beta * kl(lp, lm) + (1 - beta) * kl(lq, lm)


@functools.lru_cache(maxsize=None)
def _inputs(shape, both_masked):
    """(student, teacher) on the CPU in the case's dtype, labels or None, upstream dloss. Rows by index, where the case has
    them: 1 masked, 2 -inf teacher logits on every third column (`both_masked`, for the reverse KL whose reference is +inf
    where only the teacher is -inf: the student too), 3 student == teacher, 4 teacher one-hot-dominated, 5 student."""
    V, _, dtype, rows, ldt = SHAPES[shape]
    g = torch.Generator().manual_seed(4321 + V)
    z, t = torch.randn(rows, V, generator=g) * 2, torch.randn(rows, V, generator=g) * 2
    if rows > 2:
        t[2, ::3] = -math.inf
        if both_masked:
            z[2, ::3] = -math.inf
    if rows > 5:
        t[3] = z[3]
        t[4] = -10.0
        t[4, 17] = 10.0
        z[5] = -10.0
        z[5, V - 1] = 10.0
    labels = None
    if ldt is not None:
        labels = torch.randint(0, V, (rows,), generator=g).to(ldt)
        labels[1] = -100
    return z.to(dtype), t.to(dtype), labels, torch.randn(rows, generator=g)


def _on_device(x, layout):
    rows, V = x.shape
    if layout == "dense":
        return x.to(DEV)
    if layout == "padded":
        d = torch.zeros(rows, PAD[V], dtype=x.dtype, device=DEV)[:, :V]
    else:
        d = torch.zeros(rows * V + 1, dtype=x.dtype, device=DEV)[1:].view(rows, V)
        assert d.data_ptr() % 16 != 0
    d.copy_(x)
    return d


def _reference(z, t, labels, dloss, beta, tau):
    """fp64 (loss [rows], d sum(loss * dloss) / dz [rows, V]) with the masked rows at 0."""
    live = torch.ones(z.shape[0], dtype=torch.float64) if labels is None else (labels != -100).double()
    z64 = z.double().requires_grad_(True)
    loss = ref_rows(z64, t.double(), beta, tau) * live
    (loss * dloss.double()).sum().backward()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(z64.grad).all())
    return loss.detach(), z64.grad


def _check_grad(dz, want, dtype, skip, tag, cancelling=None):
    """Per row: worst |dz - want| over worst |round(want) - want|; rows in `skip` (reference gradient identically 0) left out,
    row `cancelling` held to its own margin."""
    err = (dz.double().cpu() - want).abs().amax(-1)
    unit = (want.to(dtype).double() - want).abs().amax(-1)
    rows = [r for r in range(want.shape[0]) if r not in skip and r != cancelling and unit[r] > 0]
    worst = max((err[r] / unit[r]).item() for r in rows)
    print(f"gradient {tag}: worst row ratio {worst:.3f} (margin {GRAD_MARGIN[dtype]})")
    assert worst <= GRAD_MARGIN[dtype], (tag, worst)
    if cancelling is not None:
        ratio = (err[cancelling] / unit[cancelling]).item()
        print(f"gradient {tag}: cancelling row ratio {ratio:.3f} (margin {CANCELLING_ROW_MARGIN})")
        assert ratio <= CANCELLING_ROW_MARGIN, (tag, ratio)


@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_loss_and_gradient_match_fp64(shape, beta, tau):
    from unsloth_amd.kernels.cross_entropy_loss import _distill_backward_, _distill_forward
    V, layout, dtype, rows, _ = SHAPES[shape]
    z, t, labels, dloss = _inputs(shape, beta == 1.0)
    want_loss, want_dz = _reference(z, t, labels, dloss, beta, tau)
    dz, dt = _on_device(z, layout), _on_device(t, layout)
    lab = labels.to(DEV) if labels is not None else None
    loss, lse_s, lse_t, kl_s = _distill_forward(dz, dt, lab, beta, tau)
    _distill_backward_(dz, dt, dloss.to(DEV), lse_s, lse_t, kl_s, lab, beta, tau)      # dz <- gradient, in place
    got = loss.double().cpu()
    bound = 1e-3 * (math.log(V) + 1)
    err = (got - want_loss).abs().max().item()
    print(f"loss {shape} beta={beta} tau={tau}: worst |loss - ref| = {err:.3e} (bound {bound:.3e})")
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(dz.float()).all())
    assert err <= bound, err
    assert torch.equal(dt.cpu(), t)                                  # the teacher is read only
    skip = set()
    if labels is not None:                                           # masked: loss 0 and an exactly zero gradient row
        assert got[1].item() == 0.0 and float(dz[1].float().abs().max()) == 0.0
        skip.add(1)
    if rows > 5:                                                     # student == teacher: no divergence, no gradient
        assert abs(got[3].item()) <= bound and float(dz[3].float().abs().max()) <= 1e-5
        skip.add(3)
    _check_grad(dz, want_dz, dtype, skip, f"{shape} beta={beta} tau={tau}", cancelling=5 if rows > 5 else None)


@pytest.mark.parametrize("reduction", ["batchmean", "sum", "mean", "none"])
def test_public_entry_reductions_and_autograd(reduction):
    from unsloth_amd.kernels import fast_generalized_jsd_loss
    B, L, V, beta, tau = 2, 5, 1000, 0.3, 1.5
    g = torch.Generator().manual_seed(7)
    z, t = (torch.randn(B, L, V, generator=g) * 2).to(BF), (torch.randn(B, L, V, generator=g) * 2).to(BF)
    labels = torch.randint(0, V, (B, L), generator=g)
    labels[0, 0] = labels[1, 3] = -100
    live = (labels != -100).reshape(-1).double()
    z64 = z.double().reshape(-1, V).requires_grad_(True)
    rows = ref_rows(z64, t.double().reshape(-1, V), beta, tau) * live
    up = torch.randn(B, L, generator=g).double()
    want = {"batchmean": rows.sum() / live.sum(), "sum": rows.sum(), "mean": rows.sum() / (live.sum() * V),
            "none": rows.view(B, L)}[reduction]
    (want * up).sum().backward() if reduction == "none" else want.backward()
    zd = z.to(DEV).requires_grad_(True)
    got = fast_generalized_jsd_loss(zd, t.to(DEV), labels.to(DEV), beta=beta, temperature=tau, reduction=reduction)
    (got * up.to(DEV)).sum().backward() if reduction == "none" else got.backward()
    assert got.dtype == torch.float32 and got.shape == want.shape
    n_summed = live.sum().item() if reduction == "sum" else 1          # a sum of n rows: n times a row's bound
    assert (got.detach().double().cpu() - want.detach()).abs().max().item() <= 1e-3 * (math.log(V) + 1) * n_summed
    _check_grad(zd.grad.reshape(-1, V), z64.grad, BF, {0, 8}, f"public entry {reduction}")


@pytest.mark.parametrize("teacher_as", ["hidden", "logits"])
def test_chunked_driver_matches_unchunked_fp64(teacher_as):
    """hidden 256, V 1000, 70 rows in chunks of 32 (32 + 32 + 6). The operands are small integers over powers of two, so every
    logit is exact in fp32 whatever the GEMM's summation order and its rounding to bf16 is the reference's. d(hidden) =
    dlogits @ W with dlogits rounded to bf16 (2^-9 relative each), the product rounded to bf16 and rounded once more after the
    upstream 1 / n: |d(hidden) - ref| <= 3 * 2^-9 * (|dlogits| @ |W|), element by element."""
    from unsloth_amd.models.rl_replacements import chunked_hidden_states_distillation_loss as f
    T, H, Ht, V, beta, tau = 70, 256, 128, 1000, 0.5, 2.0
    g = torch.Generator().manual_seed(11)
    h = (torch.randint(-2, 3, (T, H), generator=g) / 4).to(BF)
    W = (torch.randint(-32, 33, (V, H), generator=g) / 64).to(BF)
    ht = (torch.randint(-2, 3, (T, Ht), generator=g) / 4).to(BF)
    Wt = (torch.randint(-32, 33, (V, Ht), generator=g) / 64).to(BF)
    labels = torch.randint(0, V, (T,), generator=g)
    labels[5] = labels[40] = labels[69] = -100
    live = (labels != -100).double()
    z64 = (h.float() @ W.float().t()).to(BF).double().requires_grad_(True)
    t_logits = (ht.float() @ Wt.float().t()).to(BF)
    want = (ref_rows(z64, t_logits.double(), beta, tau) * live).sum() / live.sum()
    want.backward()
    want_dh, tol = z64.grad @ W.double(), 3 * 2.0 ** -9 * (z64.grad.abs() @ W.double().abs())
    hd = h.to(DEV).requires_grad_(True)
    teacher = (ht.to(DEV), Wt.to(DEV)) if teacher_as == "hidden" else (t_logits.to(DEV), None)
    got = f(hd, teacher[0], W.to(DEV), teacher[1], labels.to(DEV), beta, tau, chunk_rows=32)
    got.backward()
    err, over = abs(got.item() - want.item()), ((hd.grad.double().cpu() - want_dh).abs() - tol).max().item()
    print(f"driver teacher as {teacher_as}: |loss - ref| = {err:.3e} (bound {1e-3 * (math.log(V) + 1):.3e}), "
          f"worst |d hidden - ref| - tol = {over:.3e}, worst |d hidden - ref| / tol = "
          f"{((hd.grad.double().cpu() - want_dh).abs() / tol.clamp(min=1e-300)).max().item():.3f}")
    assert err <= 1e-3 * (math.log(V) + 1)
    assert over <= 0 and float(hd.grad[5].abs().max()) == 0.0
