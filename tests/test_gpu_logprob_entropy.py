"""-m gpu: per-token entropy from the log-prob kernel's own pass over the logits (uamd_logprob_entropy_forward,
`return_entropy=True` of the two chunked log-prob entry points, `compute_entropy=True` of the GRPO driver).

Reference, written here: fp64 on the CPU, H = lse - sum_{p > 0} p * z over the transformed logits z (scale, then soft cap),
p = exp(z - lse). On given logits the bound is 1e-3 (ln V + 1), the bound tests/test_gpu_rl_logprobs.py has for log-probs
computed from given logits (the same formula in fp32 is 6e-7 off fp64 on these inputs); through the lm_head GEMM it is
2e-3 (ln V + 1) against logits rounded to bf16 where the product rounds them, that path's log-prob bound.

Measured on an MI355X: worst |H - H_ref| 1.7e-6 over the given-logits cases (each case prints its own), 9.0e-5 through the
lm_head GEMM, 1.1e-6 in the driver; DESIGN.md section 9, "Per-token entropy"."""
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

MODES = {"plain": (0.0, 0.0), "scale": (0.0, 1.0 / 0.9), "cap": (30.0, 0.0), "cap_scale": (30.0, 1.0 / 0.9)}
#        name: (V, layout, dtype, rows)
SHAPES = {
    "v1000": (1000, "dense", torch.bfloat16, 16),           # fewer 16-byte vectors than threads
    "v1001": (1001, "dense", torch.bfloat16, 16),           # scalar tail
    "v6496": (6496, "dense", torch.bfloat16, 16),           # the two-vector trip plus the single-vector remainder
    "v70000": (70000, "dense", torch.bfloat16, 8),          # > 65536
    "v1001_stride1008": (1001, "padded", torch.bfloat16, 16),   # row stride != vocab
    "v1000_offset1": (1000, "offset", torch.bfloat16, 16),  # starts one element into its buffer: the non-vector path
    "v1001_fp16": (1001, "dense", torch.float16, 16),
    "v1001_fp32": (1001, "dense", torch.float32, 16),
}


def ref_transform(x64, softcap, scale):
    z = x64
    if scale:
        z = z * scale
    if softcap:
        z = softcap * torch.tanh(z / softcap)
    return z


def ref_entropy(z64):
    """fp64: lse - sum over p > 0 of p * z."""
    lse = torch.logsumexp(z64, dim=-1)
    p = torch.exp(z64 - lse.unsqueeze(-1))
    pz = torch.where(p > 0, p * torch.where(p > 0, z64, torch.zeros_like(z64)), torch.zeros_like(z64))
    return lse - pz.sum(-1)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(logits on the CPU in the case's dtype [rows, V], index [rows] with two -100 rows); computed once per shape."""
    V, _, dtype, rows = SHAPES[shape]
    g = torch.Generator().manual_seed(1234 + V)
    x = torch.randn(rows, V, generator=g) * 3
    x[0] = 1.5                                              # all equal: H = ln V
    x[1] = -20.0
    x[1, 17] = 20.0                                         # H ~ 0
    x[2, 100:] = -math.inf                                  # masked vocabulary
    x[3] = -math.inf
    x[3, V - 1] = 0.75                                      # one column left: H = 0
    idx = torch.randint(0, V, (rows,), generator=g)
    idx[2] = 5
    idx[3] = V - 1
    idx[4] = -100
    idx[rows - 1] = -100
    return x.to(dtype), idx


def _on_device(shape):
    """The case's logits on the GPU in the layout under test, as a [rows, V] view."""
    V, layout, dtype, rows = SHAPES[shape]
    x, idx = _inputs(shape)
    if layout == "dense":
        d = x.to(DEV)
    elif layout == "padded":
        buf = torch.zeros(rows, 1008, dtype=dtype, device=DEV)
        d = buf[:, :V]
        d.copy_(x)
    else:
        buf = torch.zeros(rows * V + 1, dtype=dtype, device=DEV)
        d = buf[1:].view(rows, V)
        d.copy_(x)
        assert d.data_ptr() % 16 != 0
    return d, idx.to(DEV)


@functools.lru_cache(maxsize=None)
def _want(shape, mode):
    x, _ = _inputs(shape)
    cap, scale = MODES[mode]
    return ref_entropy(ref_transform(x.double(), cap, scale))


def _check_entropy(got, want, V, tag):
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), (tag, got)
    err = (got - want).abs().max().item()
    print(f"entropy {tag}: worst |H - H_ref| = {err:.3e} (bound {1e-3 * (math.log(V) + 1):.3e})")
    assert got.min().item() >= -1e-4 and got.max().item() <= math.log(V) + 1e-3, (tag, got.min().item(), got.max().item())
    assert err <= 1e-3 * (math.log(V) + 1), (tag, err)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_entropy_matches_fp64_formula(shape, mode):
    from unsloth_amd.kernels.cross_entropy_loss import _logprob_entropy_forward
    V = SHAPES[shape][0]
    cap, scale = MODES[mode]
    d, idx = _on_device(shape)
    lp, lse, ent = _logprob_entropy_forward(d, idx, cap, scale)
    assert ent.dtype == torch.float32 and ent.shape == (d.shape[0],)
    want = _want(shape, mode)
    assert abs(want[0].item() - math.log(V)) < 1e-9                # the reference on the rows whose entropy is known
    if not cap:                                                     # (the soft cap maps -inf to -cap: no longer masked)
        assert want[1].item() < 1e-9 and want[3].item() == 0.0       # (V - 1) e^-40 (40 + ...) ~ 1e-11 at V = 70000
    _check_entropy(ent, want, V, f"kernel {shape} {mode}")


@pytest.mark.parametrize("mode", ["plain", "scale"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_logits_entry_entropy_matches_fp64_formula(shape, mode):
    from unsloth_amd.models.rl_replacements import chunked_selective_log_softmax
    V, _, _, rows = SHAPES[shape]
    d, idx = _on_device(shape)
    idx = idx.clamp(min=0)
    lp, ent = chunked_selective_log_softmax(d.unsqueeze(0), idx.unsqueeze(0), temperature=0.9 if mode == "scale" else 1.0,
                                            return_entropy=True)
    assert lp.shape == ent.shape == (1, rows) and ent.dtype == torch.float32 and not ent.requires_grad
    _check_entropy(ent[0], _want(shape, mode), V, f"logits entry {shape} {mode}")
    x, _ = _inputs(shape)
    z = ref_transform(x.double(), *MODES[mode])
    want_lp = (z - torch.logsumexp(z, -1, keepdim=True)).gather(-1, idx.cpu().unsqueeze(-1)).squeeze(-1)
    assert (lp[0].double().cpu() - want_lp).abs().max().item() <= 1e-3 * (want_lp.abs().max().item() + 1)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_logprob_and_lse_are_the_cross_entropy_forwards_bits(shape, mode):
    from unsloth_amd.kernels.cross_entropy_loss import _ce_forward, _logprob_entropy_forward
    cap, scale = MODES[mode]
    d, idx = _on_device(shape)
    losses, lse0 = _ce_forward(d, idx, cap, scale)
    lp, lse1, ent = _logprob_entropy_forward(d, idx, cap, scale)
    assert torch.equal(lse0, lse1)
    assert torch.equal(lp, -losses)
    ignored = (idx == -100)
    assert int(ignored.sum()) == 2 and float(lp[ignored].abs().max()) == 0.0
    # index -100 rows still get their entropy
    want = _want(shape, mode)[ignored.cpu()]
    V = SHAPES[shape][0]
    assert (ent[ignored].double().cpu() - want).abs().max().item() <= 1e-3 * (math.log(V) + 1)


def _hidden_case(B, L, H, V, wscale=0.1, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(B, L, H, generator=g) * 0.5).to(torch.bfloat16)
    W = (torch.randn(V, H, generator=g) * wscale).to(torch.bfloat16)
    idx = torch.randint(0, V, (B, L), generator=g)
    return h, W, idx


def test_flag_leaves_logprobs_and_gradient_bitwise_alone():
    from unsloth_amd.models.rl_replacements import chunked_hidden_states_selective_log_softmax as f
    B, L, H, V = 2, 96, 256, 1000
    h, W, idx = _hidden_case(B, L, H, V, 0.4)
    idx[0, 3] = -100
    idx[1, 95] = -100
    up = torch.randn(B, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    Wd, idxd = W.to(DEV), idx.to(DEV)
    h0 = h.to(DEV).requires_grad_(True)
    lp0 = f(h0, Wd, idxd, temperature=0.9)
    (lp0 * up).sum().backward()
    h1 = h.to(DEV).requires_grad_(True)
    lp1, ent = f(h1, Wd, idxd, temperature=0.9, return_entropy=True)
    assert ent.requires_grad is False and ent.dtype == torch.float32 and ent.shape == (B, L)
    (lp1 * up).sum().backward()
    assert torch.equal(lp0.detach(), lp1.detach())
    assert torch.equal(h0.grad, h1.grad)
    ignored = (idx == -100)
    assert float(lp1.detach().cpu()[ignored].abs().max()) == 0.0
    z = (h.float() @ W.float().t()).to(torch.bfloat16).double() / 0.9
    want = ref_entropy(z)
    assert (ent.double().cpu() - want)[ignored].abs().max().item() <= 2e-3 * (math.log(V) + 1)


@pytest.mark.parametrize("B,L,H,V,wscale,kw", [
    (2, 96, 256, 1000, 0.4, {}),                            # entropies spread over roughly 1-4 nats
    (1, 300, 512, 32000, 0.1, dict(temperature=0.7)),
    (2, 40, 256, 32001, 0.1, {}),                           # vocab % 8 != 0: padded row stride
    (1, 513, 256, 1000, 0.1, dict(chunks=3)),               # chunk boundaries are crossed
])
def test_hidden_states_entry_entropy(B, L, H, V, wscale, kw):
    from unsloth_amd.models.rl_replacements import chunked_hidden_states_selective_log_softmax as f
    h, W, idx = _hidden_case(B, L, H, V, wscale)
    temp = kw.get("temperature", 1.0)
    lg = h.float() @ W.float().t()
    want_lp = torch.log_softmax(lg / temp, dim=-1).gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    want = ref_entropy(lg.to(torch.bfloat16).double() / temp)   # the product's (and the reference library's) rounding point
    lp, ent = f(h.to(DEV), W.to(DEV), idx.to(DEV), return_entropy=True, **kw)
    assert lp.shape == ent.shape == (B, L) and ent.dtype == torch.float32 and not ent.requires_grad
    got = ent.double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs().max().item()
    print(f"hidden-state entry V={V} L={L}: entropy {want.min().item():.3f}..{want.max().item():.3f} nats, "
          f"worst |H - H_ref| = {err:.3e} (bound {2e-3 * (math.log(V) + 1):.3e})")
    assert err <= 2e-3 * (math.log(V) + 1), err
    assert (lp.cpu() - want_lp).abs().max().item() <= 2e-3 * (want_lp.abs().max().item() + 1.0)


def test_entropy_costs_no_fp32_weight_copy():
    from unsloth_amd.models.rl_replacements import chunked_hidden_states_selective_log_softmax as f
    h, W, idx = _hidden_case(1, 300, 512, 32000)
    h, W, idx = h.to(DEV), W.to(DEV), idx.to(DEV)
    f(h, W, idx, return_entropy=True)                       # warm-up: allocator pools, cached operands
    peak = {}
    for flag in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = f(h, W, idx, return_entropy=flag)
        torch.cuda.synchronize()
        peak[flag] = torch.cuda.max_memory_allocated()
        del out
    print(f"peak allocated: log-probs {peak[False]} B, with entropy {peak[True]} B, delta {peak[True] - peak[False]} B")
    assert peak[True] - peak[False] <= 1 << 20


def _left_padded_batch(gen, B=4, P=24, C=40, vocab=1000, pad=0):
    ids = torch.full((B, P + C), pad)
    mask = torch.zeros(B, P + C, dtype=torch.long)
    plen, clen = [24, 7, 15, 20], [40, 11, 33, 1]
    for b in range(B):
        ids[b, P - plen[b]:P] = torch.randint(1, vocab, (plen[b],), generator=gen)
        ids[b, P:P + clen[b]] = torch.randint(1, vocab, (clen[b],), generator=gen)
        mask[b, P - plen[b]:P + clen[b]] = 1
    return ids, mask


def test_driver_entropy_of_left_padded_rows():
    from tests.test_gpu_model import _tiny
    from unsloth_amd.models.rl_replacements import _packed_completion_index, get_per_token_logps_and_entropies
    model = _tiny(load_in_4bit=True, gc=False, head_dim=128, r=8)
    ids, mask = _left_padded_batch(torch.Generator().manual_seed(7))
    C, V = 40, 1000
    ids_d, mask_d = ids.to(DEV), mask.to(DEV)
    lp, ent = get_per_token_logps_and_entropies(model, ids_d, mask_d, C, temperature=0.9, compute_entropy=True)
    lp0, none = get_per_token_logps_and_entropies(model, ids_d, mask_d, C, temperature=0.9, compute_entropy=False)
    assert none is None and torch.equal(lp.detach(), lp0.detach())
    assert ent.shape == (4, C) and ent.dtype == torch.float32 and not ent.requires_grad
    cm = mask[:, -C:].bool()
    assert float(ent.cpu()[~cm].abs().max()) == 0.0         # padding columns stay 0
    # the hidden states of the same packed forward, the same row selection, logits rounded to bf16 where the product rounds
    flat_ids, pos, lens, src, _, (dst_r, dst_c) = _packed_completion_index(ids_d, mask_d, C)
    prev = os.environ.get("UNSLOTH_RETURN_HIDDEN_STATES")
    os.environ["UNSLOTH_RETURN_HIDDEN_STATES"] = "1"
    try:
        with torch.no_grad():
            hidden = model(input_ids=flat_ids, position_ids=pos.to(torch.int32), packed_seq_lengths=lens, use_cache=False).logits
    finally:
        if prev is None:
            os.environ.pop("UNSLOTH_RETURN_HIDDEN_STATES", None)
        else:
            os.environ["UNSLOTH_RETURN_HIDDEN_STATES"] = prev
    W = model.get_base_model().get_output_embeddings().weight
    rows = hidden[0].index_select(0, src).float().cpu()
    z = (rows @ W.detach().float().cpu().t()).to(torch.bfloat16).double() / 0.9
    want = torch.zeros(4, C, dtype=torch.float64).index_put_((dst_r.cpu(), dst_c.cpu()), ref_entropy(z))
    assert int(cm.sum()) == z.shape[0]
    err = (ent.double().cpu() - want)[cm].abs().max().item()
    print(f"driver: worst |H - H_ref| on completion columns = {err:.3e} (bound {2e-3 * (math.log(V) + 1):.3e})")
    assert err <= 2e-3 * (math.log(V) + 1), err
