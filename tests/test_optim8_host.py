"""CPU: the 8-bit AdamW state (optim="adamw_8bit") -- make_optimizer's dispatch, and ShardedAdamW(optim_bits=8)'s host branch
against a restatement of the block-wise rule written here (not imported from the product): per 256-element block, decode
m = code_m[m8] * absmax_m, v = code_v[v8] * absmax_v; AdamW with decoupled decay on the fp32 moments; new absmax = max |m| /
max v; code = nearest map entry to m / absmax (torch.bucketize on the midpoints); absmax 0 stores the code of 0.0."""
import copy

import pytest
import torch

from unsloth_amd.nf4 import create_dynamic_map

QB = 256
CODE_M, CODE_V = create_dynamic_map(signed=True), create_dynamic_map(signed=False)


def encode(x, code, signed):
    n = x.numel()
    xp = torch.nn.functional.pad(x, (0, (-n) % QB)).view(-1, QB)
    absmax = (xp.abs() if signed else xp).amax(dim=1)
    scaled = torch.where(absmax[:, None] > 0, xp / absmax[:, None], torch.zeros_like(xp)).reshape(-1)[:n]
    return torch.bucketize(scaled.contiguous(), (code[:-1] + code[1:]) / 2).to(torch.uint8), absmax


def decode(codes, absmax, code):
    return code[codes.long()] * absmax.repeat_interleave(QB)[:codes.numel()]


def restated_step(p, g, m8, v8, am, av, t, lr, wd, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """One step of the rule on flat fp32 `p`, `g` and the 8-bit state; `wd` a scalar or a per-element tensor. Returns the
    new (p, m8, v8, absmax_m, absmax_v). fp32 throughout, every constant formed in double and rounded once."""
    dev = p.device
    f = lambda x: torch.as_tensor(x, dtype=torch.float64).to(torch.float32).to(dev)
    code_m, code_v = CODE_M.to(dev), CODE_V.to(dev)
    m, v = decode(m8, am, code_m), decode(v8, av, code_v)
    g = g * f(grad_scale)
    p = p - f(lr * torch.as_tensor(wd, dtype=torch.float64)) * p
    m = f(b1) * m + f(1.0 - b1) * g
    v = f(b2) * v + f(1.0 - b2) * g * g
    p = p - f(lr / (1.0 - b1 ** t)) * m / (v.sqrt() / f((1.0 - b2 ** t) ** 0.5) + f(eps))
    m8, am = encode(m, code_m, True)
    v8, av = encode(v, code_v, False)
    return p, m8, v8, am, av


def zero_state(n, dev="cpu"):
    nblk = (n + QB - 1) // QB
    return (torch.full((n,), 127, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
            torch.zeros(nblk, device=dev), torch.zeros(nblk, device=dev))


def check_codes(got, want, what=""):
    """The mismatch condition: at most 1 code in 4096 differs, each by exactly one step of the sorted map. Returns the mask
    of differing elements."""
    d = (got.reshape(-1).int() - want.reshape(-1).int()).abs()
    n_bad = int((d != 0).sum())
    print(f"{what}: {n_bad} of {d.numel()} codes differ, largest step {int(d.max()) if d.numel() else 0}")
    assert int(d.max()) <= 1 if d.numel() else True, f"{what}: a code is {int(d.max())} steps off"
    assert n_bad * 4096 <= d.numel(), f"{what}: {n_bad} of {d.numel()} codes differ (more than 1 in 4096)"
    return d != 0


def test_maps_are_what_the_rule_assumes():
    for code in (CODE_M, CODE_V):
        assert code.shape == (256,) and bool((code[1:] > code[:-1]).all()) and float(code[-1]) == 1.0
    assert float(CODE_M[127]) == 0.0 and float(CODE_V[0]) == 0.0 and float(CODE_M[0]) < 0


# ---- make_optimizer ----------------------------------------------------------------------------------------------------
def test_make_optimizer_dispatch():
    from unsloth_amd.optim import FlatAdamW
    from unsloth_amd.trainer import make_optimizer
    lin = torch.nn.Linear(8, 4, bias=False)
    opt = make_optimizer(lin)
    assert isinstance(opt, torch.optim.AdamW) and not isinstance(opt, FlatAdamW)             # the default is untouched
    for name in (None, "adamw_torch", "adamw_torch_fused"):
        assert type(make_optimizer(lin, optim=name)) is torch.optim.AdamW
    for name in ("adamw_8bit", "adamw_bnb_8bit", "paged_adamw_8bit"):
        with pytest.raises(NotImplementedError, match=name):                                 # accepted, but not on the CPU
            make_optimizer(lin, optim=name)
    with pytest.raises(NotImplementedError):
        make_optimizer(lin, optim="adamw_8bit", flat=False)
    with pytest.raises(ValueError, match="adamw_8bit.*adamw_bnb_8bit.*paged_adamw_8bit"):
        make_optimizer(lin, optim="adamw_apex_fused")
    with pytest.raises(ValueError, match="adamw_torch"):
        make_optimizer(lin, optim="lion_8bit")


def test_optim_bits_is_8_or_32():
    from unsloth_amd.full_finetune import ShardedAdamW
    from unsloth_amd.optim import FlatAdamW
    with pytest.raises(ValueError, match="optim_bits"):
        ShardedAdamW(Tiny(), optim_bits=4)
    with pytest.raises(ValueError, match="optim_bits"):
        FlatAdamW(torch.nn.Linear(8, 4, bias=False), optim_bits=16)


# ---- ShardedAdamW(optim_bits=8), host branch ---------------------------------------------------------------------------
class Tiny(torch.nn.Module):
    """With the default sizes, buckets (backward order): head = final norm [24] + lm_head [40 x 24] (the decay boundary at element 24, INSIDE quant
    block 0), two layers = q_proj [24 x 24] + norm [24] (576 + 24 -> shard 640: two full blocks and a partial one, the
    boundary at 576 inside block 2), embedding [40 x 24]."""

    def __init__(self, seed=0, hidden=24, vocab=40):
        super().__init__()
        torch.manual_seed(seed)
        self.model = torch.nn.Module()
        self.model.embed_tokens = torch.nn.Embedding(vocab, hidden)
        self.model.layers = torch.nn.ModuleList()
        for _ in range(2):
            blk = torch.nn.Module()
            blk.q_proj = torch.nn.Linear(hidden, hidden, bias=False)
            blk.norm = torch.nn.LayerNorm(hidden, bias=False)
            self.model.layers.append(blk)
        self.model.norm = torch.nn.LayerNorm(hidden, bias=False)
        self.lm_head = torch.nn.Linear(hidden, vocab, bias=False)
        with torch.no_grad():
            for p in self.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))


def _grads(opt, step, sigma=0.1):
    """Fixed Gaussian gradients written into the gradient buckets (what backward + finish() would leave there)."""
    gen = torch.Generator().manual_seed(1000 + step)
    for b in opt.buckets.buckets:
        b["flat_g"].copy_((torch.randn(b["numel"], generator=gen) * sigma).to(b["flat_g"].dtype))


def _decay_vector(opt, bi, wd):
    b = opt.buckets.buckets[bi]
    w = torch.zeros(b["numel"], dtype=torch.float64)
    for p, o in zip(b["params"], b["offsets"]):
        if p.dim() > 1:
            w[o:o + p.numel()] = wd
    return w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sharded_adamw8_host_matches_the_restatement(dtype):
    from unsloth_amd.full_finetune import ShardedAdamW
    lr, wd = 1e-3, 0.1
    model = Tiny().to(dtype)
    opt = ShardedAdamW(model, lr=lr, weight_decay=wd, optim_bits=8)
    B = opt.buckets
    assert any(b["shard"] % QB for b in B.buckets) and any(p.dim() == 1 for p in model.parameters())
    ref = [(opt.master[bi].clone(),) + zero_state(b["shard"]) for bi, b in enumerate(B.buckets)]
    start = [m.clone() for m in opt.master]
    # the state size: 2 B per element + two fp32 scales per block
    n_total = 0
    for bi, b in enumerate(B.buckets):
        n = b["shard"]
        n_total += 2 * n + 8 * ((n + QB - 1) // QB)
    assert opt.moment_bytes() == n_total
    assert ShardedAdamW(Tiny().to(dtype), optim_bits=32).moment_bytes() == 8 * sum(b["shard"] for b in B.buckets)
    for step in range(1, 6):
        _grads(opt, step)
        opt.step()
        for bi, b in enumerate(B.buckets):
            p, m8, v8, am, av = ref[bi]
            ref[bi] = restated_step(p, b["flat_g"].float(), m8, v8, am, av, step, lr, _decay_vector(opt, bi, wd))
    for bi, b in enumerate(B.buckets):
        p, m8, v8, am, av = ref[bi]
        torch.testing.assert_close(opt.master[bi], p, rtol=1e-5, atol=1e-6)
        check_codes(opt.exp_avg[bi], m8, f"bucket {bi} state1")
        check_codes(opt.exp_avg_sq[bi], v8, f"bucket {bi} state2")
        torch.testing.assert_close(opt.absmax_m[bi], am, rtol=1e-6, atol=0)
        torch.testing.assert_close(opt.absmax_v[bi], av, rtol=1e-6, atol=0)
        assert torch.equal(B.param_shard(bi), opt.master[bi].to(dtype))                      # rounded once from the master
        assert float((opt.master[bi] - start[bi]).abs().max()) > 1e-3                        # (it moved)
    # a 1-D parameter sees no decay: the same run with weight_decay = 0 moves it identically, a 2-D one differently
    model0 = Tiny().to(dtype)
    opt0 = ShardedAdamW(model0, lr=lr, weight_decay=0.0, optim_bits=8)
    for step in range(1, 6):
        _grads(opt0, step)
        opt0.step()
    for (n, p), (_, q) in zip(model.named_parameters(), model0.named_parameters()):
        if p.dim() == 1:
            assert torch.equal(p.data, q.data), n
        else:
            assert not torch.equal(p.data, q.data), n
    opt.buckets.close()
    opt0.buckets.close()


def test_sharded_adamw8_state_dict_round_trip_and_cross_width_refusal():
    from unsloth_amd.full_finetune import ShardedAdamW

    def run(opt, steps):
        for step in steps:
            _grads(opt, step)
            opt.step()

    a = ShardedAdamW(Tiny().bfloat16(), lr=1e-3, weight_decay=0.1, optim_bits=8)
    run(a, (1, 2))
    saved = copy.deepcopy(a.state_dict())
    assert saved["uamd_sharded"]["blocksize"] == QB and saved["uamd_sharded"]["exp_avg"][0].dtype == torch.uint8
    run(a, (3, 4))
    b = ShardedAdamW(Tiny(seed=5).bfloat16(), lr=1e-3, weight_decay=0.1, optim_bits=8)
    run(b, (7, 8))                                       # (other gradients: everything it holds must come from the load)
    b.load_state_dict(saved)
    run(b, (3, 4))
    for bi in range(len(a.buckets.buckets)):
        assert torch.equal(a.master[bi], b.master[bi])
        assert torch.equal(a.exp_avg[bi], b.exp_avg[bi]) and torch.equal(a.exp_avg_sq[bi], b.exp_avg_sq[bi])
        assert torch.equal(a.absmax_m[bi], b.absmax_m[bi]) and torch.equal(a.absmax_v[bi], b.absmax_v[bi])
        assert torch.equal(a.buckets.buckets[bi]["flat_p"], b.buckets.buckets[bi]["flat_p"])
    c = ShardedAdamW(Tiny().bfloat16(), lr=1e-3, weight_decay=0.1, optim_bits=32)
    with pytest.raises(ValueError, match="optim_bits=8.*optim_bits=32"):
        c.load_state_dict(saved)
    run(c, (1,))
    with pytest.raises(ValueError, match="optim_bits=32.*optim_bits=8"):
        a.load_state_dict(c.state_dict())
    for o in (a, b, c):
        o.buckets.close()


def test_sharded_adamw8_refuses_split_decay_ranges():
    """Decaying parameters on both sides of a one-dimensional one in one bucket: one launch cannot carry two ranges."""
    from unsloth_amd.full_finetune import ShardedAdamW

    class Split(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(8, 8, bias=False)
            self.n = torch.nn.LayerNorm(8, bias=False)
            self.b = torch.nn.Linear(8, 8, bias=False)

    with pytest.raises(NotImplementedError, match="bucket 0"):
        ShardedAdamW(Split(), optim_bits=8)
    ShardedAdamW(Split(), optim_bits=32).buckets.close()                                     # (fp32: two launches, fine)
