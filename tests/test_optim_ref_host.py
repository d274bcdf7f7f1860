"""CPU: what the element-wise AdamW kernel tests (tests/test_gpu_optim_kernels.py, the fp32 optimizer tests of
tests/test_gpu_optim.py and tests/test_gpu_full_finetune.py) stand on.
  * tests/_util.adamw_ref64 is an independent statement of AdamW: pinned to torch.optim.AdamW on float64 tensors;
  * the bound those tests use is 4 x the worst |fp32 - fp64| / (2^-24 x operand scale) of the kernel's arithmetic restated in
    fp32 torch operations (tests/_util.adamw_restated_f32), over all of that module's inputs: recomputed here and held to the
    figures the module records;
  * ShardedAdamW's host branch on the `Awkward` module (the one the GPU tests run) against that restatement: masters and
    moments within the bound, 16-bit parameters equal except where the two masters straddle a rounding boundary -- at most
    1 element in 4096 per step at the seed the GPU test uses."""
import pytest
import torch

from tests._util import adamw_ratio, adamw_ref64, adamw_restated_f32, assert_adamw_close


def test_adamw_ref64_is_torch_adamw():
    gen = torch.Generator().manual_seed(0)
    for betas, wd in (((0.9, 0.999), 0.1), ((0.8, 0.95), 0.0), ((0.0, 0.5), 0.01)):
        p = torch.randn(1000, generator=gen, dtype=torch.float64)
        q = torch.nn.Parameter(p.clone())
        opt = torch.optim.AdamW([q], lr=1e-2, betas=betas, eps=1e-8, weight_decay=wd, foreach=False, fused=False)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step in range(1, 8):
            lr = 1e-2 if step < 4 else 3e-3
            opt.param_groups[0]["lr"] = lr
            g = torch.randn(1000, generator=gen, dtype=torch.float64) * (0.05 + 0.3 * step)
            q.grad = 0.5 * g                                        # (an exact scaling: grad_scale = 0.5 on g)
            opt.step()
            p, m, v, scale = adamw_ref64(p, g, m, v, lr, betas, 1e-8, wd, step, grad_scale=0.5)
            st = opt.state[q]
            for got, want in ((p, q.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert bool(((got - want).abs() <= 1e-12 * want.abs()).all()), (betas, step)
            assert bool((scale["m"] >= m.abs() * (1 - 1e-12)).all()) and bool((scale["v"] >= v * (1 - 1e-12)).all())


def test_fp32_restatement_ratios_are_the_recorded_ones():
    """The three figures in the docstring of tests/test_gpu_optim_kernels.py: measured, not chosen."""
    from tests.test_gpu_optim_kernels import MEASURED, RATIO_BOUND, cases, make_inputs
    worst = dict(p=0.0, m=0.0, v=0.0)
    for gdtype in (torch.float32, torch.bfloat16, torch.float16):
        for n, h in cases():
            p, g, m, v = make_inputs(n, gdtype=gdtype)
            ref = adamw_ref64(p, g.float(), m, v, **h)
            got = adamw_restated_f32(p, g, m, v, **h)
            for k, a, b in zip("pmv", got, ref[:3]):
                worst[k] = max(worst[k], float(adamw_ratio(a, b, ref[3][k]).max()))
    print("worst |fp32 - fp64| / (2^-24 x operand scale):", {k: round(r, 4) for k, r in worst.items()})
    for k, r in worst.items():
        assert 0.95 * MEASURED[k] <= r <= MEASURED[k], (k, r, MEASURED[k])
        assert RATIO_BOUND[k] == 4.0 * MEASURED[k]


# ---- the module the fp32 ShardedAdamW tests run (CPU here, the GPU in tests/test_gpu_full_finetune.py) -------------------
class Awkward(torch.nn.Module):
    """Two buckets of awkward sizes. Views start on multiples of 8 elements, so 15 / 7 / 33 / 5 elements leave padding
    between them; 1-D parameters (no decay) sit between and behind 2-D ones (decay), so a bucket is several runs.
    head:    w [3, 5] | bias [7] | norm_weight [33] | W [64, 40]              = 2624 elements, no padding at the end
    layer 0: W [64, 40] | norm_weight [33] | bias [7] | w [3, 5] | gate [5]   = 2632 -> 2688: 56 padding elements behind"""

    def __init__(self, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=gen)
        P = torch.nn.Parameter
        self.w, self.bias, self.norm_weight, self.W = P(r(3, 5)), P(r(7) * 0.1), P(1 + 0.1 * r(33)), P(r(64, 40) * 0.05)
        blk = torch.nn.Module()
        blk.W, blk.norm_weight, blk.bias, blk.w, blk.gate = P(r(64, 40) * 0.05), P(1 + 0.1 * r(33)), P(r(7) * 0.1), P(r(3, 5)), P(r(5))
        self.layers = torch.nn.ModuleList([blk])


def backward_and_finish(opt, model, step):
    """A backward whose gradients are fixed Gaussians (sigma grows with the step), delivered the way training delivers them:
    autograd -> the buckets' post-accumulate hooks -> finish()."""
    gen = torch.Generator().manual_seed(1000 + step)
    loss = 0.0
    for p in model.parameters():
        c = (torch.randn(p.shape, generator=gen) * (0.05 + 0.1 * step)).to(p.device)
        loss = loss + (p.float() * c).sum()
    loss.backward()
    opt.buckets.finish()


def layout(B, bi):
    """(parameter, offset, numel, decays) of bucket `bi`, and the mask of its padding elements."""
    b = B.buckets[bi]
    pad = torch.ones(b["numel"], dtype=torch.bool)
    items = []
    for p, o in zip(b["params"], b["offsets"]):
        items.append((p, o, p.numel(), p.dim() > 1))
        pad[o:o + p.numel()] = False
    return items, pad


def decay_mask(B, bi):
    """Elements of bucket `bi` weight decay applies to: a 2-D parameter and the padding behind it (ShardedAdamW._runs)."""
    b = B.buckets[bi]
    mask = torch.zeros(b["numel"], dtype=torch.bool)
    ends = b["offsets"][1:] + [b["numel"]]
    for p, o, e in zip(b["params"], b["offsets"], ends):
        mask[o:e] = p.dim() > 1
    return mask


LR, WD, STEPS, LR_DROP_AT = 1e-3, 0.1, 6, 4                  # (the lr halves from step 4 on)
CAP = 4096                                                   # straddles: at most 1 element in CAP


def lr_at(step):
    return LR if step < LR_DROP_AT else 0.5 * LR


def restated_bucket_step(B, bi, state, g16, step):
    """The kernel's arithmetic (tests/_util.adamw_restated_f32) on bucket `bi` from `state` = fp32 (p, m, v), decay where
    decay_mask says; returns ({p, m, v} in fp32, the operand scales of the fp64 step from the same state)."""
    dec = decay_mask(B, bi).to(g16.device)
    h = dict(lr=lr_at(step), betas=(0.9, 0.999), eps=1e-8, step=step)
    with_wd = adamw_restated_f32(*state[:1], g16, *state[1:], weight_decay=WD, **h)
    without = adamw_restated_f32(*state[:1], g16, *state[1:], weight_decay=0.0, **h)
    s_wd = adamw_ref64(state[0], g16.float(), state[1], state[2], weight_decay=WD, **h)[3]
    s_no = adamw_ref64(state[0], g16.float(), state[1], state[2], weight_decay=0.0, **h)[3]
    want = dict(p=torch.where(dec, with_wd[0], without[0]), m=with_wd[1], v=with_wd[2])
    return want, dict(p=torch.where(dec, s_wd["p"], s_no["p"]), m=s_wd["m"], v=s_wd["v"])


def count_straddles(p16_a, p16_b, master_a, master_b, what):
    """Elements whose 16-bit parameters differ. Each must be a straddle: the two fp32 masters round to neighbouring 16-bit
    values. Returns their number (the caller caps it)."""
    diff = p16_a != p16_b
    n = int(diff.sum())
    if n:
        assert torch.equal(master_a.to(p16_a.dtype)[diff], p16_a[diff]) and torch.equal(master_b.to(p16_b.dtype)[diff], p16_b[diff])
        assert not torch.equal(master_a[diff], master_b[diff]), what
    print(f"{what}: {n} of {diff.numel()} parameters straddle a rounding boundary")
    return n


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_host_branch_against_the_restated_kernel_arithmetic(dtype):
    from tests.test_gpu_optim_kernels import RATIO_BOUND
    from unsloth_amd.full_finetune import ShardedAdamW
    model = Awkward().to(dtype)
    opt = ShardedAdamW(model, lr=LR, weight_decay=WD)
    B = opt.buckets
    assert [b["numel"] for b in B.buckets] == [2624, 2688]
    assert [len(r) for r in opt._runs] == [3, 4] and any(not d for r in opt._runs for _, _, d in r)
    for step in range(1, STEPS + 1):
        opt.param_groups[0]["lr"] = lr_at(step)
        backward_and_finish(opt, model, step)
        grads = [b["flat_g"].clone() for b in B.buckets]
        # every step is compared from the optimizer's OWN state before it: the bound is that of ONE step's rounding (two fp32
        # runs left alone drift apart by more -- an element that has shrunk carries the absolute errors of its larger past)
        before = [(opt.master[bi].clone(), opt.exp_avg[bi].clone(), opt.exp_avg_sq[bi].clone()) for bi in range(len(B.buckets))]
        opt.step()
        opt.zero_grad()
        straddles = 0
        for bi, b in enumerate(B.buckets):
            want, scale = restated_bucket_step(B, bi, before[bi], grads[bi], step)
            for k, got in (("p", opt.master[bi]), ("m", opt.exp_avg[bi]), ("v", opt.exp_avg_sq[bi])):
                assert_adamw_close(got, want[k].double(), scale[k], RATIO_BOUND[k], f"{dtype} step {step} bucket {bi} {k}")
            straddles += count_straddles(B.param_shard(bi), want["p"].to(dtype), opt.master[bi], want["p"],
                                         f"{dtype} step {step} bucket {bi}")
            assert torch.equal(B.param_shard(bi), opt.master[bi].to(dtype))
        total = sum(b["numel"] for b in B.buckets)
        assert straddles * CAP <= total, f"step {step}: {straddles} straddles in {total} elements"
    B.close()
