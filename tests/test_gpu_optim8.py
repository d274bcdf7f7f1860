"""-m gpu: the 8-bit AdamW kernels (csrc/adamw.hip uamd_adamw8_flat / uamd_adamw8_shard) through FlatAdamW(optim_bits=8),
ShardedAdamW(optim_bits=8) and make_optimizer(optim="adamw_8bit"), against the restatement of the block-wise rule in
tests/test_optim8_host.py (run on the device: separate fp32 torch ops, no fused multiply-add -- like the library, which is
built with -ffp-contract=off).

Code-mismatch condition (check_codes): at most 1 code in 4096 differs from the restatement, each by exactly one step of the
sorted map -- only exact ties and last-ulp differences in m / absmax can move a code. Parameters / masters are compared
within rtol=1e-5, atol=1e-6 (tests/test_gpu_optim.py's bounds for the same adamw_one arithmetic): the parameter update uses
the fp32 moments BEFORE they are rounded, so a moved code does not show in the same step's parameters."""
import copy

import pytest
import torch

from tests.test_optim8_host import QB, Tiny, _grads, check_codes, restated_step, zero_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _bag(shapes, seed=0):
    from tests.test_gpu_optim import _Bag
    return _Bag(shapes, seed=seed)


def _feed(opt, model, grads):
    """Gradients are ADDED into the (zeroed) arena, like uamd_lora_tn does."""
    for p, gr in zip(model.parameters(), grads):
        p.grad.add_(gr)
        opt.arena.ready(p)


def _gauss(model, seed, sigma=0.1):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(p.shape, generator=gen) * sigma).to(DEV) for p in model.parameters()]


def _flat(tensors):
    return torch.cat([t.reshape(-1) for t in tensors])


def _set_state(opt, p, m8, v8, am, av):
    opt.flat_p.copy_(p)
    opt.flat_m.copy_(m8)
    opt.flat_v.copy_(v8)
    opt.absmax_m.copy_(am)
    opt.absmax_v.copy_(av)


# 64: less than one block; 256: exactly one; 1024 + 8: a full workgroup and a partial tail block; 5.12 M: past the grid cap
# (4096 workgroups x 4 blocks x 256 = 4.19 M elements), so the grid-stride loop runs
@pytest.mark.parametrize("shapes,zero_block", [
    ([((4, 8), (8, 4))], None),
    ([((8, 16), (16, 8))], None),
    ([((8, 64), (65, 8))], None),
    ([((8, 64), (65, 8))], 1),
    ([((16, 160000), (160000, 16))], None),
], ids=["n64", "n256", "n1032", "n1032-zero-block", "n5M"])
def test_adamw8_flat_one_step_exactness(shapes, zero_block):
    from unsloth_amd.optim import FlatAdamW
    lr, wd = 1e-2, 0.1
    model = _bag(shapes)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.1)
    opt = FlatAdamW(model, lr=lr, weight_decay=wd, optim_bits=8)
    n = opt.flat_p.numel()
    assert n == sum(a[0] * a[1] + b[0] * b[1] for a, b in shapes)
    state = (opt.flat_p.clone(),) + zero_state(n, DEV)
    for step in range(1, 7):
        grads = _gauss(model, 50 + step)
        g = _flat(grads)
        if zero_block is not None:
            g[zero_block * QB:(zero_block + 1) * QB] = 0
            grads, o = [], 0
            for p in model.parameters():
                grads.append(g[o:o + p.numel()].view(p.shape))
                o += p.numel()
        _set_state(opt, *state)                    # the state is carried by the restatement: flips cannot compound
        _feed(opt, model, grads)
        opt.step()
        opt.zero_grad()
        assert float(opt.arena.arena.abs().max()) == 0.0                      # zeroed by the step's own pass
        state = restated_step(state[0], g, *state[1:], step, lr, wd)
        if step in (1, 2, 6):
            p, m8, v8, am, av = state
            assert bool(torch.isfinite(opt.flat_p).all())
            torch.testing.assert_close(opt.flat_p, p, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(opt.absmax_m, am, rtol=1e-6, atol=0)
            torch.testing.assert_close(opt.absmax_v, av, rtol=1e-6, atol=0)
            check_codes(opt.flat_m, m8, f"step {step} state1")
            check_codes(opt.flat_v, v8, f"step {step} state2")
            if zero_block is not None:
                blk = slice(zero_block * QB, (zero_block + 1) * QB)
                assert float(opt.absmax_m[zero_block]) == 0.0 and float(opt.absmax_v[zero_block]) == 0.0
                assert bool((opt.flat_m[blk] == 127).all()) and bool((opt.flat_v[blk] == 0).all())
                for k in (0, 1):                                               # decodes to exactly 0, no NaN
                    assert float(_flat([opt.moments(q)[k] for q in model.parameters()])[blk].abs().max()) == 0.0
    for q in model.parameters():
        st = opt.state[q]
        assert st["state1"].dtype == torch.uint8 and st["state1"].shape == q.shape and int(st["step"]) == 6
        m, v = opt.moments(q)
        assert m.shape == q.shape and v.shape == q.shape and m.dtype == torch.float32 and float(v.min()) >= 0.0


def test_adamw8_flat_grad_scale_equals_prescaled_gradients():
    from unsloth_amd.optim import FlatAdamW
    shapes = [((8, 64), (65, 8))]
    a, b = _bag(shapes, seed=3), _bag(shapes, seed=3)
    oa, ob = FlatAdamW(a, lr=1e-2, optim_bits=8), FlatAdamW(b, lr=1e-2, optim_bits=8)
    c = torch.tensor(0.37, dtype=torch.float32, device=DEV)
    for step in range(3):
        grads = _gauss(a, 9 + step)
        _feed(oa, a, grads)
        _feed(ob, b, [gr * c for gr in grads])
        oa.step(grad_scale=0.37)
        ob.step()
        oa.zero_grad()
        ob.zero_grad()
    assert torch.equal(oa.flat_p, ob.flat_p)
    assert torch.equal(oa.flat_m, ob.flat_m) and torch.equal(oa.flat_v, ob.flat_v)
    assert torch.equal(oa.absmax_m, ob.absmax_m) and torch.equal(oa.absmax_v, ob.absmax_v)


def test_adamw8_flat_state_dict_resumes_bit_identically_and_refuses_the_other_width():
    from unsloth_amd.optim import FlatAdamW
    shapes = [((8, 64), (65, 8)), ((4, 4), (36, 8))]

    def run(opt, model, steps):
        for s in steps:
            _feed(opt, model, _gauss(model, 100 + s))
            opt.step()
            opt.zero_grad()

    a = _bag(shapes, seed=1)
    oa = FlatAdamW(a, lr=1e-2, optim_bits=8)
    run(oa, a, (1, 2))
    saved = oa.state_dict()                              # a snapshot: codes and scales are copies
    params = [p.detach().clone() for p in a.parameters()]
    assert saved["uamd_flat8"]["blocksize"] == QB
    run(oa, a, (3, 4))
    b = _bag(shapes, seed=1)
    ob = FlatAdamW(b, lr=1e-2, optim_bits=8)
    run(ob, b, (7, 8))
    with torch.no_grad():
        for p, q in zip(b.parameters(), params):
            p.copy_(q)
    ob.load_state_dict(saved)
    assert int(ob.state[next(b.parameters())]["step"]) == 2
    run(ob, b, (3, 4))
    assert torch.equal(oa.flat_p, ob.flat_p)
    assert torch.equal(oa.flat_m, ob.flat_m) and torch.equal(oa.flat_v, ob.flat_v)
    assert torch.equal(oa.absmax_m, ob.absmax_m) and torch.equal(oa.absmax_v, ob.absmax_v)
    c = _bag(shapes, seed=1)
    oc = FlatAdamW(c, lr=1e-2)
    with pytest.raises(ValueError, match="optim_bits=8.*optim_bits=32"):
        oc.load_state_dict(saved)
    with pytest.raises(ValueError, match="optim_bits=32.*optim_bits=8"):
        oa.load_state_dict(oc.state_dict())


def test_adamw8_flat_missing_gradient_steps_whole_blocks():
    """Where the 8-bit path differs from torch's skip: runs are widened to quant-block boundaries, so a parameter without a
    gradient that shares a block with one that has a gradient is stepped with a zero gradient (decay only, on its first
    step); a parameter whose blocks hold no gradient at all stays untouched."""
    from unsloth_amd.optim import FlatAdamW
    # elements: A0 [0, 128)  B0 [128, 256)  A1 [256, 768)  B1 [768, 1280): B0 shares block 0 with A0, B1 owns blocks 3, 4
    model = _bag([((8, 16), (16, 8)), ((8, 64), (64, 8))], seed=2)
    lr, wd = 1e-2, 0.1
    opt = FlatAdamW(model, lr=lr, weight_decay=wd, optim_bits=8)
    a0, b0, a1, b1 = list(model.parameters())
    before = [p.detach().clone() for p in (a0, b0, a1, b1)]
    for p, gr in zip((a0, a1), _gauss(model, 4)[::2]):
        p.grad.add_(gr)
        opt.arena.ready(p)
    b0.grad = None
    b1.grad = None
    assert opt._runs() == [[0, 768]]
    opt.step()
    assert not torch.equal(a0.data, before[0]) and not torch.equal(a1.data, before[2])
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)
    assert torch.equal(b0.data, before[1] - f32(lr * wd) * before[1])         # zero gradient, zero moments: decay alone
    assert torch.equal(b1.data, before[3])
    assert float(opt.absmax_m[3:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_adamw8_shard_matches_the_host_branch(dtype):
    """uamd_adamw8_shard against ShardedAdamW(optim_bits=8) on a CPU copy (the host branch, pinned to the restatement by
    tests/test_optim8_host.py), one rank, 4 steps. The head bucket's decay boundary (after the final norm's 72 elements) and
    the layer buckets' (5184 = 20.25 blocks) fall inside quant blocks. 16-bit parameters equal bit for bit and masters
    within the bounds, except at elements where a code has legitimately differed (the mismatch condition) in this or an
    earlier step: from there on that element's moment, hence its parameter, differs by up to one step of the map."""
    from unsloth_amd.full_finetune import ShardedAdamW
    from unsloth_amd.trainer import make_optimizer
    lr, wd = 1e-3, 0.1
    host = Tiny(hidden=72, vocab=200).to(dtype)
    dev = copy.deepcopy(host).to(DEV)
    dev._unsloth_full_finetuning = True
    og = make_optimizer(dev, lr=lr, weight_decay=wd, optim="adamw_8bit")
    assert isinstance(og, ShardedAdamW) and og.optim_bits == 8 and og.exp_avg[0].dtype == torch.uint8
    oh = ShardedAdamW(host, lr=lr, weight_decay=wd, optim_bits=8)
    nb = len(oh.buckets.buckets)
    assert any(b["shard"] > 4 * QB and b["shard"] % QB for b in oh.buckets.buckets)
    assert any(0 < d0 % QB or 0 < d1 % QB for d0, d1 in og._decay)
    moved = [torch.zeros(b["shard"], dtype=torch.bool) for b in oh.buckets.buckets]
    for step in range(1, 5):
        _grads(oh, step)
        for bh, bg in zip(oh.buckets.buckets, og.buckets.buckets):
            bg["flat_g"].copy_(bh["flat_g"])
        oh.step()
        og.step()
        for bi in range(nb):
            moved[bi] |= check_codes(og.exp_avg[bi].cpu(), oh.exp_avg[bi], f"step {step} bucket {bi} state1")
            moved[bi] |= check_codes(og.exp_avg_sq[bi].cpu(), oh.exp_avg_sq[bi], f"step {step} bucket {bi} state2")
            keep = ~moved[bi]
            torch.testing.assert_close(og.absmax_m[bi].cpu(), oh.absmax_m[bi], rtol=1e-6, atol=0)
            torch.testing.assert_close(og.absmax_v[bi].cpu(), oh.absmax_v[bi], rtol=1e-6, atol=0)
            torch.testing.assert_close(og.master[bi].cpu()[keep], oh.master[bi][keep], rtol=1e-5, atol=1e-6)
            p16g, p16h = og.buckets.param_shard(bi).cpu(), oh.buckets.param_shard(bi)
            assert torch.equal(p16g[keep], p16h[keep]), f"step {step} bucket {bi}"
            assert torch.equal(p16g, og.master[bi].cpu().to(dtype))                 # rounded once from its own master
    og.buckets.close()
    oh.buckets.close()


def test_adamw8_tracks_fp32_adamw():
    """20 steps at lr = 1e-2 on 65 536 elements: the 8-bit optimizer stays as close to FlatAdamW(optim_bits=32) as the rule
    itself does. The bound is computed here: twice the largest deviation of the restatement from the fp32 optimizer on the
    same inputs (the factor 2 covers tie flips; a wrong map or scale misses it by orders of magnitude)."""
    from unsloth_amd.optim import FlatAdamW
    shapes = [((16, 1024), (3072, 16))]
    lr, wd = 1e-2, 0.01
    m32, m8 = _bag(shapes, seed=7), _bag(shapes, seed=7)
    o32, o8 = FlatAdamW(m32, lr=lr, weight_decay=wd), FlatAdamW(m8, lr=lr, weight_decay=wd, optim_bits=8)
    n = o8.flat_p.numel()
    assert n == 65536
    start = o8.flat_p.clone()
    state = (start.clone(),) + zero_state(n, DEV)
    for step in range(1, 21):
        grads = _gauss(m32, 200 + step)
        _feed(o32, m32, grads)
        _feed(o8, m8, grads)
        o32.step()
        o8.step()
        o32.zero_grad()
        o8.zero_grad()
        state = restated_step(state[0], _flat(grads), *state[1:], step, lr, wd)
    rule = (state[0] - o32.flat_p).abs()
    got = (o8.flat_p - o32.flat_p).abs()
    travel = float((o32.flat_p - start).abs().mean())
    print(f"restatement vs fp32: max {float(rule.max()):.3e} mean {float(rule.mean()):.3e}; kernel vs fp32: max "
          f"{float(got.max()):.3e} mean {float(got.mean()):.3e}; mean travel {travel:.3e}")
    assert float(rule.max()) > 0.0
    assert float(got.max()) <= 2.0 * float(rule.max())


def test_training_with_adamw_8bit_end_to_end():
    """The tiny QLoRA model through unsloth_train with make_optimizer(model, optim="adamw_8bit")."""
    from tests.test_gpu_model import _batch, _tiny
    from unsloth_amd.optim import FlatAdamW
    from unsloth_amd.trainer import make_optimizer, unsloth_train
    ids, labels, pos = _batch(B=2, T=64, seed=4)
    batch = dict(input_ids=ids.to(DEV), labels=labels.to(DEV), position_ids=pos.to(DEV))
    model = _tiny(r=16, gc=False, head_dim=128)
    opt = make_optimizer(model, lr=2e-3, optim="adamw_8bit")
    assert isinstance(opt, FlatAdamW) and opt.optim_bits == 8
    losses = [float(x) for x in unsloth_train(model, [batch] * 8, optimizer=opt, max_steps=8)]
    print("adamw_8bit losses:", losses)
    assert len(losses) == 8 and losses[-1] < losses[0] - 0.5                       # it learns
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert opt.moment_bytes() == 2 * n + 8 * ((n + QB - 1) // QB)
    for p in (q for q in model.parameters() if q.requires_grad):
        m, v = opt.moments(p)
        assert m.shape == p.shape and v.shape == p.shape and bool(torch.isfinite(m).all()) and float(v.min()) >= 0.0
        assert opt.state[p]["state1"].dtype == torch.uint8 and opt.state[p]["state2"].shape == p.shape
    assert float(opt.absmax_v.max()) > 0.0
    opt.close()
