"""-m gpu: gradient clipping by global norm on the device (csrc/grad_norm.hip, the *_clip entry points of csrc/adamw.hip,
`max_grad_norm` of optim.FlatAdamW / full_finetune.ShardedAdamW / trainer.make_optimizer).

The norm is held to a DERIVED bound against fp64: every element is squared exactly and every sum is fp64, so the fp64 root is
within a few 2^-53 of the truth and the stored fp32 norm adds one rounding, 2^-24 relative; the check is 2^-22. Worst measured
over every case below: 5.53e-8 (2^-24.1)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PART, CAP = 8192, 1024                    # uamd_grad_sumsq: smallest part (elements), most parts
# the edges of the split and of the vector path: below / at / above one vector and one 1024-element sweep, one element either
# side of the size where a second part appears, parts that do not divide n, and a size past the cap on the number of parts
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, PART - 1, PART + 1, 3 * PART + 5, PART * CAP + PART + 5]
TINY = {torch.float32: 1e-21, torch.bfloat16: 1e-21, torch.float16: 1e-7}      # squares below 2^-126 (fp16 has no such value)


@pytest.mark.parametrize("content", ["normal", "zero", "spike", "tiny"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_norm_against_fp64(dtype, content):
    from unsloth_amd.optim import GradNorm
    base = torch.randn(SIZES[-1] + 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    if content == "zero":
        base.zero_()
    elif content == "spike":                   # one element of 1e3 among values of 1e-4: fp32 accumulation loses the small mass
        base.fill_(1e-4)
        base[1] = 1e3
    elif content == "tiny":
        base.mul_(TINY[dtype])
    base = base.to(dtype)
    gn = GradNorm(DEV, CAP)
    got, want = [], []
    for n in SIZES:
        for off in (0, 1):                     # off 1: 4 bytes past 16-byte alignment (fp32), 2 bytes past 8-byte alignment (16-bit)
            g = base[off:off + n]
            assert g.data_ptr() % 16 == off * g.element_size()
            got.append(gn.run([g], math.inf, 1)[0].double())
            want.append(g.double().square().sum().sqrt())
    got, want = torch.stack(got).cpu(), torch.stack(want).cpu()
    err = (got - want).abs()
    print(f"{dtype} {content}: worst |norm - ref| / ref = {float((err / want.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= 2.0 ** -22 * want).all()), (got, want)
    if content == "spike":                     # the small mass is there: 1e3 alone would give exactly 1000
        assert float(got[-1]) > 1000.0 + 1e-5


def test_same_bits_on_every_launch_and_graph_replay():
    from unsloth_amd.optim import GradNorm
    g = torch.randn(3 * PART + 6, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))[1:]
    gn = GradNorm(DEV, CAP)
    eager, graph = [], torch.cuda.CUDAGraph()
    for i in range(6):                         # two eager launches, the capture, three replays
        gn.partials.fill_(-1.0)
        gn.out.zero_()
        if i < 2:
            gn.run([g], 1.0, 0)
        elif i == 2:
            with torch.cuda.graph(graph):
                gn.run([g], 1.0, 0)
            continue
        else:
            graph.replay()
        eager.append((gn.out[0].clone(), gn.partials[:4].clone()))
    assert all(torch.equal(o.view(torch.int32), eager[0][0].view(torch.int32)) and
               torch.equal(q.view(torch.int64), eager[0][1].view(torch.int64)) for o, q in eager[1:]) and len(eager) == 5


@pytest.mark.parametrize("scale,max_norm", [(1e-3, 1.0), (1.0, 1.0), (0.0, 0.5), (math.inf, 2.0)],
                         ids=["below", "above", "zero", "inf"])
def test_factor_is_torchs_rule_on_the_stored_norm(scale, max_norm):
    from unsloth_amd.optim import GradNorm
    g = torch.randn(1025, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    g = g * scale if math.isfinite(scale) else g.index_fill(0, torch.tensor([7], device=DEV), math.inf)
    norm, coef = GradNorm(DEV, CAP).run([g], max_norm, 0).cpu()
    want = torch.tensor(min(1.0, max_norm / (float(norm) + 1e-6)), dtype=torch.float64).to(torch.float32)
    assert torch.equal(coef.view(torch.int32), want.view(torch.int32))
    assert (float(coef) == 1.0) == (scale <= 1e-3) and (float(coef) == 0.0) == (scale == math.inf)


@pytest.mark.parametrize("n", [5, 1025, 3 * 256 + 7])
@pytest.mark.parametrize("bits,gdtype", [(32, torch.float32), (8, torch.float32), (32, torch.bfloat16), (32, torch.float16),
                                         (8, torch.bfloat16), (8, torch.float16)])
def test_clip_step_equals_plain_step_with_the_host_factor(bits, gdtype, n):
    """uamd_adamw*_clip(grad_scale = 0.5, *coef_dev = c) leaves the bits of uamd_adamw*(grad_scale = 0.5 * c) -- the plain entry
    points are pinned to fp64 and torch in test_gpu_optim_kernels.py / test_gpu_optim8.py."""
    from unsloth_amd import _lib, optim
    gen = torch.Generator().manual_seed(n)
    flat = gdtype == torch.float32
    p = torch.randn(n, generator=gen).to(DEV)
    g = (torch.randn(n, generator=gen) * 3).to(DEV).to(gdtype)
    m, v = (torch.randn(n, generator=gen) * 0.1).to(DEV), (torch.rand(n, generator=gen) * 0.01).to(DEV)
    if bits == 8:
        cm, cv = optim.adam8_maps(DEV)
        (m, am), (v, av) = optim.adam8_encode(m, cm, True), optim.adam8_encode(v, cv, False)
    coef = torch.tensor([0.37], device=DEV)
    results = []
    for clip in (True, False):
        bufs = [p.clone(), g.clone()] + ([] if flat else [torch.zeros(n, dtype=gdtype, device=DEV)]) + [m.clone(), v.clone()] \
            + ([am.clone(), av.clone()] if bits == 8 else [])
        args = [b.data_ptr() for b in bufs] + ([cm.data_ptr(), cv.data_ptr()] if bits == 8 else []) + [n] \
            + ([2, n - 1] if bits == 8 and not flat else []) \
            + [1e-2, 0.9, 0.999, 1e-8, 0.1, 1 - 0.9 ** 3, math.sqrt(1 - 0.999 ** 3), 0.5 if clip else 0.5 * float(coef)] \
            + [1 if flat else _lib.dtype_code(gdtype)] + ([coef.data_ptr()] if clip else []) + [_lib.stream_of(p)]
        _lib.call("uamd_adamw" + ("8" if bits == 8 else "") + ("_flat" if flat else "_shard") + ("_clip" if clip else ""), p, *args)
        results.append(bufs)
    assert all(torch.equal(a, b) for a, b in zip(*results)) and not torch.equal(results[0][0], p)
    if flat:
        assert float(results[0][1].abs().max()) == 0.0          # zero_grad stays folded into the pass


@pytest.mark.parametrize("optim_name", [None, "adamw_8bit"])
def test_make_optimizer_max_grad_norm(optim_name, monkeypatch):
    from tests.test_gpu_optim import _Bag
    from unsloth_amd import _lib
    from unsloth_amd.trainer import make_optimizer
    shapes = [((16, 64), (64, 16)), ((8, 1000), (36, 8))]
    names, real = [], _lib.call                               # (the launches, recorded as tests/test_gpu_qwen3.py does)
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    bags = [_Bag(shapes, seed=3) for _ in range(3)]
    clipped, scaled, plain = (make_optimizer(b, lr=1e-2, optim=optim_name, max_grad_norm=mg)
                              for b, mg in zip(bags, (0.5, None, 0)))
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(q.shape, generator=gen).to(DEV) for q in bags[0].parameters()]
    total = math.sqrt(sum(float(x.double().square().sum()) for x in grads))
    for opt, bag in zip((clipped, scaled, plain), bags):
        for q, gr in zip(bag.parameters(), grads):
            q.grad.add_(gr * (2.0 / total))                        # norm 2.0: four times the limit
            opt.arena.ready(q)
    ref = float(clipped.arena.arena.double().square().sum().sqrt())
    kernel = "uamd_adamw8_flat" if optim_name else "uamd_adamw_flat"
    del names[:]
    clipped.step()
    assert names == ["uamd_grad_sumsq", "uamd_grad_clip_coef", kernel + "_clip"]
    norm = float(clipped.last_grad_norm)
    assert clipped.last_grad_norm.dim() == 0 and abs(norm - ref) <= 2.0 ** -22 * ref and abs(norm - 2.0) < 1e-5
    scaled.step(grad_scale=0.5 / (norm + 1e-6))
    assert torch.equal(clipped.flat_p, scaled.flat_p) and torch.equal(clipped.flat_m, scaled.flat_m)
    assert abs(float(clipped.grad_norm())) == 0.0 and abs(float(clipped.last_grad_norm) - norm) == 0.0
    # max_grad_norm None / 0: the launches and the bits of the plain entry point called directly
    state = [t.clone() for t in (plain.flat_p, plain.arena.arena, plain.flat_m, plain.flat_v)]
    del names[:]
    plain.step()
    assert names == [kernel] and plain.last_grad_norm is None
    hyper = (state[0].numel(), 1e-2, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9, math.sqrt(1 - 0.999), 1.0, 1, _lib.stream_of(state[0]))
    if optim_name:
        am, av = torch.zeros_like(plain.absmax_m), torch.zeros_like(plain.absmax_v)
        real(kernel, state[0], *(t.data_ptr() for t in state + [am, av, plain.code_m, plain.code_v]), *hyper)
    else:
        real(kernel, state[0], *(t.data_ptr() for t in state), *hyper)
    assert torch.equal(plain.flat_p, state[0]) and torch.equal(plain.flat_m, state[2]) and torch.equal(plain.flat_v, state[3])
    for opt in (clipped, scaled, plain):
        opt.close()


def test_sharded_adamw_one_rank_clips_like_a_host_grad_scale():
    from tests.test_full_finetune_gloo import Tiny, _loss
    from unsloth_amd.full_finetune import ShardedAdamW
    ids = torch.randint(0, 40, (2, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    models, opts = [], []
    for mg in (1e-2, None):
        torch.manual_seed(0)
        models.append(Tiny().to(torch.bfloat16).to(DEV))
        opts.append(ShardedAdamW(models[-1], lr=3e-2, weight_decay=0.1, max_grad_norm=mg))
        _loss(models[-1], ids).backward()
        opts[-1].buckets.finish()
    B = opts[0].buckets
    ref = math.sqrt(sum(float(B.grad_shard(bi).double().square().sum()) for bi in range(len(B.buckets))))
    opts[0].step()
    norm = float(opts[0].last_grad_norm)
    assert ref > 1e-2 and abs(norm - ref) <= 2.0 ** -22 * ref          # (above the limit: the step is really clipped)
    opts[1].step(grad_scale=1e-2 / (norm + 1e-6))
    assert all(torch.equal(p, q) for p, q in zip(models[0].parameters(), models[1].parameters()))
    for o in opts:
        o.buckets.close()
