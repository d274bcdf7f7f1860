"""-m gpu: the fp32 AdamW kernels of csrc/adamw.hip (uamd_adamw_flat, uamd_adamw_shard) through the C ABI, element by element
against the float64 reference tests/_util.adamw_ref64 (pinned to torch.optim.AdamW in tests/test_optim_ref_host.py).

Every buffer is carved out of one byte pool filled with a sentinel, 64 sentinel bytes in front of, between and behind the
buffers; each starts 16-byte aligned but not at the pool's base (g16 / p16 of the shard kernel also at 8 bytes past a 16-byte
boundary, their documented alignment). After every call the sentinel bytes must be unchanged.

Tolerance. Not chosen: measured. tests/_util.adamw_restated_f32 runs the step as separate fp32 torch operations in the
kernel's association with the scalars rounded as the entry points round them; over ALL inputs of this module (every size of
SIZES at BASE, every setting of SETTINGS x WDS x GRAD_SCALES at n = 1027, fp32 / bf16 / fp16 gradients) its worst
|fp32 - fp64| / (2^-24 x operand scale) is, on the CPU,

    p: 2.327        m: 2.379        v: 2.200

(tests/test_optim_ref_host.py::test_fp32_restatement_ratios_are_the_recorded_ones recomputes them and holds them to the
figures below). The GPU bound is 4 x that: RATIO_BOUND = p 9.308, m 9.516, v 8.800 units of 2^-24 x operand scale. The margin
covers a different but still correctly rounded sequence of division and square root, not a wrong formula: a swapped lane, a
skipped tail, decay on the wrong run or omb2 g instead of omb2 g^2 miss it by orders of magnitude.
"""
import math

import pytest
import torch

from tests._util import adamw_ref64, assert_adamw_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

MEASURED = dict(p=2.327, m=2.379, v=2.200)                   # the restatement's worst ratios (see the docstring)
RATIO_BOUND = {k: 4.0 * r for k, r in MEASURED.items()}

# tail only, one vector + every tail length; around one block of 256 x 4; past the grid cap (4096 blocks x 256 threads x 4)
# with a ragged second trip and a tail
BIG = 4194304 + 3 * 1024 + 3
SIZES = [1, 3, 4, 5, 7, 1023, 1024, 1027, BIG]
SETTINGS = [(1, (0.9, 0.999)), (2, (0.9, 0.999)), (1000, (0.9, 0.999)), (100000, (0.9, 0.999)), (3, (0.8, 0.95)),
            (5, (0.0, 0.5))]
WDS = [0.0, 0.1]
GRAD_SCALES = [1.0, 0.25, 0.0]
LR, EPS = 1e-2, 1e-8
BASE = dict(step=2, betas=(0.9, 0.999), weight_decay=0.1, grad_scale=0.25)
ERR_ARG, ERR_ALIGN = -2, -3
GUARD, FILL = 64, 0xA5


def hyper(step, betas, weight_decay, grad_scale, lr=LR):
    return dict(lr=lr, betas=betas, eps=EPS, weight_decay=weight_decay, step=step, grad_scale=grad_scale)


def make_inputs(n, seed=0, gdtype=torch.float32):
    """fp32 p, m, v and the gradient in `gdtype` (CPU). |g| log-uniform over 1e-6 .. 1e3 (g^2 and (1 - b2) g^2 stay normal
    fp32 numbers); v = s^2 with s within a factor 10 of |g|, |m| <= 0.9 s (moments some history of such gradients could have
    left); |p| over 1e-2 .. 3. From n = 7 on: a stretch with g = m = v = 0 at n // 4 and a stretch with g = 0 on non-zero
    moments at n // 2, each max(1, n // 16) long."""
    gen = torch.Generator().manual_seed(1234 + 7 * seed + n % 1000)
    u = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    sign = lambda: torch.where(u() < 0.5, -1.0, 1.0)
    g = sign() * 10.0 ** (u() * 9.0 - 6.0)
    s = g.abs() * 10.0 ** (u() * 2.0 - 1.0)
    m = (s * (u() * 1.8 - 0.9)).to(torch.float32)
    v = (s * s).to(torch.float32)
    p = (sign() * 10.0 ** (u() * 2.5 - 2.0)).to(torch.float32)
    g = g.to(torch.float32)
    if n >= 7:
        k = max(1, n // 16)
        g[n // 4:n // 4 + k] = 0
        m[n // 4:n // 4 + k] = 0
        v[n // 4:n // 4 + k] = 0
        g[n // 2:n // 2 + k] = 0
    return p, g.to(gdtype), m, v


def cases():
    """(n, hyper-parameters) of every launch the bounds are measured over: every size at BASE, every setting at 1027."""
    out = [(n, hyper(**BASE)) for n in SIZES]
    out += [(1027, hyper(t, betas, wd, gs)) for t, betas in SETTINGS for wd in WDS for gs in GRAD_SCALES]
    return out


# ---- the pool ------------------------------------------------------------------------------------------------------------
class Pool:
    """Buffers (name, CPU tensor, bytes past a 16-byte boundary) laid out in one device byte pool between sentinel bytes."""

    def __init__(self, *bufs):
        self.where, cur = {}, 0
        for name, t, mis in bufs:
            cur = (cur + GUARD + 15) // 16 * 16 + mis
            self.where[name] = (cur, t.numel() * t.element_size(), t.dtype)
            cur += t.numel() * t.element_size()
        self.bytes = torch.full(((cur + 15) // 16 * 16 + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        assert self.bytes.data_ptr() % 16 == 0
        for name, t, mis in bufs:
            self[name].copy_(t.to(DEV))
            assert self.ptr(name) % 16 == mis and self.ptr(name) != self.bytes.data_ptr()

    def __getitem__(self, name):
        start, nbytes, dtype = self.where[name]
        return self.bytes[start:start + nbytes].view(dtype)

    def ptr(self, name, first=0):
        start, _, dtype = self.where[name]
        return self.bytes.data_ptr() + start + first * torch.empty((), dtype=dtype).element_size()

    def check_sentinels(self, what=""):
        cur = 0
        for name, (start, nbytes, _) in self.where.items():
            assert bool((self.bytes[cur:start] == FILL).all()), f"{what}: bytes in front of `{name}` were written"
            cur = start + nbytes
        assert bool((self.bytes[cur:] == FILL).all()), f"{what}: bytes behind the last buffer were written"


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def flat_pool(p, g, m, v):
    return Pool(("p", p, 0), ("g", g, 0), ("m", m, 0), ("v", v, 0))


def shard_pool(p, g16, m, v, mis=0):
    return Pool(("p", p, 0), ("g16", g16, mis), ("p16", torch.zeros_like(g16), mis), ("m", m, 0), ("v", v, 0))


def _scalars(h):
    b1, b2 = h["betas"]
    return (float(h["lr"]), float(b1), float(b2), float(h["eps"]), float(h["weight_decay"]), 1.0 - b1 ** h["step"],
            math.sqrt(1.0 - b2 ** h["step"]), float(h["grad_scale"]))


def launch_flat(pool, h, zero_grad, first=0, n=None):
    """uamd_adamw_flat over elements [first, first + n) of the pool's buffers; returns the C return code."""
    from unsloth_amd import _lib
    n = pool["p"].numel() - first if n is None else n
    return _lib.lib().uamd_adamw_flat(pool.ptr("p", first), pool.ptr("g", first), pool.ptr("m", first), pool.ptr("v", first),
                                      n, *_scalars(h), int(zero_grad), _lib.stream_of(pool.bytes))


def launch_shard(pool, h, first=0, n=None):
    from unsloth_amd import _lib
    n = pool["p"].numel() - first if n is None else n
    return _lib.lib().uamd_adamw_shard(pool.ptr("p", first), pool.ptr("g16", first), pool.ptr("p16", first),
                                       pool.ptr("m", first), pool.ptr("v", first), n, *_scalars(h),
                                       _lib.dtype_code(pool["g16"].dtype), _lib.stream_of(pool.bytes))


def check_against_ref(pool, inputs, h, what):
    """p, m, v of the pool within RATIO_BOUND of the fp64 step on `inputs` = (p, g, m, v) before the call (CPU)."""
    p, g, m, v = (x.to(DEV) for x in inputs)
    rp, rm, rv, scale = adamw_ref64(p, g.float(), m, v, **h)
    worst = {}
    for k, got, want in (("p", pool["p"], rp), ("m", pool["m"], rm), ("v", pool["v"], rv)):
        worst[k] = assert_adamw_close(got, want, scale[k], RATIO_BOUND[k], f"{what} {k}")
    print(f"{what}: worst ratios " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))
    zero = (inputs[1].float() == 0) & (inputs[2] == 0) & (inputs[3] == 0)
    if bool(zero.any()):                    # g = m = v = 0: the update is exactly 0 (decay alone moves p), nothing is NaN
        z = zero.to(DEV)
        lr_wd = torch.tensor(h["lr"] * h["weight_decay"], dtype=torch.float64).to(torch.float32).to(DEV)
        assert torch.equal(pool["p"][z], p[z] - lr_wd * p[z]), f"{what}: a zero gradient on zero moments moved p"
        assert float(pool["m"][z].abs().max()) == 0.0 and float(pool["v"][z].abs().max()) == 0.0


# ---- uamd_adamw_flat -------------------------------------------------------------------------------------------------------
def _flat_case(n, h):
    inputs = make_inputs(n)
    what = f"flat n={n} t={h['step']} betas={h['betas']} wd={h['weight_decay']} gs={h['grad_scale']}"
    pool = flat_pool(*inputs)
    assert launch_flat(pool, h, zero_grad=1) == 0
    check_against_ref(pool, inputs, h, what)
    assert bool((bits(pool["g"]) == 0).all()), f"{what}: zero_grad = 1 left a gradient element that is not +0.0"
    pool.check_sentinels(what)
    keep = flat_pool(*inputs)
    assert launch_flat(keep, h, zero_grad=0) == 0
    assert same_bits(keep["g"], inputs[1].to(DEV)), f"{what}: zero_grad = 0 changed the gradient"
    for k in "pmv":
        assert same_bits(keep[k], pool[k]), f"{what}: {k} depends on zero_grad"
    keep.check_sentinels(what + " zero_grad=0")


@pytest.mark.parametrize("n", SIZES)
def test_flat_every_size(n):
    _flat_case(n, hyper(**BASE))


@pytest.mark.parametrize("t,betas", SETTINGS)
def test_flat_every_setting(t, betas):
    for wd in WDS:
        for gs in GRAD_SCALES:
            _flat_case(1027, hyper(t, betas, wd, gs))


# ---- uamd_adamw_shard ------------------------------------------------------------------------------------------------------
def _shard_case(n, h, dtype):
    inputs = make_inputs(n, gdtype=dtype)
    first = None
    for mis in (0, 8):
        what = f"shard {dtype} n={n} +{mis}B t={h['step']} betas={h['betas']} wd={h['weight_decay']} gs={h['grad_scale']}"
        pool = shard_pool(*inputs, mis=mis)
        assert launch_shard(pool, h) == 0
        check_against_ref(pool, inputs, h, what)
        assert same_bits(pool["p16"], pool["p"].to(dtype)), f"{what}: p16 is not its own master rounded once"
        assert same_bits(pool["g16"], inputs[1].to(DEV)), f"{what}: the gradient was written"
        pool.check_sentinels(what)
        if first is not None:
            for k in ("p", "m", "v", "p16"):
                assert same_bits(pool[k], first[k]), f"{what}: {k} depends on the alignment of g16 / p16"
        first = pool


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", SIZES)
def test_shard_every_size(n, dtype):
    _shard_case(n, hyper(**BASE), dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("t,betas", SETTINGS)
def test_shard_every_setting(t, betas, dtype):
    for wd in WDS:
        for gs in GRAD_SCALES:
            _shard_case(1027, hyper(t, betas, wd, gs), dtype)


def rounding_probes(dtype):
    """fp32 bit patterns around the rounding points of `dtype`: exact ties (the kept mantissa even -> down, odd -> up), one
    fp32 ulp either side of each, both signs; for fp16 also magnitudes that are fp16 subnormals (ties at odd multiples of
    2^-25, their neighbours, and values below the smallest subnormal's half); +0 and -0."""
    drop = 16 if dtype == torch.bfloat16 else 13                    # mantissa bits the conversion drops
    half = 1 << (drop - 1)
    gen = torch.Generator().manual_seed(5)
    lo_e, hi_e = (64, 190) if dtype == torch.bfloat16 else (127 - 14, 127 + 14)         # biased fp32 exponents: normal results
    out = []
    for odd in (0, 1):
        e = torch.randint(lo_e, hi_e + 1, (64,), generator=gen, dtype=torch.int64)
        kept = torch.randint(0, 1 << (23 - drop), (64,), generator=gen, dtype=torch.int64) // 2 * 2 + odd
        base = (e << 23) | (kept << drop)
        for low in (half, half - 1, half + 1, 0, 1, (1 << drop) - 1):
            out.append(base | low)
    mag = torch.cat(out)
    if dtype == torch.float16:
        k = torch.arange(0, 1024, dtype=torch.float64)
        tie = ((k + 0.5) * 2.0 ** -24).to(torch.float32).view(torch.int32).to(torch.int64)      # exact in fp32
        tiny = torch.tensor([2.0 ** -25, 2.0 ** -26, 2.0 ** -30], dtype=torch.float32).view(torch.int32).to(torch.int64)
        mag = torch.cat([mag, tie, tie - 1, tie + 1, tiny, tiny + 1, tiny[:2] - 1])
    allbits = torch.cat([mag, mag | (1 << 31), torch.tensor([0, 1 << 31])])
    allbits = torch.where(allbits >= 1 << 31, allbits - (1 << 32), allbits).to(torch.int32)
    return allbits.view(torch.float32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_shard_rounds_the_master_exactly(dtype):
    """lr = 0, wd = 0: the master does not move (p - 0 p, p - 0 m / denom), so p16 is from_f32<T> of a chosen fp32 pattern."""
    p = rounding_probes(dtype)
    n = p.numel()
    assert n % 4 == 2                                               # the last two probes (+0, -0) run in the scalar tail
    _, g, m, v = make_inputs(n, seed=1, gdtype=dtype)
    want16 = p.to(dtype)                                            # torch on the CPU: round to nearest even, subnormals kept
    assert bool(torch.isfinite(want16.float()).all())
    if dtype == torch.float16:
        sub = (want16.float().abs() < 2.0 ** -14) & (want16.float() != 0)
        assert int(sub.sum()) > 1000
    for order in (0, 1):                                            # reversed: every probe kind also meets the other lanes
        q = p.flip(0) if order else p
        pool = shard_pool(q, g, m, v)
        assert launch_shard(pool, hyper(3, (0.9, 0.999), 0.0, 1.0, lr=0.0)) == 0
        assert same_bits(pool["p"], q.to(DEV)), "the master moved (or lost the sign of a zero) under lr = 0"
        got, want = pool["p16"].cpu(), (want16.flip(0) if order else want16)
        bad = bits(got) != bits(want)
        assert not bool(bad.any()), (f"{int(bad.sum())} of {n} roundings differ; first: fp32 {q[bad][0].item()!r} -> "
                                     f"{got[bad][0].item()!r}, want {want[bad][0].item()!r}")
        pool.check_sentinels()


# ---- properties both kernels share -------------------------------------------------------------------------------------------
KERNELS = ["flat", "bf16", "fp16"]


def _pool_and_launch(kind, n, seed=0, nan_at=()):
    dtype = dict(flat=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)[kind]
    inputs = list(make_inputs(n, seed=seed, gdtype=dtype))
    for i in nan_at:
        inputs[1][i] = float("nan")
    if kind == "flat":
        return flat_pool(*inputs), (lambda pool, h, **kw: launch_flat(pool, h, 1, **kw)), ("p", "m", "v", "g")
    return shard_pool(*inputs), launch_shard, ("p", "m", "v", "p16", "g16")


@pytest.mark.parametrize("kind", KERNELS)
def test_partition_independence(kind):
    """One launch over [0, n) = launches over [0, k) and [k, n), bit for bit: how FlatAdamW._runs() (k a multiple of 4) and
    ShardedAdamW._runs (k a multiple of 8) call the kernels."""
    n, h = 1027, hyper(**BASE)
    whole, launch, names = _pool_and_launch(kind, n)
    assert launch(whole, h) == 0
    for k in (8, 520, 1024):
        parts, _, _ = _pool_and_launch(kind, n)
        assert launch(parts, h, first=0, n=k) == 0
        untouched, _, _ = _pool_and_launch(kind, n)
        for name in names:                                          # the first launch stops at k
            assert same_bits(parts[name][k:], untouched[name][k:]), f"{kind} k={k}: {name} written past the run"
        assert launch(parts, h, first=k, n=n - k) == 0
        for name in names:
            assert same_bits(parts[name], whole[name]), f"{kind} k={k}: {name} differs between one launch and two"
        parts.check_sentinels()


@pytest.mark.parametrize("kind", KERNELS)
def test_lane_independence(kind):
    """A NaN gradient in a vector lane (element 6: lane z of the second float4) and one in the scalar tail (element 1025 of
    1027) make exactly those elements of p, m, v NaN; every other element is bit-equal to the run without them."""
    n, h, at = 1027, hyper(**BASE), (6, 1025)
    clean, launch, names = _pool_and_launch(kind, n)
    dirty, _, _ = _pool_and_launch(kind, n, nan_at=at)
    assert launch(clean, h) == 0 and launch(dirty, h) == 0
    hit = torch.zeros(n, dtype=torch.bool, device=DEV)
    hit[list(at)] = True
    for name in names:
        if name in ("g", "g16"):
            continue
        assert bool(torch.isnan(dirty[name][hit].float()).all()), f"{kind}: {name} at the NaN gradients is not NaN"
        assert same_bits(dirty[name][~hit], clean[name][~hit]), f"{kind}: a NaN gradient reached a neighbour in {name}"
    dirty.check_sentinels()


@pytest.mark.parametrize("kind", KERNELS)
def test_argument_contract_writes_nothing(kind):
    """n = 0 is OK; a bias correction that is not positive is an argument error; a pointer off its documented alignment
    (16 bytes; 8 for g16 / p16) is an alignment error -- and none of them writes a byte. All pointers stay inside the pool."""
    from unsloth_amd import _lib
    n, h = 40, hyper(**BASE)
    pool, launch, names = _pool_and_launch(kind, n)
    before = pool.bytes.clone()
    L, st = _lib.lib(), _lib.stream_of(pool.bytes)
    sc = list(_scalars(h))
    ptrs = [pool.ptr(k) for k in (("p", "g", "m", "v") if kind == "flat" else ("p", "g16", "p16", "m", "v"))]
    tail = (1, st) if kind == "flat" else (_lib.dtype_code(pool["g16"].dtype), st)
    fn = L.uamd_adamw_flat if kind == "flat" else L.uamd_adamw_shard
    assert fn(*ptrs, 0, *sc, *tail) == 0
    for i, bad in ((5, 0.0), (5, -0.5), (5, float("nan")), (6, 0.0), (6, -1.0), (6, float("nan"))):
        s = list(sc)
        s[i] = bad                                                  # 5: bias_correction1, 6: bias_correction2_sqrt
        assert fn(*ptrs, n - 8, *s, *tail) == ERR_ARG, (i, bad)
    assert fn(*ptrs, -1, *sc, *tail) == ERR_ARG
    for i in range(len(ptrs)):
        half16 = kind != "flat" and i in (1, 2)
        for off in ((4, 2) if half16 else (8, 4)):                  # still a multiple of the element size
            q = list(ptrs)
            q[i] += off
            assert fn(*q, n - 8, *sc, *tail) == ERR_ALIGN, (i, off)
    torch.cuda.synchronize()
    assert torch.equal(pool.bytes, before)
