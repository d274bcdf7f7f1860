"""-m gpu: uamd_gemv_rows64 (csrc/decode.hip, kernels/decode.py gemv_rows64 / linear_group_rows) -- the rows GEMV for 17 .. 64
token rows on one pass over the weights: against the exact fp64 product of the code values, bit for bit against
uamd_gemv_rows on 16-row slices and on single rows, strided views with sentinels around them, non-finite rows among finite
ones, and the argument errors. The construction is tests/test_gpu_gemv_rows.py's, with 64 token rows."""
import pytest
import torch

from oracle import ref_ops as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (17, 31, 32, 33, 48, 63, 64)
# (Ns, K, lora) and the (RT, MT) instances the launcher picks on a 256-CU device (launch_gemv_rows_mt in csrc/decode.hip, the
# measurement behind it in DESIGN 9c). MT = 2 for M <= 32, else 4. With `tiles` the 16-row weight tiles of a launch: MT = 2
# takes RT = 2 from 1024 tiles and RT = 4 (NF4 only) from 2048; MT = 4 takes RT = 2 from 384 and RT = 4 (NF4 only) from 768.
# Together the shapes reach every instance: NF4 (1 | 2 | 4, 2 | 4), dense (1 | 2, 2 | 4).
NF4_SHAPES = [
    ((256,), 256, False),                        # 16 tiles: (1, 2), (1, 4)
    ((40,), 2080, True),                         # 3 tiles, ragged N, K ends inside a chunk: (1, 2), (1, 4)
    ((4096, 1024, 1024), 4096, True),            # 384 tiles, three groups, bias on the first: (1, 2), (2, 4)
    ((16392,), 256, False),                      # 1025 tiles, ragged last tile: (2, 2), (4, 4)
    ((32776,), 256, True),                       # 2049 tiles, ragged last tile: (4, 2), (4, 4)
]
DENSE_SHAPES = [(1000, 4096), (16392, 1024)]     # 63 tiles: (1, 2), (1, 4); 1025 tiles, ragged last tile: (2, 2), (2, 4)
_CACHE = {}


def g(seed):
    return torch.Generator().manual_seed(seed)


def _case(dtype, nested, Ns, K, lora):
    """The projections of one shape and the fp64 truth for 64 token rows, built once and shared by every M."""
    key = (dtype, nested, Ns, K, lora)
    if key in _CACHE:
        return _CACHE[key]
    from unsloth_amd.nf4 import quantize_nf4
    x = torch.randn(64, K, generator=g(1)).to(dtype)
    xd = x.to(DEV).double()
    projs, wants = [], []
    for i, N in enumerate(Ns):
        W = (torch.randn(N, K, generator=g(10 + i)) * 0.05).to(dtype)
        packed, qs = quantize_nf4(W.to(DEV), compress_statistics=nested)
        qs.dtype = dtype
        W32 = R.nf4_fp32_weight(packed, qs)                       # exact fp32 value of every code
        want = xd @ W32.to(DEV).double().t()
        A = B = s = None
        if lora:
            A = torch.randn(16, K, generator=g(20 + i)) * 0.05
            B = torch.randn(N, 16, generator=g(30 + i)) * 0.05
            s = 2.0
            want = want + s * ((xd @ A.to(dtype).to(DEV).double().t()) @ B.to(DEV).double().t())
        bias = (torch.randn(N, generator=g(40 + i)) * 0.1).to(dtype) if i == 0 else None
        if bias is not None:
            want = want + bias.to(DEV).double()
        projs.append((packed, qs, None if A is None else torch.nn.Parameter(A.to(DEV)),
                      None if B is None else torch.nn.Parameter(B.to(DEV)), s, None if bias is None else bias.to(DEV)))
        wants.append(want.cpu())
    _CACHE.clear()                                                 # one shape's weights at a time on the device
    _CACHE[key] = (x.to(DEV), projs, wants)
    return _CACHE[key]


def _dense(projs, dtype):
    return [(R.nf4_fp32_weight(p[0], p[1]).to(dtype).to(DEV), None) + p[2:] for p in projs]


def _cat(ys):
    return torch.cat(ys, dim=1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("Ns,K,lora", NF4_SHAPES)
def test_gemv_rows64_nf4_against_fp64(dtype, nested, Ns, K, lora):
    from unsloth_amd.kernels import decode as D
    x, projs, wants = _case(dtype, nested, Ns, K, lora)
    for M in MS:
        ys = D.linear_group_rows(x[:M], projs)
        for y, want, N in zip(ys, wants, Ns):
            assert y.shape == (M, N)
            scale = want[:M].abs().max().item() + 1e-6
            err = (y.double().cpu() - want[:M]).abs().max().item() / scale
            print(f"M={M} N={N} K={K} err={err:.3e}")
            assert err < (6e-3 if dtype == torch.bfloat16 else 1.5e-3), (M, N, err)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", DENSE_SHAPES)
def test_gemv_rows64_dense_and_fp32_out(dtype, N, K):
    from unsloth_amd.kernels import decode as D
    W = (torch.randn(N, K, generator=g(3)) * 0.05).to(dtype).to(DEV)
    x = torch.randn(64, K, generator=g(4)).to(dtype).to(DEV)
    want = (x.double() @ W.double().t()).cpu()
    for M in MS:
        (y,) = D.gemv_rows64(x[:M], [dict(W=W, N=N, y_f32=True)], nf4=False)
        assert y.dtype == torch.float32 and y.shape == (M, N)
        torch.testing.assert_close(y.double().cpu(), want[:M], rtol=1e-4, atol=1e-4 * want[:M].abs().max().item())
        (y16,) = D.gemv_rows64(x[:M], [dict(W=W, N=N)], nf4=False)
        assert torch.equal(y16, y.to(dtype))                                  # same sum, one rounding


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nf4", [True, False])
def test_wide_launch_equals_16_row_launches(dtype, nf4):
    """M = 64 and M = 37, LoRA and bias on: the wide launch == the concatenation of uamd_gemv_rows launches on its 16-row slices
    (the last one ragged), through linear_group_rows and through gemv_rows / gemv_rows64 directly; gemv_rows64 at M = 8 ==
    gemv_rows at M = 8; two identical launches agree."""
    from unsloth_amd.kernels import decode as D
    x, projs, _ = _case(dtype, True, (4096, 1024, 1024), 4096, True)
    if not nf4:
        projs = _dense(projs, dtype)
    for M in (64, 37):
        wide = _cat(D.linear_group_rows(x[:M], projs))
        assert torch.equal(wide, _cat(D.linear_group_rows(x[:M], projs)))
        parts = [_cat(D.linear_group_rows(x[m0:min(m0 + 16, M)], projs)) for m0 in range(0, M, 16)]
        assert all(p.shape[0] <= D.MAX_ROWS for p in parts)
        assert torch.equal(wide, torch.cat(parts, dim=0)), M
    # the bare launches, one group without LoRA (bias on), fp32 rows out of the dense one
    W, qs, bias = projs[0][0], projs[0][1], projs[0][5]
    N = 4096
    grp = lambda: [dict(W=W, N=N, qs=qs, bias=bias, y_f32=not nf4)]
    for M in (64, 37):
        (wide,) = D.gemv_rows64(x[:M], grp(), nf4=nf4)
        parts = [D.gemv_rows(x[m0:min(m0 + 16, M)], grp(), nf4=nf4)[0] for m0 in range(0, M, 16)]
        assert torch.equal(wide, torch.cat(parts, dim=0)), M
    assert torch.equal(D.gemv_rows64(x[:8], grp(), nf4=nf4)[0], D.gemv_rows(x[:8], grp(), nf4=nf4)[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nf4", [True, False])
def test_a_row_does_not_depend_on_its_neighbours(dtype, nf4):
    """Row m of the M = 64 launch == the M = 1 launch on that row alone == a 40-row launch holding it at another index among
    other rows, bit for bit."""
    from unsloth_amd.kernels import decode as D
    x, projs, _ = _case(dtype, True, (4096, 1024, 1024), 4096, True)
    if not nf4:
        projs = _dense(projs, dtype)
    full = _cat(D.linear_group_rows(x, projs))
    other = torch.randn(40, x.shape[1], generator=g(77)).to(dtype).to(DEV) * 3
    for m in (0, 15, 16, 47, 63):
        one = _cat(D.linear_group_rows(x[m:m + 1], projs))
        assert torch.equal(one[0], full[m]), m
        at = (m + 23) % 40
        mixed = other.clone()
        mixed[at] = x[m]
        forty = _cat(D.linear_group_rows(mixed, projs))
        assert torch.equal(forty[at], full[m]), m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_views_and_untouched_surroundings(dtype):
    """M = 21: x a slice of a wider buffer at a 48-byte offset (ldx > K), the groups writing adjacent column ranges of one
    sentinel-filled [64 + 8, sum N + 48] buffer: same bits as the contiguous launch; columns outside the groups and rows >= M
    come back untouched."""
    from unsloth_amd.kernels import decode as D
    x, projs, _ = _case(dtype, True, (40,), 2080, True)
    x3, projs3, _ = _case(dtype, True, (4096, 1024, 1024), 4096, True)
    for xx, pp in ((x, projs), (x3, projs3)):
        K = xx.shape[1]
        Ns = [int(p[1].shape[0]) for p in pp]
        tot = sum(Ns)
        M = 21
        want = _cat(D.linear_group_rows(xx[:M], pp))
        wide = torch.full((64, K + 64), 7.0, dtype=dtype, device=DEV)
        wide[:, 24:24 + K] = xx                                      # element offset 24 = 48 bytes
        xv = wide[:M, 24:24 + K]
        assert xv.data_ptr() % 16 == 0 and xv.stride(0) > K
        buf = torch.full((64 + 8, tot + 48), -77.0, dtype=dtype, device=DEV)
        ys = D.linear_group_rows(xv, pp, out=buf[:M, 16:16 + tot])
        assert ys[0].data_ptr() == buf[:, 16:].data_ptr()
        assert torch.equal(buf[:M, 16:16 + tot], want)
        assert bool((buf[:, :16] == -77.0).all()) and bool((buf[:, 16 + tot:] == -77.0).all()) and bool((buf[M:] == -77.0).all())
        # M below the rows of the views: the launch takes the first M rows and leaves the others alone
        buf.fill_(-77.0)
        groups = [dict(W=p[0], N=N, qs=p[1], y=buf[:, 16 + c:16 + c + N]) for p, N, c in
                  zip(pp, Ns, [sum(Ns[:i]) for i in range(len(Ns))])]
        D.gemv_rows64(wide[:, 24:24 + K], groups, nf4=True, M=M)
        assert bool((buf[M:] == -77.0).all()) and bool((buf[:M, 16:16 + tot] != -77.0).any())
        assert bool((buf[:, :16] == -77.0).all()) and bool((buf[:, 16 + tot:] == -77.0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nf4", [True, False])
def test_non_finite_rows_stay_in_their_own_outputs(dtype, nf4):
    from unsloth_amd.kernels import decode as D
    x, projs, _ = _case(dtype, True, (4096, 1024, 1024), 4096, True)
    if not nf4:
        projs = _dense(projs, dtype)
    M = 48
    clean = _cat(D.linear_group_rows(x[:M], projs))
    bad = x[:M].clone()
    bad[3] = float("nan")
    bad[40] = float("nan")
    got = _cat(D.linear_group_rows(bad, projs))
    keep = [m for m in range(M) if m not in (3, 40)]
    assert torch.equal(got[keep], clean[keep])
    assert bool(torch.isnan(got[3].float()).all()) and bool(torch.isnan(got[40].float()).all())


def test_argument_errors_launch_nothing():
    from unsloth_amd.kernels import decode as D
    dtype = torch.bfloat16
    x, projs, _ = _case(dtype, True, (256,), 256, False)
    packed, qs = projs[0][0], projs[0][1]
    y = torch.full((65, 256), -5.0, dtype=dtype, device=DEV)
    x65 = torch.zeros(65, 256, dtype=dtype, device=DEV)
    for M in (0, 65):
        with pytest.raises(RuntimeError, match="invalid argument"):
            D.gemv_rows64(x65, [dict(W=packed, N=256, qs=qs, y=y)], nf4=True, M=M)
    with pytest.raises(RuntimeError, match="invalid argument"):        # the 16-row entry point keeps its limit
        D.gemv_rows(x65, [dict(W=packed, N=256, qs=qs, y=y)], nf4=True, M=17)
    torch.cuda.synchronize()
    assert bool((y == -5.0).all())
