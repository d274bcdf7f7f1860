"""-m gpu: uamd_gemv_rows (csrc/decode.hip, kernels/decode.py gemv_rows / linear_group_rows) -- the GEMV for M = 1 .. 16 token
rows that share one pass over the weights: against the exact fp64 product of the code values, bitwise row independence,
strided views with sentinels around them, a non-finite row among finite ones, and the argument errors."""
import pytest
import torch

from oracle import ref_ops as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [((256,), 256, False), ((4096, 1024, 1024), 4096, True), ((1024, 1024), 14336, True), ((40,), 2080, True),
          ((5, 3, 2, 9), 8192, False)]
MS = (1, 2, 3, 8, 16)
_CACHE = {}


def g(seed):
    return torch.Generator().manual_seed(seed)


def _case(dtype, nested, Ns, K, lora):
    """The projections of one shape and the fp64 truth for 16 token rows, built once and shared by every M."""
    key = (dtype, nested, Ns, K, lora)
    if key in _CACHE:
        return _CACHE[key]
    from unsloth_amd.nf4 import quantize_nf4
    x = torch.randn(16, K, generator=g(1)).to(dtype)
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


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("Ns,K,lora", SHAPES)
def test_gemv_rows_nf4_against_fp64(dtype, nested, Ns, K, lora):
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
@pytest.mark.parametrize("N,K", [(128, 512), (1000, 4096), (3, 14336), (128256 // 8, 4096)])
def test_gemv_rows_dense_and_fp32_out(dtype, N, K):
    from unsloth_amd.kernels import decode as D
    W = (torch.randn(N, K, generator=g(3)) * 0.05).to(dtype).to(DEV)
    x = torch.randn(16, K, generator=g(4)).to(dtype).to(DEV)
    want = (x.double() @ W.double().t()).cpu()
    for M in MS:
        (y,) = D.gemv_rows(x[:M], [dict(W=W, N=N, y_f32=True)], nf4=False)
        assert y.dtype == torch.float32 and y.shape == (M, N)
        torch.testing.assert_close(y.double().cpu(), want[:M], rtol=1e-4, atol=1e-4 * want[:M].abs().max().item())
        (y16,) = D.gemv_rows(x[:M], [dict(W=W, N=N)], nf4=False)
        assert torch.equal(y16, y.to(dtype))                                  # same sum, one rounding


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nf4", [True, False])
def test_a_row_does_not_depend_on_its_neighbours(dtype, nf4):
    """Row m of the M = 16 launch == the M = 1 launch on that row alone == an M = 5 launch holding it at another index among
    other rows, bit for bit; and two identical launches agree."""
    from unsloth_amd.kernels import decode as D
    x, projs, _ = _case(dtype, True, (4096, 1024, 1024), 4096, True)
    if not nf4:
        projs = [(R.nf4_fp32_weight(p[0], p[1]).to(dtype).to(DEV), None) + p[2:] for p in projs]
    full = torch.cat(D.linear_group_rows(x, projs), dim=1)
    assert torch.equal(full, torch.cat(D.linear_group_rows(x, projs), dim=1))
    other = torch.randn(5, x.shape[1], generator=g(77)).to(dtype).to(DEV) * 3
    for m in (0, 3, 7, 15):
        one = torch.cat(D.linear_group_rows(x[m:m + 1], projs), dim=1)
        assert torch.equal(one[0], full[m]), m
        at = (m + 2) % 5
        mixed = other.clone()
        mixed[at] = x[m]
        five = torch.cat(D.linear_group_rows(mixed, projs), dim=1)
        assert torch.equal(five[at], full[m]), m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_views_and_untouched_surroundings(dtype):
    """x a slice of a wider buffer at a 16-byte-aligned offset (ldx > K), the groups writing adjacent column ranges of one
    wider sentinel-filled buffer (ldy > sum N): same bits as the contiguous launch; columns outside the groups and rows >= M
    come back untouched."""
    from unsloth_amd.kernels import decode as D
    x, projs, _ = _case(dtype, True, (40,), 2080, True)
    x3, projs3, _ = _case(dtype, True, (4096, 1024, 1024), 4096, True)
    for xx, pp in ((x, projs), (x3, projs3)):
        K = xx.shape[1]
        Ns = [int(p[1].shape[0]) for p in pp]
        tot = sum(Ns)
        M = 5
        want = torch.cat(D.linear_group_rows(xx[:M], pp), dim=1)
        wide = torch.full((16, K + 64), 7.0, dtype=dtype, device=DEV)
        wide[:, 24:24 + K] = xx                                      # element offset 24 = 48 bytes
        xv = wide[:M, 24:24 + K]
        assert xv.data_ptr() % 16 == 0 and xv.stride(0) > K
        buf = torch.full((8, tot + 48), -77.0, dtype=dtype, device=DEV)
        ys = D.linear_group_rows(xv, pp, out=buf[:M, 16:16 + tot])
        assert ys[0].data_ptr() == buf[:, 16:].data_ptr()
        assert torch.equal(buf[:M, 16:16 + tot], want)
        assert bool((buf[:, :16] == -77.0).all()) and bool((buf[:, 16 + tot:] == -77.0).all()) and bool((buf[M:] == -77.0).all())
        # M below the rows of the views: the launch takes the first M rows and leaves the others alone
        buf.fill_(-77.0)
        groups = [dict(W=p[0], N=N, qs=p[1], y=buf[:, 16 + c:16 + c + N]) for p, N, c in
                  zip(pp, Ns, [sum(Ns[:i]) for i in range(len(Ns))])]
        D.gemv_rows(wide[:8, 24:24 + K], groups, nf4=True, M=2)
        assert bool((buf[2:] == -77.0).all()) and bool((buf[:2, 16:16 + tot] != -77.0).any())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nf4", [True, False])
def test_a_non_finite_row_stays_in_its_own_outputs(dtype, nf4):
    from unsloth_amd.kernels import decode as D
    x, projs, _ = _case(dtype, True, (1024, 1024), 14336, True)
    if not nf4:
        projs = [(R.nf4_fp32_weight(p[0], p[1]).to(dtype).to(DEV), None) + p[2:] for p in projs]
    M = 8
    clean = torch.cat(D.linear_group_rows(x[:M], projs), dim=1)
    bad = x[:M].clone()
    bad[3] = float("nan")
    got = torch.cat(D.linear_group_rows(bad, projs), dim=1)
    keep = [m for m in range(M) if m != 3]
    assert torch.equal(got[keep], clean[keep])
    assert bool(torch.isnan(got[3].float()).all())


def test_argument_errors_launch_nothing():
    from unsloth_amd.kernels import decode as D
    dtype = torch.bfloat16
    x, projs, _ = _case(dtype, True, (256,), 256, False)
    packed, qs = projs[0][0], projs[0][1]
    y = torch.full((17, 256), -5.0, dtype=dtype, device=DEV)
    x17 = torch.zeros(17, 256, dtype=dtype, device=DEV)
    for M in (0, 17):
        with pytest.raises(RuntimeError, match="invalid argument"):
            D.gemv_rows(x17, [dict(W=packed, N=256, qs=qs, y=y)], nf4=True, M=M)
    with pytest.raises(RuntimeError, match="invalid argument"):        # K % 32 != 0 for NF4
        D.gemv_rows(x17[:4, :232], [dict(W=packed, N=256, qs=qs, y=y)], nf4=True)
    torch.cuda.synchronize()
    assert bool((y == -5.0).all())
