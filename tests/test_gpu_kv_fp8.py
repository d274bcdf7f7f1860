"""-m gpu: the two writers of the FP8 KV cache (csrc/decode.hip: kv_store_fp8_kernel, rope_append_fp8_kernel) against the torch
restatement of the stored format (tests/_kv_fp8.py), BITWISE: codes and scales by torch.equal.

  * every finite bf16 / fp16 value with |x| <= 448 at scale exactly 1 (the rounding of the code alone: ties, subnormal codes, both
    zeros, the largest code);
  * randn rows at scales 2^-20 .. 2^15 (the two IEEE divisions), a zero row, a row with a NaN (its scale only), strided sources
    (the transposed view prefill holds) and T = 1 / 17 (a partial block of rows);
  * the append: the slot at kv_len[b] equals the reference quantiser of what uamd_rope_kv_append wrote to a 16-bit cache from
    the same inputs, the rotated q|k row equals that kernel's, no other slot changes, a full cache is left alone."""
import pytest
import torch

from tests import _kv_fp8 as K8

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _store(x_dev, S=None):
    """kv_store_fp8 of x [B, Hk, T, D] (on the device, any strides) into fresh caches: (codes uint8, scales) on the host. The
    caches start as 0xAA / -7 so that a slot the kernel skipped shows."""
    from unsloth_amd.kernels import decode as Dk
    B, Hk, T, D = x_dev.shape
    S = S or T
    codes = torch.full((B, Hk, S, D), 0xAA, dtype=torch.uint8, device=DEV)
    scales = torch.full((B, Hk, S), -7.0, dtype=torch.float32, device=DEV)
    Dk.kv_store_fp8(x_dev, codes, scales)
    return codes.cpu(), scales.cpu()


def _same_scales(got, want):
    """fp32 scales bit for bit, NaN included (any NaN is the same NaN here)."""
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128])
def test_every_16_bit_value_at_scale_one(D, dtype_name):
    dtype = DTYPES[dtype_name]
    rows = K8.every_value_rows(dtype, D)                              # [R, D], R ~ 275 (bf16) / 390 (fp16) at D = 128
    want_c, want_s = K8.quantize_ref(rows)
    assert bool((want_s == 1).all())
    R = rows.shape[0]
    codes, scales = _store(rows.view(1, 1, R, D).to(DEV))
    assert _same_scales(scales.view(R), want_s)
    got, want = codes.view(R, D), K8.as_bytes(want_c)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, [(rows[i, j].item(), hex(got[i, j]), hex(want[i, j])) for i, j in bad[:8].tolist()]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 17])
def test_random_scales_zero_rows_nan_rows_and_strided_sources(T, D, dtype_name):
    dtype = DTYPES[dtype_name]
    B, Hk = 2, 3
    gen = torch.Generator().manual_seed(100 * T + D)
    # the projection output of a prefill: [B, T, Hk * D] inside a wider fused row, K = the transpose(1, 2) view of its k part
    fused = torch.randn(B, T, (Hk + 2) * D, generator=gen)
    ks = torch.arange(-20, 16, 5)                                      # 2^-20 .. 2^15: one per (b, h, t) row, round robin
    expo = ks[torch.arange(B * T * Hk) % len(ks)].view(B, T, Hk, 1).float()
    view = fused[:, :, D:(Hk + 1) * D].view(B, T, Hk, D)
    view.mul_(torch.exp2(expo))
    if dtype == torch.float16:
        view.clamp_(-6e4, 6e4)                                         # (2^15 x randn may leave fp16: that is the NaN row's subject)
    view[0, 0, 1] = 0.0                                                # a zero row
    view[1, T - 1, 2, 5] = float("nan")                                # a row with one NaN
    fused = fused.to(dtype)
    x = fused[:, :, D:(Hk + 1) * D].view(B, T, Hk, D).transpose(1, 2)  # [B, Hk, T, D], strides (T * 5D, D, 5D, 1)
    assert not x.is_contiguous() or T == 1
    want_c, want_s = K8.quantize_ref(x)
    assert want_s[0, 1, 0].item() == 1.0 and torch.isnan(want_s[1, 2, T - 1]) and int(torch.isnan(want_s).sum()) == 1
    S = 32
    xd = fused.to(DEV)[:, :, D:(Hk + 1) * D].view(B, T, Hk, D).transpose(1, 2)
    assert xd.stride() == x.stride()
    codes, scales = _store(xd, S)
    assert _same_scales(scales[:, :, :T], want_s)
    ok = ~torch.isnan(want_s)                                          # the codes of the NaN row are unspecified
    assert torch.equal(codes[:, :, :T][ok], K8.as_bytes(want_c)[ok])
    assert int(K8.as_bytes(want_c)[0, 1, 0].sum()) == 0
    # positions >= T are not touched
    assert bool((codes[:, :, T:] == 0xAA).all()) and bool((scales[:, :, T:] == -7.0).all())
    # every n-th row of a cache is a cache (prefill with `repeat`): rows 0 and 2 of a batch of 4 written, 1 and 3 untouched
    from unsloth_amd.kernels import decode as Dk
    c4 = torch.full((4, Hk, S, D), 0xAA, dtype=torch.uint8, device=DEV)
    s4 = torch.full((4, Hk, S), -7.0, dtype=torch.float32, device=DEV)
    Dk.kv_store_fp8(xd, c4[::2], s4[::2])
    assert torch.equal(c4[::2].cpu(), codes) and _same_scales(s4[::2].cpu(), scales)
    assert bool((c4[1::2] == 0xAA).all()) and bool((s4[1::2] == -7.0).all())


def _rope_tables(D, S, dtype):
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(S).float()[:, None] * inv[None, :]
    return (torch.cat([ang.cos(), ang.cos()], dim=1).to(dtype).to(DEV), torch.cat([ang.sin(), ang.sin()], dim=1).to(dtype).to(DEV))


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("Hq,Hk", [(4, 2), (7, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_the_append_stores_what_the_16_bit_append_would(D, Hq, Hk, dtype_name, with_pos):
    from unsloth_amd.kernels import decode as Dk
    dtype = DTYPES[dtype_name]
    B, S = 3, 48
    gen = torch.Generator().manual_seed(7 * D + Hq)
    qkv = (torch.randn(B, (Hq + 2 * Hk) * D, generator=gen) * 3).to(dtype)
    lens = (5, S, 17)                                                  # row 1: kv_len == s_max, nothing is written
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rope_pos = torch.tensor([31, 2, 0], dtype=torch.int32, device=DEV) if with_pos else None
    cos, sin = _rope_tables(D, S + 1, dtype)
    # the 16-bit kernel on the same inputs
    k16 = torch.zeros(B, Hk, S, D, dtype=dtype, device=DEV)
    v16 = torch.zeros(B, Hk, S, D, dtype=dtype, device=DEV)
    row16 = qkv.to(DEV)
    Dk.rope_kv_append(row16, cos, sin, kv_len, k16, v16, Hq, Hk, D, rope_pos=rope_pos)
    # the FP8 kernel over caches that already hold something everywhere
    k0 = K8.quantize_ref(torch.randn(B, Hk, S, D, generator=gen).to(dtype))
    v0 = K8.quantize_ref(torch.randn(B, Hk, S, D, generator=gen).to(dtype))
    kc, ks = K8.as_bytes(k0[0]).to(DEV), k0[1].to(DEV)
    vc, vs = K8.as_bytes(v0[0]).to(DEV), v0[1].to(DEV)
    row8 = qkv.to(DEV)
    Dk.rope_kv_append_fp8(row8, cos, sin, kv_len, kc, vc, ks, vs, Hq, Hk, D, rope_pos=rope_pos)
    assert torch.equal(row8, row16)                                    # q and k rotated as there, v untouched
    assert not torch.equal(row8[:, :(Hq + Hk) * D].cpu(), qkv[:, :(Hq + Hk) * D])
    want_kc, want_ks = K8.as_bytes(k0[0]).clone(), k0[1].clone()
    want_vc, want_vs = K8.as_bytes(v0[0]).clone(), v0[1].clone()
    for b, L in enumerate(lens):
        if L < S:
            c, s = K8.quantize_ref(k16[b, :, L].cpu())
            want_kc[b, :, L], want_ks[b, :, L] = K8.as_bytes(c), s
            c, s = K8.quantize_ref(v16[b, :, L].cpu())
            want_vc[b, :, L], want_vs[b, :, L] = K8.as_bytes(c), s
            assert float(k16[b, :, L].float().abs().sum()) > 0
    assert torch.equal(kc.cpu(), want_kc) and torch.equal(vc.cpu(), want_vc)
    assert _same_scales(ks.cpu(), want_ks) and _same_scales(vs.cpu(), want_vs)
    # ... and the store kernel makes the same bytes of the same key
    codes, scales = _store(k16[:, :, 5:6])
    c, s = K8.quantize_ref(k16[:, :, 5:6].cpu())
    assert torch.equal(codes, K8.as_bytes(c)) and _same_scales(scales, s)
    assert torch.equal(codes[0, :, 0], kc.cpu()[0, :, 5]) and torch.equal(scales[0, :, 0], ks.cpu()[0, :, 5])


def test_the_launchers_refuse_what_the_kernels_do_not_cover():
    from unsloth_amd.kernels import decode as Dk
    x = torch.zeros(1, 2, 4, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AssertionError):                                # head dim 96
        Dk.kv_store_fp8(x, torch.zeros(1, 2, 8, 96, dtype=torch.uint8, device=DEV), torch.zeros(1, 2, 8, device=DEV))
    x = torch.zeros(1, 2, 9, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AssertionError):                                # more positions than the cache has
        Dk.kv_store_fp8(x, torch.zeros(1, 2, 8, 64, dtype=torch.uint8, device=DEV), torch.zeros(1, 2, 8, device=DEV))
    x = torch.zeros(1, 2, 4, 64, dtype=torch.float32, device=DEV)
    with pytest.raises((RuntimeError, TypeError)):                     # a 16-bit source
        Dk.kv_store_fp8(x, torch.zeros(1, 2, 8, 64, dtype=torch.uint8, device=DEV), torch.zeros(1, 2, 8, device=DEV))
