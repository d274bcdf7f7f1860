"""-m gpu: uamd_attn_extend (csrc/decode.hip), attention of a chunk of T_c tokens appended to a live 16-bit cache, against a plain
fp64 softmax over the cache's own contents. Bound per output element: 3 u max |V[:, d]| over the row's key range, u = 2^-8 (bf16)
/ 2^-11 (f16): P rounded once and the output rounded once move a convex combination of the V column by at most u max |V| each;
the third u covers the fp32 summation order and exp2."""
import math

import pytest
import torch

from tests._decode_batched import DEV, g

pytestmark = pytest.mark.gpu
S_MAX, HK = 512, 2
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BF, HF = (128, torch.bfloat16), (64, torch.float16)
# (D, dtype), G, T_c, kv_len pair, window. Tokens per tile: 128 / 32 / 18 / 16 at G = 1 / 4 / 7 / 8 (G = 7: two idle rows).
CASES = [
    (BF, 1, 130, (0, 1), 0),          # empty old cache; the diagonal crosses the fill seam at key 128; tile seam; last tile of 2 tokens
    (BF, 4, 33, (127, 128), 0),       # first chunk key at / behind the fill seam; tile seam at token 32
    (BF, 7, 19, (129, 300), 200),     # idle rows; a window that starts in the old cache
    (BF, 8, 17, (127, 128), 16),      # a window that starts inside the chunk
    (BF, 1, 17, (129, 300), 200),
    (BF, 7, 130, (127, 128), 16),     # 8 tiles of 18 tokens, the last partial
    (BF, 4, 1, (0, 1), 200),          # one token on an empty cache: only itself
    (HF, 1, 129, (129, 300), 16),
    (HF, 4, 130, (129, 300), 200),    # the fill seam at key 128 off the diagonal (unmasked groups), window start in the old cache
    (HF, 7, 1, (127, 128), 0),        # the new key is the last of fill 0 / the first of fill 1
    (HF, 8, 17, (0, 1), 0),
    (HF, 8, 130, (129, 300), 0),
    (HF, 1, 130, (127, 128), 200),
]


def _inputs(D, dtype, G, Tc, kv, window, seed=0):
    """Slots at or past kv_len + T_c are NaN. Row (b, j, h): (h + j) % 4 = 1 / 2 / 3 puts most of the mass (q along that key) on the
    row's first key / its last key / the first key past its range, so a range off by one moves the output far past the bound."""
    B, Hq = len(kv), HK * G
    k = torch.randn(B, HK, S_MAX, D, generator=g(seed)).to(dtype).to(DEV)
    v = torch.randn(B, HK, S_MAX, D, generator=g(seed + 1)).to(dtype).to(DEV)
    q = torch.randn(B, Tc, Hq, D, generator=g(seed + 2)).to(DEV)
    kv_t = torch.tensor(kv, device=DEV)
    t = kv_t[:, None] + torch.arange(Tc, device=DEV)[None, :] + 1                     # [B, Tc] range ends
    first = (t - window).clamp_min(0) if window else torch.zeros_like(t)
    mode = (torch.arange(Hq, device=DEV)[None, None, :] + torch.arange(Tc, device=DEV)[None, :, None]) % 4
    hot = torch.where(mode == 1, first[..., None], torch.where(mode == 2, t[..., None] - 1, t[..., None]))
    hot = torch.minimum(hot, (kv_t + Tc - 1)[:, None, None])                          # (the last token has no key past its range)
    kh = k.float()[torch.arange(B, device=DEV)[:, None, None], torch.arange(Hq, device=DEV)[None, None, :] // G, hot]      # [B, Tc, Hq, D]
    q = torch.where((mode > 0)[..., None], kh * (12.0 / math.sqrt(D)), q).to(dtype)   # score of the hot key: about 12
    for b in range(B):
        k[b, :, kv[b] + Tc:] = float("nan")
        v[b, :, kv[b] + Tc:] = float("nan")
    return q.reshape(B * Tc, Hq * D).contiguous(), k, v, kv_t.to(torch.int32), first, t


def _ref64(q, k, v, first, t, G):
    B, Tc = t.shape
    D = k.shape[-1]
    q64 = q.view(B, Tc, -1, D).double()
    key = torch.arange(S_MAX, device=DEV)
    inr = (key[None, None, :] >= first[..., None]) & (key[None, None, :] < t[..., None])      # [B, Tc, S]
    k64 = torch.nan_to_num(k.double()).repeat_interleave(G, 1)                                 # [B, Hq, S, D]
    v64 = torch.nan_to_num(v.double()).repeat_interleave(G, 1)
    s = torch.einsum("bjhd,bhsd->bjhs", q64, k64) / math.sqrt(D)
    p = torch.softmax(s.masked_fill(~inr[:, :, None, :], float("-inf")), dim=-1)
    out = torch.einsum("bjhs,bhsd->bjhd", p, v64)
    vmax = torch.stack([torch.where(inr[b, :, None, :, None], v64[b].abs()[None].float(), 0).amax(2) for b in range(B)])
    return out.reshape(B * Tc, -1), vmax.double().reshape(B * Tc, -1)


@pytest.mark.parametrize("dd,G,Tc,kv,window", CASES)
def test_extend_matches_fp64_over_each_rows_range(dd, G, Tc, kv, window):
    from unsloth_amd.kernels import decode as Dk
    D, dtype = dd
    q, k, v, kv_len, first, t = _inputs(D, dtype, G, Tc, kv, window)
    out = torch.full_like(q, float("nan"))
    Dk.attn_extend(q, k, v, kv_len, Tc, out, 1.0 / math.sqrt(D), window=window)
    ref, vmax = _ref64(q, k, v, first, t, G)
    assert bool(torch.isfinite(out).all()), "a slot past kv_len + T_c was read, or a row was not written"
    ratio = ((out.double() - ref).abs() / (3 * U[dtype] * vmax)).max().item()
    print(f"attn_extend D={D} {dtype} G={G} T_c={Tc} kv={kv} window={window}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("dd,G,Tc,kv,window", [CASES[1], CASES[8]])
def test_append_touches_only_the_chunk_and_later_tokens_never_enter(dd, G, Tc, kv, window):
    """Slots outside [kv_len, kv_len + T_c) keep their bits; row j's output is bitwise the same when the chunk is cut after j."""
    from unsloth_amd.kernels import decode as Dk
    D, dtype = dd
    B, Hq = len(kv), HK * G
    _, k, v, kv_len, _, _ = _inputs(D, dtype, G, Tc, kv, window, seed=5)
    k, v = torch.nan_to_num(k, nan=3.0), torch.nan_to_num(v, nan=3.0)
    k0, v0 = k.clone(), v.clone()
    qkv = torch.randn(B * Tc, (Hq + 2 * HK) * D, generator=g(9)).to(dtype).to(DEV)
    ang = torch.arange(S_MAX)[:, None] * torch.exp(-torch.arange(D // 2)[None, :] * (math.log(1e4) / (D // 2)))
    cos, sin = torch.cos(ang).to(dtype).to(DEV), torch.sin(ang).to(dtype).to(DEV)
    Dk.rope_kv_append_span(qkv, cos, sin, kv_len, k, v, Tc, Hq, HK, D)
    out = torch.empty(B * Tc, Hq * D, dtype=dtype, device=DEV)
    Dk.attn_extend(qkv[:, :Hq * D], k, v, kv_len, Tc, out, 1.0 / math.sqrt(D), window=window)
    for b in range(B):
        outside = torch.ones(S_MAX, dtype=torch.bool, device=DEV)
        outside[kv[b]:kv[b] + Tc] = False
        for new, old in ((k, k0), (v, v0)):
            assert torch.equal(new[b][:, outside].view(torch.int16), old[b][:, outside].view(torch.int16))
    q3 = qkv[:, :Hq * D].view(B, Tc, Hq * D)
    for j in sorted({0, 128 // G - 1, 128 // G, Tc - 2} & set(range(Tc - 1))):
        cut = torch.empty(B * (j + 1), Hq * D, dtype=dtype, device=DEV)
        Dk.attn_extend(q3[:, :j + 1].reshape(B * (j + 1), -1), k, v, kv_len, j + 1, cut, 1.0 / math.sqrt(D), window=window)
        assert torch.equal(cut.view(B, j + 1, -1)[:, j].view(torch.int16), out.view(B, Tc, -1)[:, j].view(torch.int16)), j
