"""Helpers of the attention mask-edge tests (tests/test_attention_edge_inputs.py on the host, tests/test_gpu_attention_edges.py on
the GPU): inputs whose softmax mass sits ON the edges of the (lo, hi) band, an fp64 reference with a dense mask, a model of what
a correct 16-bit flash attention rounds away, and a row-wise error. Nothing here imports the product: the masks are written from
the docstrings of `attention_band` / `document_band` (query q attends keys lo[q] <= key <= q, or <= hi[q] when not causal)."""
import functools
import math

import torch

# id -> (B, T, Hq, Hk, D, document lengths over the flattened batch or None, sliding window or None, causal)
CASES = {
    "causal":       (1, 200, 4, 1, 128, None, None, True),        # ragged T: key T does not exist, the last tile must mask it
    "win64":        (1, 320, 4, 2, 128, None, 64, True),          # lower edge exactly one 64-key tile back
    "win65":        (1, 321, 8, 2, 128, None, 65, True),          # one past a tile; G = 4
    "win1":         (1, 130, 4, 4, 128, None, 1, True),           # every row sees itself only
    "win2_d64_g7":  (1, 130, 14, 2, 64, None, 2, True),           # Qwen2.5-0.5B layout: 64-column class, head passes 4 + 2 + 1
    "win129_g7":    (1, 400, 7, 1, 128, None, 129, True),         # window spans two tiles + 1
    "packed":       (1, 512, 8, 2, 128, [1, 2, 3, 250, 64, 63, 129], None, True),   # boundaries on and beside 32- / 64-row tile edges
    "packed_win":   (2, 256, 4, 1, 128, [100, 156, 31, 33, 192], 33, True),         # B = 2, a window inside documents
    "packed_d64":   (2, 200, 8, 2, 64, [64, 36, 100, 1, 63, 65, 71], None, True),
    "docs_nc":      (1, 384, 4, 2, 128, [64, 65, 127, 1, 127], None, False),        # `hi` edge on the key side, a one-token document
    "docs_nc_d80":  (1, 300, 4, 4, 80, [33, 31, 128, 108], None, False),            # the ViT head_dim: 96-column class
    # a head dim that is no multiple of 8 runs zero-padded (kernels/attention.py _pad_qkv); the third document (190 .. 210 of the
    # flattened batch) is cut at the boundary between the two batch rows
    "packed_d36":   (2, 200, 8, 2, 36, [64, 36, 90, 21, 63, 65, 61], None, True),
}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
TENSORS = ("o", "lse", "dq", "dk", "dv")


def case_band(B, T, lengths, window, causal):
    """(lo, hi) int64 [B, T] of a case, in plain loops: documents lie back to back over the flattened batch of B*T tokens, tokens
    past their sum form one more document, a document is cut where a batch row ends, and a window W keeps |q - key| < W."""
    bounds, end = [], 0
    for n in (lengths or []):
        if n > 0:
            bounds.append((end, min(end + n, B * T)))
            end = min(end + n, B * T)
    if end < B * T:
        bounds.append((end, B * T))
    lo = torch.zeros(B, T, dtype=torch.int64)
    hi = torch.zeros(B, T, dtype=torch.int64)
    for s, e in bounds:
        for g in range(s, e):
            b, t = divmod(g, T)
            first, last = max(s, b * T) - b * T, min(e - 1, b * T + T - 1) - b * T
            if window:
                assert causal, "the table has no non-causal window"
                first, last = max(first, t - (window - 1)), min(last, t + (window - 1))
            lo[b, t], hi[b, t] = first, last
    return lo, hi


def _dense(lo, up):
    T = lo.shape[1]
    key = torch.arange(T)[None, None, :]
    return ((key >= lo[:, :, None]) & (key <= up[:, :, None]))[:, None]


def _upper(lo, hi, causal):
    return torch.arange(lo.shape[1])[None, :].expand_as(lo) if causal else hi


def allowed_from_band(lo, hi, causal):
    """Dense bool [B, 1, T, T] of a band: allowed[b, 0, q, key] = lo[b, q] <= key <= (q if causal else hi[b, q])."""
    lo, hi = lo.long().cpu(), hi.long().cpu()
    return _dense(lo, _upper(lo, hi, causal))


def mutants(lo, hi, causal):
    """The four off-by-one masks of a band as [(name, allowed)]: the lower edge one key further / nearer, the upper edge one key
    further / nearer, each clamped to [0, T). A row that would become empty keeps its diagonal; a mutant equal to the true mask
    (window 1 with an edge pulled in) is left out."""
    lo, hi = lo.long().cpu(), hi.long().cpu()
    T = lo.shape[1]
    up = _upper(lo, hi, causal)
    true = _dense(lo, up)
    diag = torch.eye(T, dtype=torch.bool)[None, None]
    out = []
    for name, dl, du in (("lo-1", -1, 0), ("lo+1", 1, 0), ("up+1", 0, 1), ("up-1", 0, -1)):
        m = _dense((lo + dl).clamp(0, T - 1), (up + du).clamp(0, T - 1))
        empty = ~m.any(-1, keepdim=True)
        m = m | (empty & diag)
        if not torch.equal(m, true):
            out.append((name, m))
    return out


def _forward(q, k, v, scale, allowed):
    G = q.shape[2] // k.shape[2]
    kk, vv = k.repeat_interleave(G, dim=2), v.repeat_interleave(G, dim=2)
    s = torch.einsum("bthd,bshd->bhts", q, kk) * scale
    s = s.masked_fill(~allowed, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    return p, lse, kk, vv


def ref64(q, k, v, do, scale, allowed):
    """fp64 attention under the dense mask `allowed` [B,1,T,T], GQA by repeat_interleave; (o, lse, dq, dk, dv) through autograd."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    p, lse, _, vv = _forward(q, k, v, scale, allowed)
    o = torch.einsum("bhts,bshd->bthd", p, vv)
    o.backward(do.double())
    return o.detach(), lse.detach(), q.grad, k.grad, v.grad


def rounding_model(q, k, v, do, scale, allowed, dtype):
    """The same in fp32 with the rounding points the kernels document (csrc/attention.hip): P is rounded to `dtype` before P V and
    P^T dO, O is rounded, Delta = rowsum(dO * O) reads the ROUNDED O, dS = P (dP - Delta) is rounded, dQ / dK / dV are rounded
    once. What a correct 16-bit flash attention loses -- the yardstick of the GPU tests, not a model of any kernel's schedule."""
    def r(x):
        return x.to(dtype).float()
    B, T, Hq, D = q.shape
    Hk = k.shape[2]
    G = Hq // Hk
    q, k, v, do = (t.detach().float() for t in (q, k, v, do))
    p, lse, kk, vv = _forward(q, k, v, scale, allowed)
    pr = r(p)
    o = r(torch.einsum("bhts,bshd->bthd", pr, vv))
    dv = torch.einsum("bhts,bthd->bshd", pr, do)
    dp = torch.einsum("bthd,bshd->bhts", do, vv)
    delta = (do * o).sum(-1).permute(0, 2, 1)                       # [B,Hq,T]
    ds = r(p * (dp - delta[..., None]))
    dq = r(torch.einsum("bhts,bshd->bthd", ds, kk) * scale)
    dk = torch.einsum("bhts,bthd->bshd", ds, q) * scale
    dk = r(dk.view(B, T, Hk, G, D).sum(3))
    dv = r(dv.view(B, T, Hk, G, D).sum(3))
    return o, lse, dq, dk, dv


def row_err(got, ref):
    """max over rows of ||got_row - ref_row|| / (||ref_row|| + rms over rows of ||ref_row||); a row is one (b, t, head) vector of
    the last axis. The rms term keeps rows whose true value is almost zero (the first token of a document, dQ under a peaked
    softmax) from dividing by nothing."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    e = (got - ref).flatten(0, -2).norm(dim=-1)
    n = ref.flatten(0, -2).norm(dim=-1)
    return float((e / (n + n.pow(2).mean().sqrt())).max())


def edge_inputs(B, T, Hq, Hk, D, lo, hi, causal, dtype, seed):
    """(q, k, v, do) in `dtype`. Keys are codes of i.i.d. +-1 (exact in both types; a code scores D with itself, +-sqrt(D) with
    another). Query head h plays role h % 4 with up[t] = t when causal, hi[t] otherwise, and code(i) = 0 outside [0, T):
      0: a code(lo) + b code(lo - 1)      the oldest allowed key carries the mass, the first forbidden key below would carry more
      1: a code(up) + b code(up + 1)      the same at the upper edge
      2: a code((lo + up) // 2) + b code(lo - 1) + b code(up + 1)
      3: randn                            the diffuse control
    plus 0.25 randn on every head; a = 0.55 sqrt(128 / D), b = 0.85 sqrt(128 / D): after the 1 / sqrt(D) scale the allowed edge key
    scores about 6.2, its forbidden neighbour about 9.6, the noise about 1.1."""
    gen = torch.Generator().manual_seed(seed)
    lo, hi = lo.long().cpu(), hi.long().cpu()
    G = Hq // Hk
    k = (torch.randint(0, 2, (B, T, Hk, D), generator=gen) * 2 - 1).float()
    up = _upper(lo, hi, causal)
    a, b = 0.55 * math.sqrt(128 / D), 0.85 * math.sqrt(128 / D)

    def code(idx, kh):
        ok = ((idx >= 0) & (idx < T)).float()[..., None]
        return torch.gather(k[:, :, kh], 1, idx.clamp(0, T - 1)[..., None].expand(B, T, D)) * ok

    q = torch.empty(B, T, Hq, D)
    for h in range(Hq):
        kh, role = h // G, h % 4
        if role == 0:
            x = a * code(lo, kh) + b * code(lo - 1, kh)
        elif role == 1:
            x = a * code(up, kh) + b * code(up + 1, kh)
        elif role == 2:
            x = a * code((lo + up) // 2, kh) + b * code(lo - 1, kh) + b * code(up + 1, kh)
        else:
            x = torch.randn(B, T, D, generator=gen)
        q[:, :, h] = x + 0.25 * torch.randn(B, T, D, generator=gen)
    v = torch.randn(B, T, Hk, D, generator=gen)
    do = torch.randn(B, T, Hq, D, generator=gen)
    return q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype)


@functools.lru_cache(maxsize=None)
def build_case(name, dtype_name):
    """One case of the table, computed once per process and shared by every test that reads it (nothing in it is written to):
    the band, the dense mask, the inputs, the fp64 reference, the rounding model and the model's row errors."""
    B, T, Hq, Hk, D, lengths, window, causal = CASES[name]
    dtype = DTYPES[dtype_name]
    lo, hi = case_band(B, T, lengths, window, causal)
    allowed = allowed_from_band(lo, hi, causal)
    seed = 1000 + sorted(CASES).index(name)
    q, k, v, do = edge_inputs(B, T, Hq, Hk, D, lo, hi, causal, dtype, seed)
    scale = 1.0 / math.sqrt(D)
    ref = dict(zip(TENSORS, ref64(q, k, v, do, scale, allowed)))
    model = dict(zip(TENSORS, rounding_model(q, k, v, do, scale, allowed, dtype)))
    # (a row of the LSE is one number; a reference that is zero everywhere -- dQ and dK under window 1 -- has no relative error)
    model_err = {t: row_err(model[t].unsqueeze(-1) if t == "lse" else model[t], ref[t].unsqueeze(-1) if t == "lse" else ref[t])
                 if bool(ref[t].any()) else None for t in TENSORS}
    return dict(shape=(B, T, Hq, Hk, D), lengths=lengths, window=window, causal=causal, dtype=dtype, lo=lo, hi=hi,
                allowed=allowed, q=q, k=k, v=v, do=do, scale=scale, ref=ref, model=model, model_err=model_err)


BOUND_FACTOR = 4        # a kernel output may sit this many times the rounding model's row error from the fp64 reference


def judge(c, tensor, got):
    """(row_err of `got` against the case's fp64 reference, the model's, whether the first is within BOUND_FACTOR x the second)."""
    err, model = row_err(got, c["ref"][tensor]), c["model_err"][tensor]
    return err, model, bool(err <= BOUND_FACTOR * model)
