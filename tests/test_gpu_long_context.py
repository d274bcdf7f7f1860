"""-m gpu: the kernels at long-context sizes -- operands that span 2^31 / 2^32 bytes, tens of thousands of tokens per launch.

The 256-tile GEMMs address every operand through 32-bit byte offsets from its base, and their host entry points refuse a
launch whose A, rank block or B would span 4 GiB (csrc/gemm256.hip). kernels/utils.py issues such launches as row chunks
(NT / NN) or contraction chunks (TN) below utils.GEMM_SPAN_LIMIT. The tests here check, against fp32 products on the GPU and
fp64 on sampled rows, at the tolerances the suite uses for the same kernels at short lengths (test_gpu_nf4_gemm._check_gemm,
test_gpu_lora_blocks.test_lora_mlp):
  * each launch form just below and just above the line, through padded row strides (a few GB of memory, milliseconds of
    compute), with and without a rank block and `accumulate`, bf16 and fp16;
  * that chunking is invisible below the line: forced chunks equal one launch bit for bit (NT / NN), and a launch below the
    limit is exactly one library call;
  * the LoRA MLP block (NF4, r = 16, SwiGLU, the fused activation path) forward and backward at Qwen2-7B and Llama-3-8B widths
    past the ~57 K / ~75 K token line where the down projection's A operand (h, row stride 2 I + 64) reaches 4 GiB;
  * the row-indexed kernels past 2^31 elements: cross-entropy forward / in-place backward, RMSNorm forward / backward and the
    fused add form, RoPE with int32 positions up to 131,071.
Not covered here yet: a packed one-layer step at 81,920 tokens against its documents run one by one, attention at
T = 65,536 / 131,072 (packed, windowed, both sides of the persistent-kernel guard) and split-KV decode over 64K-128K caches.
A test skips only when the device has less free memory than it needs, and says how much."""
import pytest
import torch

from oracle import ref_ops as R
from tests._util import EPS, assert_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
GiB = 1 << 30


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(autouse=True)
def _fp32_matmul_and_free_memory():
    """Reference products in true fp32 (no TF32 / reduced-precision reductions); memory handed back after each test."""
    old = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cuda.matmul.allow_fp16_reduced_precision_reduction,
           torch.backends.cuda.matmul.allow_bf16_reduced_precision_reduction)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cuda.matmul.allow_fp16_reduced_precision_reduction = False
    torch.backends.cuda.matmul.allow_bf16_reduced_precision_reduction = False
    yield
    (torch.backends.cuda.matmul.allow_tf32, torch.backends.cuda.matmul.allow_fp16_reduced_precision_reduction,
     torch.backends.cuda.matmul.allow_bf16_reduced_precision_reduction) = old
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GiB:
        pytest.skip(f"needs {gib} GiB of free device memory, {free / GiB:.1f} GiB free")


def _ulp_gpu(got, want, dtype, ulps=1.0, atol=None, allow_frac=0.0, what=""):
    """tests._util.assert_ulp evaluated on the device (the same bound, for outputs of tens of millions of elements)."""
    a, b = got.float(), want.float()
    assert a.shape == b.shape, what
    assert torch.isfinite(a).all(), f"{what}: non-finite values in result"
    eps = EPS[dtype]
    if atol is None:
        atol = eps * float(b.abs().mean() + 1e-30) * 0.5
    bound = ulps * eps * b.abs() + atol
    err = (a - b).abs()
    bad = err > bound
    n_bad = int(bad.sum())
    if n_bad:
        frac = n_bad / bad.numel()
        worse = int((err > 2 * bound).sum())
        idx = torch.nonzero(bad)[0].tolist()
        msg = (f"{what}: {n_bad}/{bad.numel()} beyond {ulps} ulp ({frac:.2e}); first at {idx}: got {a[tuple(idx)].item()!r} "
               f"want {b[tuple(idx)].item()!r}; max err {err.max().item():.4e}")
        assert worse == 0 and frac <= allow_frac, msg


def _gemm_atol(want, dtype, K):
    """test_gpu_nf4_gemm._check_gemm's accumulation-noise term."""
    scale = float(want.abs().mean())
    return EPS[dtype] * scale * 0.5 + 1e-6 * scale * K ** 0.5


def _check_gemm(got, want, dtype, K, what):
    _ulp_gpu(got, want, dtype, ulps=1, atol=_gemm_atol(want, dtype, K), allow_frac=1e-3, what=what)


def _rel_fro(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _sample_rows(M, row_bytes):
    """first / last rows, rows on 32 / 64 / 256-row tile edges (+-1), and the rows whose byte offset from the operand base
    crosses 2^31 and 2^32."""
    rows = {0, 1, M - 2, M - 1}
    for t in (32, 64, 256):
        for base in (t, 2 * t, (M // t) * t):
            rows |= {base - 1, base, base + 1}
    for p in (31, 32):
        r = -(-(1 << p) // row_bytes)
        rows |= {r - 1, r, r + 1}
    return torch.tensor(sorted(r for r in rows if 0 <= r < M))


# ------------------------------------------------------------------------------------------------ GEMM across the 4 GiB span
LDA = 32768                    # padded row stride (elements): 64 KiB rows, so 65,536 rows span 4 GiB
K_MAIN, RK = 256, 64           # the contraction width A contributes; the rank block's K tiles (columns K_MAIN .. +64 of the
                               # same padded rows, so XK spans exactly what A spans)
LINE = (1 << 32) // (LDA * 2)  # 65536 rows: the first M whose A would span 4 GiB
BUF_ROWS = LINE + 256


@pytest.fixture(scope="module")
def padded():
    """One [BUF_ROWS, LDA] 16-bit buffer (4.3 GB) shared by the span tests; columns never written by a test stay NaN, so a
    kernel that reads past its operand's columns produces non-finite output."""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * GiB:
        pytest.skip(f"needs 12 GiB of free device memory, {free / GiB:.1f} GiB free")
    buf = torch.empty(BUF_ROWS, LDA, dtype=torch.int16, device=DEV)
    yield buf
    del buf
    torch.cuda.empty_cache()


def _fill(buf, dtype, M, cols, seed):
    """rows [0, M) x columns [0, cols) of `buf` viewed as `dtype` from a seeded CPU generator; the rest NaN."""
    v = buf.view(dtype)
    v.fill_(float("nan"))
    v[:M, :cols] = torch.randn(M, cols, generator=g(seed)).to(dtype).to(DEV)
    return v


# (kernel the launch takes at these shapes, N, M below the line, M above it):
#   "256s"       whole 256-row tiles and N % 256 == 0 -> gemm_nt256s_kernel (one wave per SIMD)
#   "8wave"      ragged N, 255 row tiles x 2 column tiles -> gemm_nt256_kernel (one block per tile)
#   "persistent" ragged N, >= 4 tiles per CU -> gemm_nt256p_kernel
# Above the line the first chunk (65,280 rows) takes the same kernel; the short last chunk takes the 128-row tiles.
NT_SHAPES = {"256s": (256, LINE - 256, LINE + 256), "8wave": (264, LINE - 356, LINE + 100),
             "persistent": (1288, LINE - 356, LINE + 100)}


def _chunks(M, row_bytes, align):
    from unsloth_amd.kernels import utils as U
    if M * row_bytes < U.GEMM_SPAN_LIMIT:
        return [(0, M)]
    step = U._chunk_rows(row_bytes, align)
    return [(r0, min(step, M - r0)) for r0 in range(0, M, step)]


def _count_calls(monkeypatch, name):
    """Wrap the library entry point `name`; returns the list its calls' M (NT / NN) or K (TN) land in."""
    from unsloth_amd import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    seen = []

    def wrapped(A, lda, M, K, *rest):
        seen.append(K if name == "uamd_gemm_tn_256" else M)
        return fn(A, lda, M, K, *rest)
    monkeypatch.setattr(L, name, wrapped)
    return seen


def _run_nt_nn(A, M, N, nn, rank, accumulate, dtype, seed):
    """C (+)= A[:, :K_MAIN] @ B (+ A[:, K_MAIN:K_MAIN+64] @ BK) through utils._launch_gemm. Returns (C, fp32 want, B, BK, C0)."""
    from unsloth_amd.kernels import utils as U
    Bw = (torch.randn((K_MAIN, N) if nn else (N, K_MAIN), generator=g(seed)) * 0.05).to(dtype).to(DEV)
    bk = (torch.randn((RK, N) if nn else (N, RK), generator=g(seed + 1)) * 0.05).to(dtype).to(DEV) if rank else None
    C0 = torch.randn(M, N, generator=g(seed + 2)).to(dtype).to(DEV) if accumulate else None
    C = C0.clone() if accumulate else torch.empty(M, N, dtype=dtype, device=DEV)
    Am, xk = A[:M, :K_MAIN], (A[:M, K_MAIN:K_MAIN + RK] if rank else None)
    old = U.GEMM256_MODE
    U.GEMM256_MODE = "on"
    try:
        U._launch_gemm(Am, [U._group(Bw, C, N, Bw.stride(0), xk=xk, bk=bk)], nf4=False, accumulate=accumulate, nn=nn)
    finally:
        U.GEMM256_MODE = old
    want = Am.float() @ (Bw.float() if nn else Bw.float().t())
    if rank:
        want += xk.float() @ (bk.float() if nn else bk.float().t())
    if accumulate:
        want += C0.float()
    return C, want, Bw, bk, C0


def _check_rows64(C, A, Bw, bk, C0, nn, dtype, what):
    """fp64 on the CPU for the sampled rows (first / last, tile edges, the 2^31 / 2^32 byte crossings of A)."""
    M = C.shape[0]
    rows = _sample_rows(M, LDA * 2)
    a = A[rows.to(DEV)].cpu().double()
    want = a[:, :K_MAIN] @ (Bw.cpu().double() if nn else Bw.cpu().double().t())
    if bk is not None:
        want += a[:, K_MAIN:K_MAIN + RK] @ (bk.cpu().double() if nn else bk.cpu().double().t())
    if C0 is not None:
        want += C0[rows.to(DEV)].cpu().double()
    assert_ulp(C[rows.to(DEV)], want, dtype, ulps=1, atol=_gemm_atol(want, dtype, K_MAIN + RK), what=what + " fp64 rows")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("form", ["nt:256s", "nt:8wave", "nt:persistent", "nn"])
def test_gemm_across_the_4gib_span(padded, monkeypatch, form, side, dtype):
    """A of row stride 32,768 elements: M = 65,536 rows span 4 GiB. Below the line one launch; above it the row chunks
    utils._launch_gemm issues (multiples of 256 rows). Every combination of rank block and accumulate, the whole output
    against the fp32 product, sampled rows against fp64."""
    kind = form.split(":")[-1]
    N, m_below, m_above = NT_SHAPES["8wave" if kind == "nn" else kind]
    M = m_below if side == "below" else m_above
    nn = form == "nn"
    A = _fill(padded, dtype, M, K_MAIN + RK, seed=300)
    calls = _count_calls(monkeypatch, "uamd_gemm_nn_256" if nn else "uamd_gemm_nt_256")
    # below: one launch; above: the most whole 256-row tiles below 4 GiB of 64 KiB rows (65,280), then the rest
    expect = [M] if side == "below" else [65280, M - 65280]
    for rank in (False, True):
        for accumulate in (False, True):
            what = f"{form} {side} M={M} N={N} rank={rank} acc={accumulate} {dtype}"
            calls.clear()
            C, want, Bw, bk, C0 = _run_nt_nn(A, M, N, nn, rank, accumulate, dtype, seed=310)
            assert calls == expect, (what, calls)
            _check_gemm(C, want, dtype, K_MAIN + RK * rank, what)
            _check_rows64(C, A[:M], Bw, bk, C0, nn, dtype, what)
            del C, want, C0


def _tn_bound_extra(dY, X, C0, spans, dtype):
    """one more rounding of the 16-bit output per extra chunk: eps * |partial sum after chunk k| for every chunk but the last
    (the existing ulp rule's margin: 1 ulp per 0.5-ulp rounding)."""
    part = C0.double() if C0 is not None else 0.0
    extra = 0.0
    for t0, rows in spans[:-1]:
        part = part + dY[t0:t0 + rows].double().t() @ X[t0:t0 + rows].double()
        extra = extra + EPS[dtype] * part.abs()
    return extra


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("side", ["below", "above"])
def test_gemm_tn_across_the_4gib_span(padded, monkeypatch, side, dtype):
    """dense_dw (uamd_gemm_tn_256): dW[256, 256] (+)= dY^T X with dY of row stride 32,768 elements, T tokens just below /
    above 65,536. Above, the tokens go in chunks (multiples of 64) with accumulate on after the first; the bound against fp64
    is _check_gemm's plus one rounding per extra chunk."""
    from unsloth_amd.kernels.utils import dense_dw
    T = (LINE - 64) if side == "below" else (LINE + 64)
    N_out, N_in = 256, 256
    dYb = _fill(padded, dtype, T, N_out, seed=320)
    dY = dYb[:T, :N_out]
    X = torch.randn(T, N_in, generator=g(321)).to(dtype).to(DEV)
    spans = _chunks(T, LDA * 2, 64)
    # below: one launch; above: the most 64-token steps below 4 GiB of 64 KiB rows (65,472), then the rest (128)
    assert [rows for _, rows in spans] == ([T] if side == "below" else [65472, 128])
    calls = _count_calls(monkeypatch, "uamd_gemm_tn_256")
    for accumulate in (False, True):
        what = f"tn {side} T={T} acc={accumulate} {dtype}"
        C0 = torch.randn(N_out, N_in, generator=g(322)).to(dtype).to(DEV) if accumulate else None
        out = C0.clone() if accumulate else None
        calls.clear()
        got = dense_dw(dY, X, out=out, accumulate=accumulate)
        assert calls == [rows for _, rows in spans], (what, calls)
        want32 = dY.float().t() @ X.float() + (C0.float() if accumulate else 0)
        want64 = dY.double().t() @ X.double() + (C0.double() if accumulate else 0)
        extra = _tn_bound_extra(dY, X, C0, spans, dtype)
        atol = _gemm_atol(want64, dtype, T) + extra
        _ulp_gpu(got, want64, dtype, ulps=1, atol=atol, allow_frac=1e-3, what=what + " fp64")
        _ulp_gpu(got, want32, dtype, ulps=1, atol=atol, allow_frac=1e-3, what=what + " fp32")


# ------------------------------------------------------------------------------------------------ chunking below the line
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("form,M,N,K,ch", [("nt", 16384, 4096, 512, 4096),   # whole tiles: the 256s kernel, whole and chunked
                                           ("nt", 16484, 4104, 512, 4096),   # persistent walk whole; 8-wave / 128-row chunks
                                           ("nt", 3000, 264, 320, 1024),     # 128-row tiles, ragged M and N
                                           ("nn", 16484, 4104, 512, 4096), ("nn", 3000, 264, 320, 1024)])
def test_forced_chunks_equal_one_launch(monkeypatch, form, M, N, K, ch, dtype):
    """GEMM_SPAN_LIMIT lowered so that the launch goes in `ch`-row chunks: one output tile's accumulation order does not
    depend on which rows share its launch, so the chunked result equals the single launch bit for bit -- with and without a
    rank block, with and without accumulate. At the shipped limit the same shape is exactly one library call."""
    from unsloth_amd.kernels import utils as U
    nn = form == "nn"
    ld = K + 64 + 8                                  # A and the rank block side by side in padded rows
    A = torch.randn(M, ld, generator=g(400)).to(dtype).to(DEV)
    calls = _count_calls(monkeypatch, "uamd_gemm_nn_256" if nn else "uamd_gemm_nt_256")
    Bw = (torch.randn((K, N) if nn else (N, K), generator=g(401)) * 0.05).to(dtype).to(DEV)
    bk = (torch.randn((64, N) if nn else (N, 64), generator=g(402)) * 0.05).to(dtype).to(DEV)
    C0 = torch.randn(M, N, generator=g(403)).to(dtype).to(DEV)
    item = A.element_size()

    def run(accumulate, rank):
        C = C0.clone()
        old = U.GEMM256_MODE
        U.GEMM256_MODE = "on"
        try:
            U._launch_gemm(A[:, :K], [U._group(Bw, C, N, Bw.stride(0), xk=A[:, K:K + 64] if rank else None,
                                               bk=bk if rank else None)], nf4=False, accumulate=accumulate, nn=nn)
        finally:
            U.GEMM256_MODE = old
        return C

    for rank in (False, True):
        for accumulate in (False, True):
            calls.clear()
            one = run(accumulate, rank)
            assert calls == [M]
            monkeypatch.setattr(U, "GEMM_SPAN_LIMIT", ld * item * ch + 1)
            calls.clear()
            chunked = run(accumulate, rank)
            monkeypatch.setattr(U, "GEMM_SPAN_LIMIT", 1 << 32)
            assert calls == [min(ch, M - r0) for r0 in range(0, M, ch)], calls
            assert torch.equal(one, chunked), (rank, accumulate, float((one.float() - chunked.float()).abs().max()))
            want = A[:, :K].float() @ (Bw.float() if nn else Bw.float().t())
            if rank:
                want += A[:, K:K + 64].float() @ (bk.float() if nn else bk.float().t())
            if accumulate:
                want += C0.float()
            _check_gemm(chunked, want, dtype, K + 64 * rank, f"{form} {M}x{N}x{K} chunked rank={rank} acc={accumulate}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_forced_tn_chunks_match_fp64(monkeypatch, dtype):
    """dense_dw with the limit lowered to 1,024-token chunks (5 launches, accumulate on after the first) against fp64, within
    _check_gemm's bound plus one rounding per extra chunk; one launch at the shipped limit."""
    from unsloth_amd.kernels import utils as U
    from unsloth_amd.kernels.utils import dense_dw
    T, N_out, N_in = 4160, 384, 520
    dY = torch.randn(T, N_out, generator=g(410)).to(dtype).to(DEV)
    X = torch.randn(T, N_in, generator=g(411)).to(dtype).to(DEV)
    calls = _count_calls(monkeypatch, "uamd_gemm_tn_256")
    one = dense_dw(dY, X)
    assert calls == [T]
    row_bytes = max(N_out, N_in) * dY.element_size()
    monkeypatch.setattr(U, "GEMM_SPAN_LIMIT", row_bytes * 1024 + 1)
    spans = _chunks(T, row_bytes, 64)
    calls.clear()
    got = dense_dw(dY, X)
    assert calls == [rows for _, rows in spans] and len(spans) == 5, calls
    want64 = dY.double().t() @ X.double()
    atol = _gemm_atol(want64, dtype, T) + _tn_bound_extra(dY, X, None, spans, dtype)
    _ulp_gpu(got, want64, dtype, ulps=1, atol=atol, allow_frac=1e-3, what=f"tn chunked {dtype}")
    _ulp_gpu(one, want64, dtype, ulps=1, atol=_gemm_atol(want64, dtype, T), allow_frac=1e-3, what=f"tn one launch {dtype}")


# ------------------------------------------------------------------------------------------------ LoRA MLP past the line
def _nf4_proj(out_f, in_f, r, seed):
    from unsloth_amd.nf4 import quantize_nf4
    W = (torch.randn(out_f, in_f, generator=g(seed)) * 0.03).to(torch.bfloat16)
    A = torch.randn(r, in_f, generator=g(seed + 1)) * 0.05
    B = torch.randn(out_f, r, generator=g(seed + 2)) * 0.05
    packed, qs = quantize_nf4(W.to(DEV), compress_statistics=True)
    Wd = R.nf4_dequantize_state(packed, qs)                     # what the GPU path multiplies by (CPU oracle)
    return dict(Wd=Wd.to(DEV), dev=(packed, qs), A=A.to(DEV).requires_grad_(True), B=B.to(DEV).requires_grad_(True), s=2.0)


def _lin(x, p):
    return x @ p["Wd"].float().t() + p["s"] * (x @ p["A"].detach().t()) @ p["B"].detach().t()


def _mlp_reference(X, dY, gate, up, down, chunk=8192):
    """fp32 on the GPU, in row blocks: the forward with the reference's rounding points (oracle matmul_lora / glu_forward,
    what test_lora_mlp compares the output with) and the fp32 gradients (oracle lora_mlp_reference_grads' math, written out:
    X and all six LoRA factors)."""
    M = X.shape[0]
    out = torch.empty(M, down["Wd"].shape[0], dtype=torch.float32, device=DEV)
    dX = torch.empty(X.shape, dtype=torch.float32, device=DEV)
    gr = {k: torch.zeros_like(p[w], dtype=torch.float32) for k, p, w in
          (("gA", gate, "A"), ("gB", gate, "B"), ("uA", up, "A"), ("uB", up, "B"), ("dA", down, "A"), ("dB", down, "B"))}
    cpu = lambda p: (p["Wd"], p["A"].detach(), p["B"].detach(), p["s"])
    for r0 in range(0, M, chunk):
        xb = X[r0:r0 + chunk]
        e16, g16 = R.matmul_lora(xb, *cpu(gate)), R.matmul_lora(xb, *cpu(up))
        out[r0:r0 + chunk] = R.matmul_lora(R.glu_forward(e16, g16, "swiglu"), *cpu(down)).float()
        del e16, g16
        x = xb.float()
        e, gg = _lin(x, gate), _lin(x, up)
        sig = torch.sigmoid(e)
        f = e * sig
        h = f * gg
        dy = dY[r0:r0 + chunk].float()
        s = down["s"]
        dyB = dy @ down["B"].detach()
        dh = dy @ down["Wd"].float() + s * dyB @ down["A"].detach()
        gr["dA"] += s * dyB.t() @ h
        gr["dB"] += s * dy.t() @ (h @ down["A"].detach().t())
        dg = dh * f
        de = dh * gg * sig * (1.0 + e * (1.0 - sig))
        del e, gg, f, h, dh, sig
        dgB, deB = dg @ up["B"].detach(), de @ gate["B"].detach()
        gr["uA"] += up["s"] * dgB.t() @ x
        gr["uB"] += up["s"] * dg.t() @ (x @ up["A"].detach().t())
        gr["gA"] += gate["s"] * deB.t() @ x
        gr["gB"] += gate["s"] * de.t() @ (x @ gate["A"].detach().t())
        dX[r0:r0 + chunk] = (dg @ up["Wd"].float() + up["s"] * dgB @ up["A"].detach()
                             + de @ gate["Wd"].float() + gate["s"] * deB @ gate["A"].detach())
    return out, dX, gr


def _mlp_rows64(X, rows, gate, up, down):
    """fp64 on the CPU for sampled rows, with the reference's rounding points (bf16 after each matmul_lora and in the GLU)."""
    bf = torch.bfloat16
    rd = lambda t: t.to(bf).double()

    def ml(x, p):
        W, A, B = p["Wd"].cpu().double(), rd(p["A"].detach().cpu()), rd(p["B"].detach().cpu())
        return rd(rd(x @ W.t()) + p["s"] * (rd(x @ A.t()) @ B.t()))
    x = X[rows.to(DEV)].cpu().double()
    e, gg = ml(x, gate), ml(x, up)
    h = rd(rd(e * torch.sigmoid(e)) * gg)
    return ml(h, down)


@pytest.mark.parametrize("H,I,M", [(3584, 18944, 57344),          # Qwen2-7B widths: h spans 4.35 GB (line at 56,585 tokens)
                                   (4096, 14336, 81920)],         # Llama-3-8B widths: 4.71 GB (line at 74,732 tokens)
                         ids=["qwen2_7b", "llama3_8b"])
def test_lora_mlp_past_the_4gib_line(H, I, M):
    """LoRA_MLP forward + backward (NF4 weights, r = 16, SwiGLU, the fused activation kernels) at a token count where the
    down projection's A operand h -- and the merged dX's [df | de] -- have row stride 2 I + 64 and span more than 4 GiB:
    output, dX and the six LoRA gradients against fp32 at test_lora_mlp's bounds, sampled output rows against fp64."""
    _need(48)
    import unsloth_amd.kernels as K
    from unsloth_amd.kernels.fast_lora import LoRA_MLP
    from unsloth_amd.kernels import utils as U
    r = 16
    gate, up, down = _nf4_proj(I, H, r, 500), _nf4_proj(I, H, r, 510), _nf4_proj(H, I, r, 520)
    X = (torch.randn(M, H, generator=g(530)) * 0.5).to(torch.bfloat16).to(DEV)
    dY = torch.randn(M, H, generator=g(531)).to(torch.bfloat16).to(DEV)
    assert M * (2 * I + U.ROW_PAD) * 2 >= 1 << 32                       # the shape is past the line
    Xg = X.clone().requires_grad_(True)
    out = LoRA_MLP.apply(Xg * 1.0, gate["dev"][0], gate["dev"][1], gate["A"], gate["B"], gate["s"],
                         up["dev"][0], up["dev"][1], up["A"], up["B"], up["s"],
                         down["dev"][0], down["dev"][1], down["A"], down["B"], down["s"],
                         K.swiglu_fg_kernel, K.swiglu_DWf_DW_dfg_kernel, True)
    out.backward(dY)
    torch.cuda.synchronize()
    got = [Xg.grad, gate["A"].grad, gate["B"].grad, up["A"].grad, up["B"].grad, down["A"].grad, down["B"].grad]
    del Xg
    torch.cuda.empty_cache()
    want_out, want_dX, gr = _mlp_reference(X, dY, gate, up, down)
    assert torch.isfinite(out).all()
    rel = _rel_fro(out, want_out)
    assert rel < 6e-3, ("out", rel)
    del want_out
    names = ["dX", "d_gateA", "d_gateB", "d_upA", "d_upB", "d_downA", "d_downB"]
    wants = [want_dX, gr["gA"], gr["gB"], gr["uA"], gr["uB"], gr["dA"], gr["dB"]]
    for nm, a, b in zip(names, got, wants):
        assert a is not None, nm
        assert a.dtype == (torch.bfloat16 if nm == "dX" else torch.float32), nm
        rel = _rel_fro(a, b)
        assert rel < 2e-2, (nm, rel)
    rows = _sample_rows(M, (2 * I + U.ROW_PAD) * 2)
    want64 = _mlp_rows64(X, rows, gate, up, down)
    rel = float((out.detach()[rows.to(DEV)].cpu().double() - want64).norm() / want64.norm())
    assert rel < 6e-3, ("out fp64 rows", rel)


# ------------------------------------------------------------------------------------------------ row-indexed kernels past 2^31 elements
# Inputs of billions of elements come from a device generator with a fixed seed (a CPU generator would take tens of seconds
# per tensor); the references are the oracle's functions (fp32 with the reference's rounding points) applied on the GPU in
# row blocks, at test_gpu_elementwise's tolerances, and fp64 on the CPU for sampled rows.
def dg(seed):
    return torch.Generator(DEV).manual_seed(seed)


def test_cross_entropy_past_2g_elements():
    """uamd_cross_entropy_forward / _backward (in place) on 16,768 x 128,256 bf16 logits (2.15e9 elements, 4.3 GB: row
    offsets past 2^31 elements and 2^32 bytes)."""
    _need(20)
    from unsloth_amd.kernels.cross_entropy_loss import _ce_backward_, _ce_forward
    rows, V = 16768, 128256
    dtype = torch.bfloat16
    logits = (torch.randn(rows, V, generator=dg(600), device=DEV) * 4).to(dtype)
    labels = torch.randint(0, V, (rows,), generator=dg(601), device=DEV)
    labels[3] = -100
    labels[-1] = V - 1
    labels[-2] = 0
    dl = torch.rand(rows, generator=dg(602), device=DEV)
    losses, lse = _ce_forward(logits, labels, 0, 0)
    want_grad = torch.empty_like(logits)
    blk = 2048
    for r0 in range(0, rows, blk):
        lo, ls = R.cross_entropy_forward(logits[r0:r0 + blk], labels[r0:r0 + blk])
        torch.testing.assert_close(losses[r0:r0 + blk], lo, rtol=2e-5, atol=2e-5)
        want_grad[r0:r0 + blk] = R.cross_entropy_backward(logits[r0:r0 + blk], dl[r0:r0 + blk], ls, labels[r0:r0 + blk])
    assert losses[3].item() == 0.0
    sample = _sample_rows(rows, V * 2)
    x = logits[sample.to(DEV)].cpu().double()
    lse64 = torch.logsumexp(x, dim=1)
    lab = labels[sample.to(DEV)].cpu()
    loss64 = torch.where(lab != -100, lse64 - x.gather(1, lab.clamp(min=0)[:, None])[:, 0], torch.zeros_like(lse64))
    torch.testing.assert_close(losses[sample.to(DEV)].cpu().double(), loss64, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(lse[sample.to(DEV)].cpu().double(), lse64, rtol=2e-5, atol=2e-5)
    _ce_backward_(logits, dl, lse, labels, 0, 0)
    for r0 in range(0, rows, blk):
        _ulp_gpu(logits[r0:r0 + blk], want_grad[r0:r0 + blk], dtype, ulps=2, atol=1e-6, allow_frac=5e-3,
                 what=f"ce bwd rows {r0}+")
    assert torch.all(logits[3] == 0), "ignored row must have an exactly zero gradient"


def test_rms_norm_and_fused_add_past_2g_elements():
    """RMSNorm forward + in-place backward at 262,144 x 8,192 bf16 and the fused add form's forward at 524,288 x 4,096 (2.15e9
    elements per operand): Y, r, dX (and H) against the oracle in row blocks; r against fp64 on sampled rows."""
    _need(40)
    from unsloth_amd.kernels.rms_layernorm import add_rms_fwd, add_rms_supported, rms_bwd_, rms_fwd
    rows, dim, eps = 262144, 8192, 1e-5
    dtype = torch.bfloat16
    X = torch.randn(rows, dim, generator=dg(610), device=DEV).to(dtype)
    W = torch.rand(dim, generator=g(611)).to(dtype).to(DEV)
    blk = 16384
    Y, r = rms_fwd(X, W, eps)
    for r0 in range(0, rows, blk):
        Yo, ro = R.rms_layernorm_forward(X[r0:r0 + blk], W, eps)
        _ulp_gpu(Y[r0:r0 + blk], Yo, dtype, ulps=1, allow_frac=2e-3, what=f"rms fwd rows {r0}+")
        torch.testing.assert_close(r[r0:r0 + blk], ro, rtol=1e-5, atol=0)
    sample = _sample_rows(rows, dim * 2)
    x = X[sample.to(DEV)].cpu().double()
    r64 = torch.rsqrt((x * x).mean(dim=1) + eps)
    torch.testing.assert_close(r[sample.to(DEV)].cpu().double(), r64, rtol=1e-5, atol=0)
    del Y
    dY = torch.randn(rows, dim, generator=dg(612), device=DEV).to(dtype)
    want = torch.empty_like(dY)
    for r0 in range(0, rows, blk):
        want[r0:r0 + blk] = R.rms_layernorm_backward(dY[r0:r0 + blk], X[r0:r0 + blk], W, r[r0:r0 + blk])
    ptr = dY.data_ptr()
    dX = rms_bwd_(dY, X, W, r)
    assert dX.data_ptr() == ptr
    for r0 in range(0, rows, blk):
        _ulp_gpu(dX[r0:r0 + blk], want[r0:r0 + blk], dtype, ulps=2, allow_frac=2e-3, what=f"rms bwd rows {r0}+")
    del dY, dX, want, r
    torch.cuda.empty_cache()
    # the fused add kernel takes rows of up to 4,096 bf16 (add_rms_supported; wider rows take torch add + rms_fwd): the same
    # 2.15e9 elements as 524,288 x 4,096
    X = X.view(2 * rows, dim // 2)
    W = W[: dim // 2].contiguous()
    assert add_rms_supported(X, W)
    Res = torch.randn(2 * rows, dim // 2, generator=dg(613), device=DEV).to(dtype)
    H, Y, r = add_rms_fwd(X, Res, W, eps)
    for r0 in range(0, 2 * rows, blk):
        assert torch.equal(H[r0:r0 + blk], X[r0:r0 + blk] + Res[r0:r0 + blk]), f"add rms H rows {r0}+"
        Yo, ro = R.rms_layernorm_forward(H[r0:r0 + blk], W, eps)
        _ulp_gpu(Y[r0:r0 + blk], Yo, dtype, ulps=1, allow_frac=2e-3, what=f"add rms fwd rows {r0}+")
        torch.testing.assert_close(r[r0:r0 + blk], ro, rtol=1e-5, atol=0)


def test_rope_indexed_positions_to_131071():
    """rope_embedding_qk with int32 position indices over a 131,072-token row (a permutation: every position up to 131,071,
    in scattered order), Llama-3-8B heads (32 / 8 x 128), the bf16 table from models.llama.RopeTables: bit-exact against the
    oracle, as test_rope_qk_indexed_and_dense asserts at 50 tokens."""
    _need(24)
    from transformers import LlamaConfig
    from unsloth_amd.kernels.rope_embedding import fast_rope_embedding
    from unsloth_amd.models.llama import RopeTables
    T, Hq, Hk, D = 131072, 32, 8, 128
    dtype = torch.bfloat16
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hk, head_dim=D,
                      max_position_embeddings=T, rope_parameters={"rope_type": "default", "rope_theta": 5e5})
    cos, sin = RopeTables(cfg).get(T, DEV, dtype)
    assert cos.shape[0] >= T
    idx = ((torch.arange(T, dtype=torch.int64) * 7919) % T).to(torch.int32).to(DEV)
    assert int(idx.max()) == T - 1
    Q = torch.randn(1, T, Hq, D, generator=dg(620), device=DEV).to(dtype)
    K = torch.randn(1, T, Hk, D, generator=dg(621), device=DEV).to(dtype)
    Qv, Kv = Q.transpose(1, 2), K.transpose(1, 2)
    Qo, Ko = R.rope_embedding_qk(Qv, Kv, cos, sin, idx)
    Qr, Kr = fast_rope_embedding(Qv, Kv, cos, sin, idx)
    assert Qr.data_ptr() == Q.data_ptr()
    assert torch.equal(Qr.float(), Qo), "rope Q"
    assert torch.equal(Kr.float(), Ko), "rope K"
