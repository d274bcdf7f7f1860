"""-m gpu: the MFMA GEMM family (csrc/gemm.hip, csrc/gemm256.hip) and the LoRA side kernels (csrc/lora_side.hip, lora_xa in
csrc/gemm.hip) on the operands production hands them: row strides wider than the row, column blocks of a wider buffer, base
pointers off the 16-byte grid, an odd `ldc`. tests/test_gpu_views.py does the same for the row-wise kernels.

Every operand is a view into a 1-D pool of its own dtype (`place`) with at least 256 rows' worth + 256 elements of margin on
either side, so that a tile-granular over-read stays inside the allocation and lands in the fill:
  * around an INPUT (A, B, XK, BK, bias, fp32 XA / P, Z, absmax) every pool element is NaN -- row padding, the rows in front and
    behind, the neighbouring column blocks -- so a load that takes padding into a contraction poisons the result. (Packed NF4
    bytes have no NaN: their pool is 0xFF, which decodes to +-absmax and moves the result far outside the bound.) Padding an
    operand DOCUMENTS as zero (XK's columns past the rank, BK's unused rank columns) is part of the view and zero;
  * around an OUTPUT or accumulate target every element is a sentinel whose BITS must survive; inside, an overwritten output
    starts as NaN, so an element the kernel never wrote shows up.
Results are checked against an fp64 CPU product of the same rounded inputs at the bound of the aligned-data test of the same
kernel (tests/test_gpu_nf4_gemm.py `_check_gemm`, test_lora_linear_dx_accumulates_groups, test_lora_xa, test_lora_tn_matches_fp64;
tests/test_gpu_full_finetune.py test_dense_dw_matches_torch), and -- where the view does not change which kernel runs -- bit for
bit against the same launch on contiguous copies. A call recorder (`calls`) asserts that the launch went to the entry point the
case names with the views' own pointers and strides: nothing was copied to a contiguous buffer on the way.

C layouts (elements; `store_c4` in csrc/common.h picks the 8-byte vector form by `ldc % 4 == 0` and an 8-byte aligned C, and
`whole_tiles()` in csrc/gemm256.hip keeps a launch on gemm_nt256s_kernel only with `ldc % 8 == 0` and a 16-byte aligned C):
    plain       ldc = N        offset 0      control
    pad8_off8   ldc = N + 8    offset 8      vector stores, 16-byte aligned
    rowpad64    ldc = N + 64   offset 0      utils.ROW_PAD
    pad4_off4   ldc = N + 4    offset 4      vector stores, 8-byte aligned only
    odd_ld      ldc = N + 1    offset 0      scalar epilogue through `ldc % 4`
    off1        ldc = N        offset 1      scalar epilogue through the pointer
A, B, XK, BK must be 16-byte aligned with `ld % 8 == 0` (the C entry points answer UAMD_ERR_ALIGN otherwise): they go along as
(ld + 8, offset 8) or (ld + 64, offset 0); what the Python wrappers do with operands outside that contract is the last section.
"""
import contextlib
import ctypes

import pytest
import torch

from oracle import ref_ops as R
from tests._util import assert_ulp, rel_fro
from tests.test_gpu_nf4_gemm import _check_gemm
from tests.test_gpu_views import SENTINEL, assert_unchanged, bits, g

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAN = float("nan")
MARGIN = 256                                    # rows' worth and elements of pool on either side of a view: one full tile
C_LAYOUTS = {"plain": (0, 0), "pad8_off8": (8, 8), "rowpad64": (64, 0), "pad4_off4": (4, 4), "odd_ld": (1, 0), "off1": (0, 1)}
IN_LAYOUTS = {"plain": (0, 0), "rowpad64": (64, 0)}            # every other C layout goes with inputs at (ld + 8, offset 8)
KNOB_DEFAULTS = {6: 1, 7: 1, 9: 1, 11: 1}      # UAMD_TUNE_GEMM_HALF, _PERSIST, _PLAIN, _S
GEMM_ENTRIES = ("uamd_gemm_nt", "uamd_gemm_nt_nf4", "uamd_gemm_nt_256", "uamd_gemm_nn_256", "uamd_gemm_tn_256")
SIDE_ENTRIES = ("uamd_lora_xa", "uamd_lora_xa2", "uamd_lora_xa2k", "uamd_lora_tn")


def place(data, ld, off, fill):
    """(pool, view): `data` [rows, cols] (CPU) as a view of row stride `ld`, `off` elements past a 16-byte aligned position of
    a fresh 1-D device pool that is `fill` everywhere else, MARGIN rows' worth + MARGIN elements in front and behind."""
    rows, cols = data.shape
    assert ld >= cols and off >= 0
    lead = -(-(MARGIN * ld + MARGIN) // 64) * 64
    pool = torch.full((2 * lead + off + rows * ld,), fill, dtype=data.dtype, device=DEV)
    assert pool.data_ptr() % 16 == 0
    view = pool.as_strided((rows, cols), (ld, 1), lead + off)
    view.copy_(data)
    assert (view.data_ptr() % 16 == 0) == ((off * data.element_size()) % 16 == 0)
    return pool, view


def assert_guard(pool, views, before, what):
    """Every pool element outside `views` holds the bits it held in `before`."""
    m = torch.ones(pool.numel(), dtype=torch.bool, device=pool.device)
    for v in views:
        m.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(False)
    assert int(m.sum()) == pool.numel() - sum(v.numel() for v in views)
    assert torch.equal(bits(pool)[m], bits(before)[m]), f"{what}: the kernel wrote outside its view"


@contextlib.contextmanager
def gemm_mode(mode, **knobs):
    """utils.GEMM256_MODE and the library's tuning knobs (k6=.., k7=..) for one block; both restored."""
    from unsloth_amd import _lib
    from unsloth_amd.kernels import utils as U
    L = _lib.lib()
    old = U.GEMM256_MODE
    U.GEMM256_MODE = mode
    try:
        for k, v in knobs.items():
            assert L.uamd_set_tuning(int(k[1:]), v) == 0
        yield
    finally:
        U.GEMM256_MODE = old
        for k, v in KNOB_DEFAULTS.items():
            L.uamd_set_tuning(k, v)


@pytest.fixture
def calls(monkeypatch):
    """[(entry point, its arguments)] of every GEMM / side-kernel launch, in order."""
    from unsloth_amd import _lib
    L = _lib.lib()
    seen = []
    for name in GEMM_ENTRIES + SIDE_ENTRIES:
        def wrapped(*a, _fn=getattr(L, name), _name=name):
            seen.append((_name, a))
            return _fn(*a)
        monkeypatch.setattr(L, name, wrapped)
    return seen


def _addr(p):
    return p.value if isinstance(p, ctypes.c_void_p) else int(p)


def assert_launch(calls, name, A, pairs):
    """The GEMM launches recorded are exactly one of `name`, with A and every group's (B, C) read and written in place."""
    got = [c for c in calls if c[0] in GEMM_ENTRIES]
    assert [c[0] for c in got] == [name], [c[0] for c in got]
    a = got[0][1]
    assert _addr(a[0]) == A.data_ptr() and a[1] == A.stride(0), "A was copied"
    assert a[5] == len(pairs)
    for i, (B, C) in enumerate(pairs):
        assert a[4][i].B == B.data_ptr() and a[4][i].C == C.data_ptr() and a[4][i].ldc == C.stride(0), f"group {i} was copied"


def fresh(t):
    """A contiguous copy in an allocation of its own (16-byte aligned)."""
    return t.clone(memory_format=torch.contiguous_format)


def in_layout(lay):
    return IN_LAYOUTS.get(lay, (8, 8))


def sample_rows(M, tile=256):
    """First and last row of the first and of the last row tile, and a few in between."""
    last = (M - 1) // tile * tile
    return sorted({0, min(tile - 1, M - 1), last, M - 1, M // 3, M // 2 + 1})


# ------------------------------------------------------------------------------------------------ NT / NN through _launch_gemm
def run_gemm(calls, entry, dtype, M, Ns, K, lay, *, nn=False, accumulate=False, rank=0, bias=None, prologue=(), zero_cols=0,
             sampled=False, same_kernel=True, seed=11):
    """One utils._launch_gemm over `len(Ns)` groups whose C are the column blocks of ONE [M, sum Ns] buffer in layout `lay`
    (+ `zero_cols` zeroed padding columns that must stay zero). rank: live columns of a 64-wide rank block (XK zero past them,
    BK zero in the unused rank columns / rows); prologue: per group the rank R_g of a register-prologue LoRA term (fp32 XA
    with a padded `ld_xa`, LB with a padded `ld_lb`; the 128-tile kernel only); bias: None | "aligned" | "odd"."""
    from unsloth_amd.kernels.utils import _group, _launch_gemm
    gen = g(seed)
    ie, io = in_layout(lay)
    ce, co = C_LAYOUTS[lay]
    what = f"{entry} {M}x{Ns}x{K} {lay} {dtype} nn={nn} acc={accumulate} rank={rank} bias={bias}"
    A = torch.randn(M, K, generator=gen).to(dtype)
    Ntot = sum(Ns)
    C0 = torch.randn(M, Ntot, generator=gen).to(dtype) if accumulate else torch.full((M, Ntot), NAN, dtype=dtype)
    xk = None
    if rank:
        xk = torch.zeros(M, 64, dtype=dtype)
        xk[:, :rank] = torch.randn(M, rank, generator=gen).to(dtype)
    xa = None
    if prologue:
        xa = torch.randn(M, sum(prologue), generator=gen)                     # fp32, rounded to `dtype` by the kernel
    inputs = []                                                                 # [(pool, snapshot)]

    def put(data, ld, off, fill=NAN):
        pool, view = place(data, ld, off, fill)
        inputs.append((pool, pool.clone()))
        return view

    # a [K, N] operand of the NN form is a column block of a wider buffer: 136 + offset columns in front, more behind
    wide = (lambda t: put(t, t.shape[1] + 264 + ie, 136 + io)) if (ie or io) else (lambda t: put(t, t.shape[1], 0))
    rowp = lambda t: put(t, t.shape[1] + ie, io)
    Av = rowp(A)
    xkv = rowp(xk) if rank else None
    xav = put(xa, xa.shape[1] + 4, 4) if prologue else None                    # ld_xa % 4 == 0, 16-byte aligned fp32
    cpool, Cv = place(C0, Ntot + zero_cols + ce, co, SENTINEL)
    if zero_cols:
        cpool.as_strided((M, zero_cols), (Cv.stride(0), 1), Cv.storage_offset() + Ntot).zero_()
    cbefore = cpool.clone()
    host, dev, col, xcol = [], [], 0, 0
    for gi, N in enumerate(Ns):
        B = (torch.randn((K, N) if nn else (N, K), generator=gen) * 0.05).to(dtype)
        h = dict(B=B, cols=(col, col + N))
        d = dict(B=wide(B) if nn else rowp(B), C=Cv[:, col:col + N])
        if rank:
            bk = torch.zeros((64, N) if nn else (N, 64), dtype=dtype)
            blk = (torch.randn(rank, N, generator=gen) * 0.05).to(dtype)
            if nn:
                bk[:rank] = blk
            else:
                bk[:, :rank] = blk.t()
            h["bk"] = bk
            d["bk"] = wide(bk) if nn else rowp(bk)
        if prologue:
            r = prologue[gi]
            lb = (torch.randn(N, r, generator=gen) * 0.05).to(dtype)
            h.update(lb=lb, xa=(xcol, xcol + r), scale=0.5 + gi)
            d["lb"] = put(lb, r + 8, 8)
            xcol += r
        if bias:
            b = (torch.randn(N, generator=gen) * 2.0).to(dtype)
            h["bias"] = b
            d["bias"] = put(b.view(1, N), N, 1 if bias == "odd" else 0)[0]
            assert (d["bias"].data_ptr() % 8 != 0) == (bias == "odd")
        host.append(h)
        dev.append(d)
        col += N

    def launch(Ad, xkd, xad, devs):
        groups = []
        for h, d in zip(host, devs):
            kw = {}
            if rank:
                kw.update(xa=xkd, ld_xa=xkd.stride(0), R=rank, scale=1.0, xk=xkd, bk=d["bk"])
            if prologue:
                a, b = h["xa"]
                kw.update(xa=xad[:, a:], ld_xa=xad.stride(0), lb=d["lb"], R=b - a, scale=h["scale"])
            groups.append(_group(d["B"], d["C"], d["C"].shape[1], d["B"].stride(0), bias=d.get("bias"), **kw))
        _launch_gemm(Ad, groups, nf4=False, accumulate=accumulate, nn=nn)
        torch.cuda.synchronize()

    calls.clear()
    launch(Av, xkv, xav, dev)
    assert_launch(calls, entry, Av, [(d["B"], d["C"]) for d in dev])
    assert_guard(cpool, [Cv], cbefore, what)
    for pool, before in inputs:
        assert_unchanged(pool, before, what)
    # fp64 on the CPU (a sample of rows at the sizes where the reference is the cost)
    rows = torch.tensor(sample_rows(M) if sampled else list(range(M)))
    got = Cv[rows.to(DEV)].cpu()
    Ad64 = A[rows].double()
    for h in host:
        a, b = h["cols"]
        want = Ad64 @ (h["B"].double() if nn else h["B"].double().t())
        if rank:
            want += xk[rows].double() @ (h["bk"].double() if nn else h["bk"].double().t())
        if prologue:
            xa0, xa1 = h["xa"]
            want += h["scale"] * (xa[rows, xa0:xa1].to(dtype).double() @ h["lb"].double().t())
        if bias:
            want += h["bias"].double()
        if accumulate:
            want += C0[rows, a:b].double()
        _check_gemm(got[:, a:b], want, dtype, K, what + f" cols {a}:{b}")
    # the same launch on contiguous copies; same kernel -> same bits
    if same_kernel:
        cont = [{k: fresh(v) for k, v in d.items()} for d in dev]
        for h, c in zip(host, cont):
            a, b = h["cols"]
            c["C"] = C0[:, a:b].contiguous().to(DEV)
            assert all(t.data_ptr() % 16 == 0 for t in c.values())
        launch(fresh(Av), fresh(xkv) if rank else None, fresh(xav) if prologue else None, cont)
        for d, c in zip(dev, cont):
            assert torch.equal(d["C"], c["C"]), what + ": differs from the contiguous launch"


# 1. uamd_gemm_nt, gemm_nt_kernel (128 x 128 x 64 tiles, register-staged), GEMM256_MODE "off". The layouts only move the
#    epilogue between store_c4's forms inside that one kernel. (200, 130, 136): ragged in M, N and K -- the last K tile is 8 of
#    64 columns and the row padding behind it is NaN; N = 130 ends in a 2-column scalar tail on every layout. (1, 128, 64): one
#    row. (129, 257, 64): two row tiles, three column tiles, one column in the last.
@pytest.mark.parametrize("lay", list(C_LAYOUTS))
@pytest.mark.parametrize("M,N,K", [(200, 130, 136), (1, 128, 64), (129, 257, 64)])
def test_nt128_on_views(calls, M, N, K, lay):
    with gemm_mode("off"):
        run_gemm(calls, "uamd_gemm_nt", BF16, M, [N], K, lay)
        run_gemm(calls, "uamd_gemm_nt", BF16, M, [N], K, lay, accumulate=True, bias="odd" if lay == "off1" else "aligned")


def test_nt128_fp16_ragged(calls):
    with gemm_mode("off"):
        run_gemm(calls, "uamd_gemm_nt", F16, 200, [130], 136, "pad8_off8")


def test_nt128_zero_padding_columns_stay_zero(calls):
    """cross_entropy_loss._logits_chunk's layout in small (V = 32001 in rows of 32008): N = 257 in rows of 264 whose 7 padding
    columns are zero before the launch and -- the guard band includes them -- after it."""
    with gemm_mode("off"):
        run_gemm(calls, "uamd_gemm_nt", BF16, 129, [257], 64, "plain", zero_cols=7)


@pytest.mark.parametrize("lay", ["pad8_off8", "odd_ld"])
def test_nt128_register_prologue_lora_three_groups(calls, lay):
    """The LoRA term as (fp32 XA, LB, scale) in front of the K loop: three groups of different N and rank, XA a column block
    per group of one fp32 buffer with a padded `ld_xa`, LB with a padded `ld_lb`, C the column blocks of one buffer."""
    with gemm_mode("off"):
        run_gemm(calls, "uamd_gemm_nt", BF16, 200, [130, 64, 257], 136, lay, prologue=(16, 8, 24))
        run_gemm(calls, "uamd_gemm_nt", BF16, 200, [130, 64, 257], 136, lay, prologue=(16, 8, 24), accumulate=True, bias="aligned")


# 2. uamd_gemm_nt_nf4, gemm_nt_kernel<T, NF4 = true>: B is the packed weight (a flat byte array, 16-byte aligned, no stride)
#    and its fp32 absmax; the views are A and C. (77, 1024, 256): ragged M, 8 column tiles; (128, 128, 64): one whole tile.
@pytest.mark.parametrize("dtype,lay", [(BF16, lay) for lay in C_LAYOUTS] + [(F16, "pad8_off8")])
@pytest.mark.parametrize("M,N,K", [(77, 1024, 256), (128, 128, 64)])
def test_nf4_fused_on_views(calls, M, N, K, dtype, lay):
    from unsloth_amd.kernels.utils import _group, _launch_gemm
    from unsloth_amd.nf4 import quantize_nf4
    ie, io = in_layout(lay)
    ce, co = C_LAYOUTS[lay]
    X = torch.randn(M, K, generator=g(40)).to(dtype)
    W = (torch.randn(N, K, generator=g(41)) * 0.02).to(dtype).to(DEV)
    packed, qs = quantize_nf4(W, compress_statistics=False)
    Wd = R.nf4_dequantize_state(packed, qs).double()
    xpool, Xv = place(X, K + ie, io, NAN)
    ppool, pv = place(packed.cpu().view(1, -1), packed.numel(), 0, 0xFF)
    apool, av = place(qs.absmax.cpu().view(1, -1), qs.absmax.numel(), 0, NAN)
    before = [t.clone() for t in (xpool, ppool, apool)]
    want = X.double() @ Wd.t()
    for accumulate in (False, True):
        what = f"nf4 {M}x{N}x{K} {lay} {dtype} acc={accumulate}"
        C0 = torch.randn(M, N, generator=g(42)).to(dtype) if accumulate else torch.full((M, N), NAN, dtype=dtype)
        cpool, Cv = place(C0, N + ce, co, SENTINEL)
        cbefore = cpool.clone()
        calls.clear()
        _launch_gemm(Xv, [_group(pv, Cv, N, 0, absmax=av)], nf4=True, accumulate=accumulate)
        assert_launch(calls, "uamd_gemm_nt_nf4", Xv, [(pv, Cv)])
        assert_guard(cpool, [Cv], cbefore, what)
        _check_gemm(Cv, want + (C0.double() if accumulate else 0), dtype, K, what)
        Cc = C0.to(DEV)
        _launch_gemm(Xv.contiguous(), [_group(packed, Cc, N, 0, absmax=qs.absmax)], nf4=True, accumulate=accumulate)
        assert torch.equal(Cv, Cc), what + ": differs from the contiguous launch"
    for pool, b in zip((xpool, ppool, apool), before):
        assert torch.equal(pool.view(torch.uint8), b.view(torch.uint8)), "an input buffer was written"


# 3. uamd_gemm_nt_256 -> G256_PLAIN, gemm_nt256_kernel (8 waves, one workgroup per 256 x 256 tile): knobs 6 = 0 (no 128-row
#    tiles) and 7 = 0 (no persistent walk). (300, 260, 192): ragged M and N (4 columns in the last tile), never a candidate for
#    gemm_nt256s_kernel, so the contiguous run takes the same kernel.
PLAIN = dict(k6=0, k7=0)


@pytest.mark.parametrize("lay", list(C_LAYOUTS))
def test_nt256_plain_ragged_on_views(calls, lay):
    with gemm_mode("on", **PLAIN):
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 300, [260], 192, lay)
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 300, [260], 192, lay, rank=16, accumulate=True,
                 bias="odd" if lay in ("off1", "pad4_off4") else "aligned")


@pytest.mark.parametrize("kw", [dict(rank=16), dict(bias="aligned"), dict(bias="odd"), dict(accumulate=True)],
                         ids=["rank", "bias", "odd_bias", "accumulate"])
@pytest.mark.parametrize("lay", ["pad8_off8", "off1"])
def test_nt256_plain_epilogue_variants(calls, lay, kw):
    """Rank block, bias, accumulate one at a time; "odd_bias" with pad8_off8 is the unaligned-bias branch of store_c4's vector
    form (C takes 8-byte stores, bias + n does not take 8-byte loads)."""
    with gemm_mode("on", **PLAIN):
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 300, [260], 192, lay, **kw)


def test_nt256_plain_fp16_ragged(calls):
    with gemm_mode("on", **PLAIN):
        run_gemm(calls, "uamd_gemm_nt_256", F16, 300, [260], 192, "pad8_off8", rank=16)


@pytest.mark.parametrize("lay,kw", [("pad4_off4", {}), ("off1", {}), ("odd_ld", {}), ("pad8_off8", dict(bias="odd")),
                                    ("pad8_off8", dict(bias="odd", accumulate=True, rank=16))],
                         ids=["c_8byte_ldc516", "c_2byte", "ldc_odd", "bias_2byte", "bias_2byte_acc_rank"])
def test_nt256_whole_tiles_leave_the_s_kernel(calls, lay, kw):
    """(256, 512, 192): whole tiles, K = 3 tiles -- gemm_nt256s_kernel's launch when C and the bias take 16-byte accesses. A C
    4 elements in with ldc = 516, a C or a bias 1 element in, an odd ldc: whole_tiles() says no and the launch falls back to
    gemm_nt256_kernel. The contiguous run would take the S kernel, so no bit comparison here: the fp64 bound alone (that the
    two kernels agree bit for bit on aligned data is test_gemm256s_one_wave_per_simd_kernel_is_bit_identical's claim)."""
    with gemm_mode("on", **PLAIN):
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 256, [512], 192, lay, same_kernel=False, **kw)


# 4. uamd_gemm_nt_256 -> G256_HALF, gemm_nt256h_kernel (128 x 256 tiles, three-stage ring): knob 6 = 2. (129, 255, 320): one
#    row in the second row tile, N one short of a tile (the last store_c4 of a row has 3 of 4 columns); (300, 516, 192).
@pytest.mark.parametrize("lay", list(C_LAYOUTS))
@pytest.mark.parametrize("M,N,K", [(129, 255, 320), (300, 516, 192)])
def test_nt256_half_height_on_views(calls, M, N, K, lay):
    with gemm_mode("on", k6=2):
        run_gemm(calls, "uamd_gemm_nt_256", BF16, M, [N], K, lay)
        if lay in ("pad8_off8", "off1"):
            run_gemm(calls, "uamd_gemm_nt_256", BF16, M, [N], K, lay, rank=16, accumulate=True, bias="aligned")
        if lay == "pad8_off8" and M == 129:
            run_gemm(calls, "uamd_gemm_nt_256", F16, M, [N], K, lay)


# 5. uamd_gemm_nt_256 -> G256_S, gemm_nt256s_kernel<PERSIST = false> (4 waves, one workgroup per tile): whole tiles, K = 192.
#    fast_lora._gate_up's layout: the two groups' C are the column halves of ONE buffer with ldc = 2 * 512 + 64, A has
#    lda = K + 64 ("rowpad64"). Every C start and ldc is a multiple of 8: the launch stays on the S kernel, as does the
#    contiguous one.
@pytest.mark.parametrize("kw", [{}, dict(rank=16), dict(accumulate=True, rank=16, bias="aligned")], ids=["plain", "rank", "all"])
def test_nt256_s_kernel_gate_up_layout(calls, kw):
    with gemm_mode("on", k6=0, k11=2):
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 512, [512, 512], 192, "rowpad64", **kw)
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 512, [512, 512], 192, "pad8_off8", **kw)


# 6. uamd_gemm_nt_256 -> G256_S, gemm_nt256s_kernel<PERSIST = true>: knob 11 = 9 walks from two tiles per compute unit on;
#    (4096, 8192, 192) is 512 tiles. fp64 on sampled rows, the guard band in full.
@pytest.mark.parametrize("accumulate", [False, True])
def test_nt256_s_kernel_persistent_walk_padded(calls, accumulate):
    with gemm_mode("on", k6=0, k11=9):
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 4096, [8192], 192, "rowpad64", accumulate=accumulate, sampled=True)


# 7. uamd_gemm_nt_256 -> G256_PERSIST, gemm_nt256p_kernel (8 waves, one workgroup per compute unit): knobs 6 = 0, 7 = 2,
#    11 = 0; (4096 + 40, 4096 + 8, 256) is 17 x 17 tiles, ragged both ways. knob 9 picks the load-free-epilogue instance
#    (PLAIN = true, taken without accumulate and bias) or the run-time-dispatch one. odd_ld: its scalar epilogue.
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("plain9", [1, 0])
@pytest.mark.parametrize("lay", ["pad8_off8", "odd_ld"])
def test_nt256_persistent_kernel_on_views(calls, lay, plain9, accumulate):
    with gemm_mode("on", k6=0, k7=2, k11=0, k9=plain9):
        run_gemm(calls, "uamd_gemm_nt_256", BF16, 4096 + 40, [4096 + 8], 256, lay, accumulate=accumulate, sampled=True)


# 8. uamd_gemm_nn_256: B [K, N] and BK [Rk, N] row-major, read through transposing LDS fragments. B and BK are column blocks
#    of wider buffers (136 + 8 columns in front, ldb = N + 272), NaN in the neighbouring blocks. (300, 520, 192) and
#    (77, 4104, 128), 256-row (knob 6 = 0, gemm_nt256_kernel<BNN>) and 128-row tiles (6 = 2, gemm_nt256h_kernel<BNN>).
@pytest.mark.parametrize("lay", ["plain", "pad8_off8", "pad4_off4", "odd_ld", "off1"])
@pytest.mark.parametrize("half", [0, 2])
@pytest.mark.parametrize("M,N,K", [(300, 520, 192), (77, 4104, 128)])
def test_nn256_on_views(calls, M, N, K, half, lay):
    with gemm_mode("auto", k6=half, k7=0):
        run_gemm(calls, "uamd_gemm_nn_256", BF16, M, [N], K, lay, nn=True)
        if lay in ("pad8_off8", "off1"):
            run_gemm(calls, "uamd_gemm_nn_256", BF16, M, [N], K, lay, nn=True, rank=16, accumulate=True)
        if lay == "pad8_off8" and M == 300:
            run_gemm(calls, "uamd_gemm_nn_256", F16, M, [N], K, lay, nn=True, rank=16)


# ------------------------------------------------------------------------------------------------ 9. dense_dw (uamd_gemm_tn_256)
# gemm_nt256_kernel<BNN, ATN>: both operands with the contracted token dimension as rows. dY is the MIDDLE column block of a
# three-block buffer (dQ | dK | dV), X has a padded row stride, `out` is a row-padded, column-offset view. (192, 264, 328):
# ragged in both output dimensions; (512, 256, 512): whole tiles.
@pytest.mark.parametrize("dtype,lay", [(BF16, lay) for lay in ("plain", "pad8_off8", "pad4_off4", "odd_ld", "off1")]
                         + [(F16, "pad8_off8")])
@pytest.mark.parametrize("T,n_out,n_in", [(192, 264, 328), (512, 256, 512)])
def test_dense_dw_on_views(calls, T, n_out, n_in, dtype, lay):
    from unsloth_amd.kernels.utils import dense_dw
    ie, io = in_layout(lay)
    ce, co = C_LAYOUTS[lay]
    gen = g(T + n_out)
    dY = (torch.randn(T, n_out, generator=gen) * 0.1).to(dtype)
    X = (torch.randn(T, n_in, generator=gen) * 0.5).to(dtype)
    ypool, dYv = place(dY, 3 * n_out + ie, n_out + io, NAN) if lay != "plain" else place(dY, n_out, 0, NAN)
    xpool, Xv = place(X, n_in + ie, io, NAN)
    ybefore, xbefore = ypool.clone(), xpool.clone()
    ref = dY.double().t() @ X.double()
    lib = (dY.to(DEV).t() @ X.to(DEV)).float().cpu()
    for accumulate in (False, True):
        what = f"dense_dw {T}x{n_out}x{n_in} {lay} {dtype} acc={accumulate}"
        C0 = torch.randn(n_out, n_in, generator=gen).to(dtype) if accumulate else torch.full((n_out, n_in), NAN, dtype=dtype)
        opool, ov = place(C0, n_in + 64 + ce, 64 + co, SENTINEL)           # a column block of a row-padded buffer
        obefore = opool.clone()
        calls.clear()
        got = dense_dw(dYv, Xv, out=ov, accumulate=accumulate)
        assert got.data_ptr() == ov.data_ptr()
        assert_launch(calls, "uamd_gemm_tn_256", dYv, [(Xv, ov)])
        assert_guard(opool, [ov], obefore, what)
        assert torch.isfinite(ov.float()).all(), what
        # test_dense_dw_matches_torch's bounds
        if accumulate:
            assert rel_fro(ov, ref + C0.double()) < (6e-3 if dtype == BF16 else 1e-3), what
        else:
            assert rel_fro(ov, ref) < (4e-3 if dtype == BF16 else 6e-4), what
            assert rel_fro(ov, ref) <= 1.5 * rel_fro(lib, ref) + 1e-6, what
        # same kernel on contiguous copies -> same bits
        oc = C0.to(DEV)
        dense_dw(dY.to(DEV), X.to(DEV), out=oc, accumulate=accumulate)
        assert torch.equal(ov, oc), what + ": differs from the contiguous launch"
    assert_unchanged(ypool, ybefore, "dY")
    assert_unchanged(xpool, xbefore, "X")


# ---------------------------------------------------------------------------------- 10. uamd_lora_xa / uamd_lora_xa2 / uamd_lora_xa2k
# X @ A^T in fp32 (+ the same sums in the activation dtype, zero-filled to the rank block's width). (333, 520, [16, 8]): ragged
# M (11 row groups of 32, the last of 13), K = 8 whole 64-steps + 8 columns -- the kernels' ragged-K clamp re-reads valid
# bytes and must not reach the NaN behind the row; (33, 64, [64]): one row in the second group, one K step, four rank tiles.
#   "xa"   utils.LORA_XA_V2 = False -> lora_xa_kernel (csrc/gemm.hip)
#   "xa2"  lora_xa2_kernel, fp32 output only
#   "xa2k" lora_xa2_kernel with the rank-block output `out_k`
@pytest.mark.parametrize("dtype,lay", [(BF16, "plain"), (BF16, "pad8_off8"), (BF16, "rowpad64"), (F16, "pad8_off8")])
@pytest.mark.parametrize("entry", ["xa", "xa2", "xa2k"])
@pytest.mark.parametrize("M,K,Rs", [(333, 520, [16, 8]), (33, 64, [64])])
def test_lora_xa_on_views(calls, M, K, Rs, entry, dtype, lay):
    from unsloth_amd.kernels import utils as U
    ie, io = in_layout(lay)
    X = torch.randn(M, K, generator=g(90)).to(dtype)
    As = [(torch.randn(r, K, generator=g(91 + i)) * 0.05).to(dtype) for i, r in enumerate(Rs)]
    Rt = sum(Rs)
    want = torch.cat([X.double() @ a.double().t() for a in As], dim=1)
    xpool, Xv = place(X, K + ie, io, NAN)
    xbefore = xpool.clone()
    pad = 4 if lay != "plain" else 0
    opool, ov = place(torch.full((M, Rt), NAN), Rt + pad, pad, SENTINEL)          # fp32: ld % 4, any alignment
    kpool, kv = place(torch.full((M, 64), NAN, dtype=dtype), 64 + ie, io, SENTINEL)
    obefore, kbefore = opool.clone(), kpool.clone()
    old = U.LORA_XA_V2
    U.LORA_XA_V2 = entry != "xa"
    try:
        calls.clear()
        if entry == "xa2k":
            out, offs = U.lora_xa(Xv, [a.to(DEV) for a in As], out=ov, out_k=kv, k_cols=64)
        else:
            out, offs = U.lora_xa(Xv, [a.to(DEV) for a in As], out=ov)
    finally:
        U.LORA_XA_V2 = old
    side = [c for c in calls if c[0] in SIDE_ENTRIES]
    assert [c[0] for c in side] == ["uamd_lora_" + entry]
    a = side[0][1]
    assert _addr(a[0]) == Xv.data_ptr() and a[1] == Xv.stride(0) and _addr(a[4]) == ov.data_ptr() and a[5] == ov.stride(0)
    assert out.data_ptr() == ov.data_ptr() and [o for o, _ in offs] == [sum(Rs[:i]) for i in range(len(Rs))]
    what = f"lora_{entry} {M}x{K}x{Rs} {lay} {dtype}"
    assert torch.isfinite(ov).all(), what
    torch.testing.assert_close(ov.cpu(), want.float(), rtol=1e-4, atol=1e-4 * float(want.abs().mean()) + 1e-5)   # test_lora_xa's
    assert_guard(opool, [ov], obefore, what)
    assert_unchanged(xpool, xbefore, what)
    if entry == "xa2k":
        assert _addr(a[6]) == kv.data_ptr() and a[7] == kv.stride(0)
        assert torch.equal(kv[:, :Rt], ov.to(dtype)), "the rank block holds the fp32 sums rounded once"
        assert torch.all(kv[:, Rt:] == 0), "columns past the rank up to the rank block's width are zero"
        assert_guard(kpool, [kv], kbefore, what)
    else:
        assert_unchanged(kpool, kbefore, what)
    # same kernel on contiguous copies -> same bits
    U.LORA_XA_V2 = entry != "xa"
    try:
        out2, _ = U.lora_xa(X.to(DEV), [a.to(DEV) for a in As])
    finally:
        U.LORA_XA_V2 = old
    assert torch.equal(ov, out2)


@pytest.mark.parametrize("M,K,Rs", [(333, 520, [16, 8]), (33, 64, [64])])
def test_xa_and_rank_block_on_a_padded_activation(calls, M, K, Rs):
    """utils._xa_and_rank_block, what lora_linear_forward calls for the 256-tile kernels: uamd_lora_xa2k into buffers of its own;
    the rank block is 64 wide, zero past the ranks."""
    from unsloth_amd.kernels import utils as U
    X = torch.randn(M, K, generator=g(90)).to(BF16)
    As = [(torch.randn(r, K, generator=g(91 + i)) * 0.05).to(BF16) for i, r in enumerate(Rs)]
    Rt = sum(Rs)
    want = torch.cat([X.double() @ a.double().t() for a in As], dim=1)
    xpool, Xv = place(X, K + 64, 0, NAN)
    calls.clear()
    terms = U._xa_and_rank_block(Xv, [a.to(DEV) for a in As], True)
    xa, xk = torch.cat([t.P for t in terms], dim=1), terms[0].xk
    assert all(t.xk is xk for t in terms) and [t.col for t in terms] == [sum(Rs[:i]) for i in range(len(Rs))]
    side = [c for c in calls if c[0] in SIDE_ENTRIES]
    assert [c[0] for c in side] == ["uamd_lora_xa2k"] and _addr(side[0][1][0]) == Xv.data_ptr() and side[0][1][1] == K + 64
    torch.testing.assert_close(xa.cpu(), want.float(), rtol=1e-4, atol=1e-4 * float(want.abs().mean()) + 1e-5)
    assert tuple(xk.shape) == (M, 64) and torch.equal(xk[:, :Rt], xa.to(BF16)) and torch.all(xk[:, Rt:] == 0)


# ------------------------------------------------------------------------------------------------------------ 11. uamd_lora_tn
# G = s P^T Z (fp32): lora_tn_kernel + lora_tn_reduce_kernel. Z is a column block of a wider 16-bit buffer with a padded
# `ldz`; P is fp32 with `ldp` padded to a multiple of 4 and NaN behind its R columns (the kernel fetches P in float4s: with
# R = 1 three of the four floats are padding it must drop, not multiply by zero); `out` is a view with a padded `ldo` in either
# layout, overwritten or added to. utils.lora_tn passes `ldo` = the width, so the padded `ldo` goes to the entry point directly.
def _tn_launch(probs, M, dtype):
    from unsloth_amd import _lib
    S = (M + 127) // 128
    need = sum(S * 16 * ((p.N + 127) // 128) * 128 for p in probs)
    ws = torch.empty(need, dtype=F32, device=DEV)
    arr = (_lib.LoraTnProblem * len(probs))(*probs)
    _lib.call("uamd_lora_tn", ws, arr, len(probs), M, _lib.ptr(ws), need, _lib.dtype_code(dtype), _lib.stream_of(ws))
    torch.cuda.synchronize()


def _tn_bound(want, M):
    return 2e-5 * (want.abs().max().item() + 1e-30) * max(1.0, (M / 512) ** 0.5)      # test_lora_tn_matches_fp64's


@pytest.mark.parametrize("dtype,padded", [(BF16, False), (BF16, True), (F16, True)])
@pytest.mark.parametrize("M,N,R", [(777, 1032, 16), (3, 8, 1)])
def test_lora_tn_on_views(calls, M, N, R, dtype, padded):
    from unsloth_amd import _lib
    P = torch.randn(M, R, generator=g(201))
    Z = torch.randn(M, N, generator=g(202)).to(dtype)
    R4 = (R + 3) // 4 * 4
    ppool, Pv = place(P, R4 + 4, 4, NAN) if padded else place(P, R4, 0, NAN)
    zpool, Zv = place(Z, 2 * N + 72, N + 8, NAN) if padded else place(Z, N, 0, NAN)
    pbefore, zbefore = ppool.clone(), zpool.clone()
    base = P.to(dtype).double().t() @ Z.double()                                      # [R, N]
    for out_nr in (False, True):
        for add in (False, True):
            what = f"lora_tn {M}x{N}x{R} {dtype} padded={padded} out_nr={out_nr} add={add}"
            scale = 2.0 if out_nr else 0.5
            want = scale * (base.t() if out_nr else base)
            prior = torch.randn(want.shape, generator=g(203)) if add else torch.full(want.shape, NAN)
            opool, ov = place(prior, want.shape[1] + (3 if padded else 0), 1 if padded else 0, SENTINEL)
            obefore = opool.clone()
            calls.clear()
            _tn_launch([_lib.LoraTnProblem(P=Pv.data_ptr(), Z=Zv.data_ptr(), out=ov.data_ptr(), ldp=Pv.stride(0), ldz=Zv.stride(0),
                                           ldo=ov.stride(0), N=N, R=R, out_nr=int(out_nr) | (2 if add else 0), scale=scale)], M, dtype)
            assert [c[0] for c in calls] == ["uamd_lora_tn"]
            assert torch.isfinite(ov).all(), what + ": padding reached the product"
            if add:
                want = want + prior.double()
            err = (ov.double().cpu() - want).abs().max().item()
            assert err <= _tn_bound(want, M), (what, err)
            assert_guard(opool, [ov], obefore, what)
    assert_unchanged(ppool, pbefore, "P")
    assert_unchanged(zpool, zbefore, "Z")


@pytest.mark.parametrize("case", ["aligned", "ldp_odd", "p_off1", "ldz_odd", "z_off1"])
def test_lora_tn_wrapper_splits_ranks_and_takes_any_view(calls, case):
    """utils.lora_tn with R = 40 (three descriptors of 16 + 16 + 8 ranks in ONE launch) on a padded P and a column block Z that
    the entry point takes as they are ("aligned": the descriptors carry the views' own pointers), and on the views it answers
    UAMD_ERR_ALIGN to -- `ldp % 4`, P off the 16-byte grid, `ldz % 8`, Z off the 16-byte grid -- which the wrapper hands over
    as aligned copies: the same bits."""
    from unsloth_amd.kernels.utils import lora_tn
    M, N, Rr = 300, 264, 40
    P = torch.randn(M, Rr, generator=g(211))
    Z = torch.randn(M, N, generator=g(212)).to(BF16)
    ldp, poff = {"ldp_odd": (Rr + 3, 0), "p_off1": (Rr + 4, 1)}.get(case, (Rr + 4, 4))
    ldz, zoff = {"ldz_odd": (N + 3, 0), "z_off1": (N + 8, 1)}.get(case, (2 * N + 8, N))
    ppool, Pv = place(P, ldp, poff, NAN)
    zpool, Zv = place(Z, ldz, zoff, NAN)
    base = P.to(BF16).double().t() @ Z.double()
    ref = lora_tn([(P.to(DEV), Z.to(DEV), Rr, False, 0.5), (P.to(DEV), Z.to(DEV), Rr, True, 2.0)])
    calls.clear()
    outs = lora_tn([(Pv, Zv, Rr, False, 0.5), (Pv, Zv, Rr, True, 2.0)])
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["uamd_lora_tn"] and calls[0][1][1] == 6
    d = calls[0][1][0]
    assert [d[i].R for i in range(6)] == [16, 16, 8] * 2
    p_in_place, z_in_place = case in ("aligned", "ldz_odd", "z_off1"), case in ("aligned", "ldp_odd", "p_off1")
    assert (d[1].P == Pv.data_ptr() + 64 and d[0].ldp == ldp) == p_in_place
    assert (d[0].Z == Zv.data_ptr() and d[0].ldz == ldz) == z_in_place
    for o, w, r in zip(outs, (0.5 * base, 2.0 * base.t()), ref):
        err = (o.double().cpu() - w).abs().max().item()
        assert torch.isfinite(o).all() and err <= _tn_bound(w, M), (case, err)
        assert torch.equal(o, r), "the same bits as on contiguous operands"
    # `+=` onto a known prior
    prior = [torch.randn(o.shape, generator=g(213)).to(DEV) for o in outs]
    tg = [p.clone() for p in prior]
    lora_tn([(Pv, Zv, Rr, False, 0.5), (Pv, Zv, Rr, True, 2.0)], targets=tg)
    for t, p, o in zip(tg, prior, outs):
        assert torch.equal(t, p + o)


# ------------------------------------------------------------------------------------------------------------------- wrappers
# The production layouts through the public helpers, then the views the C contract does not take.
def _proj(N, K, r, seed, dtype=BF16):
    W = (torch.randn(N, K, generator=g(seed)) * 0.05).to(dtype)
    A = torch.randn(r, K, generator=g(seed + 1)) * 0.05
    B = torch.randn(N, r, generator=g(seed + 2)) * 0.05
    return W, A, B


def _fwd_ref(X, W, A, B, s, dtype):
    xa = (X.double() @ A.to(dtype).double().t()).to(dtype).double()                    # utils.py:1166's rounding point
    return X.double() @ W.double().t() + s * (xa @ B.to(dtype).double().t())


@pytest.mark.parametrize("mode,entry", [("off", "uamd_gemm_nt"), ("on", "uamd_gemm_nt_256")])
def test_lora_linear_forward_into_column_halves(calls, mode, entry):
    """fast_lora._gate_up: e and g are the column halves of one alloc_rows buffer, I = 320, ld = 2 I + 64. "off": the 128-tile
    kernel with the register-prologue LoRA term; "on": the 256-tile family with the rank block."""
    from unsloth_amd.kernels.utils import alloc_rows, lora_linear_forward
    M, K, I, r, s = 300, 192, 320, 16, 2.0
    X = torch.randn(M, K, generator=g(7)).to(BF16)
    (Wg, Ag, Bg), (Wu, Au, Bu) = _proj(I, K, r, 10), _proj(I, K, r, 20)
    eg = alloc_rows(M, 2 * I, BF16, DEV, ld=2 * I + 64)
    buf = eg._base
    assert tuple(buf.shape) == (M, 2 * I + 64)
    buf.fill_(SENTINEL)
    eg.fill_(NAN)
    before = buf.clone()
    Xd, Wgd, Wud = X.to(DEV), Wg.to(DEV), Wu.to(DEV)
    with gemm_mode(mode):
        calls.clear()
        e, gg = lora_linear_forward(Xd, [(Wgd, None, Ag.to(DEV), Bg.to(DEV), s), (Wud, None, Au.to(DEV), Bu.to(DEV), s)],
                                    outs=[eg[:, :I], eg[:, I:]])
        torch.cuda.synchronize()
    assert_launch(calls, entry, Xd, [(Wgd, eg[:, :I]), (Wud, eg[:, I:])])
    assert e.data_ptr() == eg.data_ptr() and gg.data_ptr() == eg[:, I:].data_ptr()
    assert_guard(buf.view(-1), [eg], before.view(-1), "gate|up")
    # (s = 2: folding the scale into BK before its rounding, as rank_block_bk does for the 256-tile kernels, changes nothing)
    want = [_fwd_ref(X, W, A, B, s, BF16) for W, A, B in ((Wg, Ag, Bg), (Wu, Au, Bu))]
    _check_gemm(eg[:, :I], want[0], BF16, K, "gate")
    _check_gemm(eg[:, I:], want[1], BF16, K, "up")


def _dx_case(M, Kin, Ns, r, dtype=BF16):
    from unsloth_amd.nf4 import quantize_nf4
    want = torch.zeros(M, Kin, dtype=torch.float64)
    dYs, projs = [], []
    for i, N in enumerate(Ns):
        W = (torch.randn(N, Kin, generator=g(50 + i)) * 0.02).to(dtype).to(DEV)
        packed, qs = quantize_nf4(W, compress_statistics=True)
        Wd = R.nf4_dequantize_state(packed, qs).double()
        A = torch.randn(r, Kin, generator=g(60 + i)) * 0.05
        B = torch.randn(N, r, generator=g(70 + i)) * 0.05
        dY = torch.randn(M, N, generator=g(80 + i)).to(dtype)
        dyb = (dY.double() @ B.to(dtype).double()).to(dtype).double()
        want = want + dY.double() @ Wd + 0.5 * dyb @ A.to(dtype).double()
        dYs.append(dY)
        projs.append((packed, qs, A.to(DEV), B.to(DEV), 0.5))
    return dYs, projs, want


@pytest.mark.parametrize("merged", [False, True])
@pytest.mark.parametrize("mode", ["off", "on"])
def test_lora_linear_dx_onto_a_padded_output(calls, mode, merged):
    """mlp_backward's layout: df | de are the column halves of one buffer with ld = 2 I + 64 (merged: ONE GEMM over the
    concatenated features reads [df | de] in place) or two buffers (one GEMM per projection, the second accumulating), dX
    goes to an alloc_rows(ld = Kin + 64) buffer. The 2-ulp bound of test_lora_linear_dx_accumulates_groups."""
    from unsloth_amd.kernels.utils import alloc_rows, lora_linear_dx
    M, Kin, I, r = 260, 256, 320, 16
    dYs, projs, want = _dx_case(M, Kin, [I, I], r)
    if merged:
        ypool, both = place(torch.cat(dYs, dim=1), 2 * I + 64, 0, NAN)
        dYd = [both[:, :I], both[:, I:]]
    else:
        dYd = [place(dY, I + 8, 8, NAN)[1] for dY in dYs]
    out = alloc_rows(M, Kin, BF16, DEV, ld=Kin + 64)
    buf = out._base
    buf.fill_(SENTINEL)
    out.fill_(7.0)                                   # must be overwritten, not added to
    before = buf.clone()
    with gemm_mode(mode):
        calls.clear()
        got = lora_linear_dx(dYd, projs, out=out)
        torch.cuda.synchronize()
    gemms = [c for c in calls if c[0] in GEMM_ENTRIES]
    form = "uamd_gemm_nn_256" if mode == "on" else "uamd_gemm_nt"
    assert [c[0] for c in gemms] == [form] * (1 if merged else 2)
    for i, c in enumerate(gemms):
        A = both if merged else dYd[i]
        assert _addr(c[1][0]) == A.data_ptr() and c[1][1] == A.stride(0), "dY was copied"
        assert c[1][4][0].C == out.data_ptr() and c[1][4][0].ldc == Kin + 64 and c[1][6] == int(i > 0)
    assert got.data_ptr() == out.data_ptr()
    assert_guard(buf.view(-1), [out], before.view(-1), "dX")
    assert_ulp(out, want, BF16, ulps=2, atol=2.0 ** -7 * float(want.abs().mean()), what="dX", allow_frac=1e-3)


@pytest.mark.parametrize("mode", ["off", "on"])
@pytest.mark.parametrize("what", ["weight_off1", "weight_off4", "x_off1", "x_ld_odd"])
def test_lora_linear_forward_takes_misaligned_operands_through_a_copy(calls, what, mode):
    """A dense weight or an activation that starts off the 16-byte grid (or has `ld % 8 != 0`): the entry points answer
    UAMD_ERR_ALIGN, the wrapper hands them an aligned copy -- the same bits as the aligned call."""
    from unsloth_amd.kernels.utils import lora_linear_forward
    M, K, N = 200, 192, 264
    X = torch.randn(M, K, generator=g(5)).to(BF16)
    W = (torch.randn(N, K, generator=g(6)) * 0.05).to(BF16)
    off = {"weight_off1": 1, "weight_off4": 4}.get(what, 0)
    Wv = place(W, K + 8 if off else K, off, NAN)[1]
    Xv = place(X, K + 3 if what == "x_ld_odd" else K, 1 if what == "x_off1" else 0, NAN)[1]
    entry = "uamd_gemm_nt_256" if mode == "on" else "uamd_gemm_nt"
    with gemm_mode(mode):
        calls.clear()
        (ref,) = lora_linear_forward(X.to(DEV), [(W.to(DEV), None, None, None, None)])
        a = calls[0][1]
        assert calls[0][0] == entry and a[1] == K and a[4][0].ldb == K                  # aligned: read in place, as before
        calls.clear()
        (Y,) = lora_linear_forward(Xv, [(Wv, None, None, None, None)])
        torch.cuda.synchronize()
    a = calls[0][1]
    assert [c[0] for c in calls] == [entry] and _addr(a[0]) % 16 == 0 and a[4][0].B % 16 == 0
    assert (_addr(a[0]) == Xv.data_ptr()) == what.startswith("weight") and (a[4][0].B == Wv.data_ptr()) == what.startswith("x_")
    _check_gemm(Y, X.double() @ W.double().t(), BF16, K, what)
    assert torch.equal(Y, ref)


def test_lora_linear_dx_takes_a_misaligned_dense_weight_through_a_copy(calls):
    from unsloth_amd.kernels.utils import lora_linear_dx
    M, N, Kin = 300, 192, 264
    dY = torch.randn(M, N, generator=g(5)).to(BF16)
    W = (torch.randn(N, Kin, generator=g(6)) * 0.05).to(BF16)
    Wv = place(W, Kin + 8, 1, NAN)[1]
    with gemm_mode("on"):                           # the NN form reads a dense [out, in] weight in place when it can
        calls.clear()
        ref = lora_linear_dx([dY.to(DEV)], [(W.to(DEV), None, None, None, None)])
        assert [c[0] for c in calls] == ["uamd_gemm_nn_256"] and calls[0][1][4][0].ldb == Kin
        calls.clear()
        got = lora_linear_dx([dY.to(DEV)], [(Wv, None, None, None, None)])
        torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["uamd_gemm_nn_256"] and calls[0][1][4][0].B % 16 == 0 and calls[0][1][4][0].B != Wv.data_ptr()
    _check_gemm(got, dY.double() @ W.double(), BF16, N, "dX")
    assert torch.equal(got, ref)


def test_output_buffers_the_epilogue_cannot_address_are_refused(calls):
    """`outs=` / `out=` with a column stride, the wrong shape or the wrong dtype: a ValueError that names the argument, before
    anything is launched (the kernel sees a pointer and `ldc` and would write elsewhere)."""
    from unsloth_amd.kernels.utils import dense_dw, lora_linear_dx, lora_linear_forward, matmul_lora
    M, K, N = 64, 64, 128
    X = torch.randn(M, K, generator=g(1)).to(BF16).to(DEV)
    W = (torch.randn(N, K, generator=g(2)) * 0.05).to(BF16).to(DEV)
    dY = torch.randn(M, N, generator=g(3)).to(BF16).to(DEV)
    bad = {"column stride": lambda r, c: torch.zeros(r, 2 * c, dtype=BF16, device=DEV)[:, ::2],
           "shape": lambda r, c: torch.zeros(r, c + 8, dtype=BF16, device=DEV),
           "transposed": lambda r, c: torch.zeros(c, r, dtype=BF16, device=DEV).t(),
           "dtype": lambda r, c: torch.zeros(r, c, dtype=F32, device=DEV)}
    calls.clear()
    for why, make in bad.items():
        with pytest.raises(ValueError, match=r"outs\[0\]"):
            lora_linear_forward(X, [(W, None, None, None, None)], outs=[make(M, N)])
        with pytest.raises(ValueError, match="out"):
            lora_linear_dx([dY], [(W, None, None, None, None)], out=make(M, K))
        with pytest.raises(ValueError, match="out"):
            dense_dw(dY, X, out=make(N, K))
    assert calls == [], "nothing may be launched"
    # a dense [batch, seq, N] buffer, as matmul_lora's callers pass it, is the [M, N] matrix
    out3 = torch.full((2, M // 2, N), NAN, dtype=BF16, device=DEV)
    got = matmul_lora(X.view(2, M // 2, K), W, None, None, None, None, out=out3)
    assert got.data_ptr() == out3.data_ptr() and tuple(got.shape) == (2, M // 2, N)
    _check_gemm(out3.view(M, N), X.double().cpu() @ W.double().cpu().t(), BF16, K, "3-D out")
