"""Host-side mirror of unsloth/kernels/utils.py for the MI355X path.

Same names and argument meaning as the reference:
  QUANT_STATE                utils.py:319-320
  get_lora_parameters(_bias) utils.py:335-440   (the plug-in contract with PEFT)
  fast_dequantize            utils.py:567-679
  matmul_lora                utils.py:1128-1170
  calculate_settings         utils.py:114-133   (kept for API compatibility; the HIP kernels have no
                                                 65536-column limit, so nothing here raises on size)
plus the grouped entry points the manual-autograd Functions in fast_lora.py use
(`lora_linear_forward`, `lora_linear_dx`), which is where the MI355X design differs: projections
that share their input (q/k/v, gate/up) are ONE uamd_lora_xa launch and ONE grouped MFMA GEMM
launch, with NF4 decode and the LoRA term fused into the GEMM (csrc/gemm.hip).
"""
import ctypes
import functools
import os

import torch

from .. import _lib
from .. import nf4 as _nf4
from .._lib import GemmGroup

MAX_FUSED_SIZE = 65536
next_power_of_2 = lambda n: 1 << (max(int(n), 1) - 1).bit_length()

# NF4 forward policy. Decoding NF4 inside the GEMM (csrc/gemm.hip, no bf16 copy of W in HBM) repeats the decode
# once per 128-row M tile, so it only pays while the launch is weight-bandwidth-bound (few tokens). From
# FUSED_NF4_MAX_M tokens on, W is decoded ONCE into a per-device bf16 scratch (2.5 B/param of HBM traffic,
# ~3 % of the GEMM time at 8192 tokens) and the dense 256x256 LDS-DMA kernel runs at ~2x the fused rate.
FUSED_NF4 = True
FUSED_NF4_MAX_M = 512
# dense GEMM kernel selection: "auto" = the 256x256 ping-pong kernel (csrc/gemm256.hip: LDS-DMA, 8 waves in two
# anti-phase groups) once the launch has enough 256x256 tiles to fill the 256 CUs (GEMM256_MIN_TILES), else the
# 128x128 register-staged kernel (csrc/gemm.hip); "on"/"off" force it.
GEMM256_MODE = "auto"
# (160 since round 4: Qwen2-VL's ViT linears with N = 1280 at 4096 patches are 160 half-height tiles -- on the 128 x 128 kernel
# they ran at 0.18 PFLOP/s, the config-4 step is 2.7 % faster with them on the 256 family: profiles/r04p_config4_min_tiles_ab.txt)
GEMM256_MIN_TILES = 160
# X @ A^T / dY @ B: streaming LDS-DMA kernel (csrc/lora_side.hip) for total rank <= LORA_XA2_MAX_RANKS, else the first version
LORA_XA_V2 = True
# rank columns of one uamd_lora_xa launch (csrc/gemm.hip: twelve 16-rank tiles); wider stacks go in chunks (_rank_plan)
LORA_XA_MAX_RANKS = 192
# rank columns of one uamd_lora_xa2 / uamd_lora_xa2k launch
LORA_XA2_MAX_RANKS = 64


def calculate_settings(n):
    """(BLOCK_SIZE, num_warps) as utils.py:114-133. Informational only on this backend."""
    BLOCK_SIZE = next_power_of_2(n)
    num_warps = 4
    if BLOCK_SIZE >= 32768:
        num_warps = 32
    elif BLOCK_SIZE >= 8192:
        num_warps = 16
    elif BLOCK_SIZE >= 2048:
        num_warps = 8
    return BLOCK_SIZE, num_warps


def QUANT_STATE(W):
    return getattr(W, "quant_state", None)


# utils.py:325-332: the dtypes for which a layer's `weight_scale(_inv)` IS its quant state. A bf16 weight that still
# carries a scale (a decompressed compressed-tensors layer) must NOT get one, or the NF4 path would read a missing absmax
# (the reference's tests/test_fast_gemv_dispatch.py:38-63 pins exactly this resolution).
_FP8_WEIGHT_DTYPES = tuple(d for d in (getattr(torch, "float8_e4m3fn", None), getattr(torch, "float8_e5m2", None))
                           if d is not None)


def _resolve_quant_state(base_layer, W):
    """utils.py:351-366 / :407-422: bitsandbytes' quant_state off the weight; for a weight that is still fp8 the layer's
    weight_scale_inv / weight_scale (block size stamped the way the reference passes it along). This backend has no fp8
    GEMM: the resolution is kept for the plugin contract, the kernels refuse such a weight loudly (_refuse_fp8)."""
    W_quant = getattr(W, "quant_state", None)
    if W_quant is None and W.dtype in _FP8_WEIGHT_DTYPES:
        W_quant = getattr(base_layer, "weight_scale_inv", None)
        if W_quant is None:
            W_quant = getattr(base_layer, "weight_scale", None)
    if getattr(base_layer, "quant_method", None) == "fp8":
        W.block_size = getattr(base_layer, "block_size", [128, 128])
        if W_quant is not None:
            W_quant.block_size = W.block_size
    return W_quant


def _refuse_fp8(projs):
    for p in projs:
        if p[0].dtype in _FP8_WEIGHT_DTYPES:
            raise NotImplementedError(
                "fp8 base weights (weight_scale / weight_scale_inv quant state) are outside this backend's scope: the MI355X "
                "path takes NF4 (bitsandbytes layout) or 16-bit base weights. The reference routes them to "
                "unsloth/kernels/fp8.py (utils.py:1146-1152).")


def get_lora_parameters(proj):
    """(W, quant_state, A, B, scaling) of a PEFT-style LoRA layer; utils.py:335-397.
    Disabled / merged adapters -> (W, quant_state, None, None, None) (:369-370)."""
    base_layer = getattr(proj, "base_layer", proj)
    W = base_layer.weight
    if hasattr(base_layer, "weight_fake_quantizer"):
        fq = getattr(base_layer, "weight_fake_quantizer", None)
        if fq is not None:
            W = fq(W)
    W_quant = _resolve_quant_state(base_layer, W)
    if getattr(proj, "disable_adapters", True) or proj.merged:
        return W, W_quant, None, None, None
    adapter = getattr(proj, "active_adapters", None)
    if adapter is None:
        adapter = getattr(proj, "active_adapter", ("default"))
    adapter = adapter[0]
    A = proj.lora_A[adapter].weight
    B = proj.lora_B[adapter].weight
    fq = getattr(proj.lora_A[adapter], "weight_fake_quantizer", None)
    if fq is not None:
        A = fq(A)
    fq = getattr(proj.lora_B[adapter], "weight_fake_quantizer", None)
    if fq is not None:
        B = fq(B)
    return W, W_quant, A, B, proj.scaling[adapter]


def get_lora_parameters_bias(proj):
    """utils.py:400-440: same plus the base layer's bias."""
    base_layer = getattr(proj, "base_layer", proj)
    W = base_layer.weight
    W_quant = _resolve_quant_state(base_layer, W)
    if getattr(proj, "disable_adapters", True) or proj.merged:
        return W, W_quant, None, None, None, base_layer.bias
    adapter = getattr(proj, "active_adapters", None)
    if adapter is None:
        adapter = getattr(proj, "active_adapter", ("default"))
    adapter = adapter[0]
    return (W, W_quant, proj.lora_A[adapter].weight, proj.lora_B[adapter].weight,
            proj.scaling[adapter], base_layer.bias)


@torch.inference_mode()
def fast_dequantize(W, quant_state=None, out=None, use_global_buffer=False):
    """utils.py:567-679. Dense [out,in] weight in quant_state.dtype; passthrough when
    quant_state is None (:578-579); returns the TRANSPOSE when handed `W.t()` of the packed
    storage, i.e. W.shape[0] == 1 (:678-679). With use_global_buffer the result is a view of a
    per-device scratch buffer that the next call overwrites (:608-632)."""
    if quant_state is None:
        return W
    _refuse_fp8([(W,)])
    is_transposed = W.shape[0] == 1
    packed = W.t() if is_transposed else W
    out = _nf4.dequantize_nf4(packed, quant_state, out=out, use_global_buffer=use_global_buffer)
    return out.t() if is_transposed else out


# ------------------------------------------------------------------------------------------------
# GEMM plumbing
def _group(B, C, N, ldb, absmax=None, xa=None, ld_xa=0, lb=None, R=0, scale=0.0, xk=None, bk=None, bias=None):
    # (for uamd_gemm_nn_256 `B` is [K, N] and `bk` is [Rk, N]; the struct is the same)
    """One uamd_gemm_group. The LoRA term comes either as (xa fp32, lb, scale) -- the register prologue of the
    128x128 kernels -- or as the rank block (xk, bk) the 256x256 kernel contracts as extra K tiles; `xa` and `R` are
    kept in both cases (the benchmark's flop accounting reads them)."""
    return GemmGroup(
        B=B.data_ptr(), C=C.data_ptr(), absmax=absmax.data_ptr() if absmax is not None else None,
        lora_xa=xa.data_ptr() if xa is not None else None, lora_b=lb.data_ptr() if lb is not None else None,
        ldb=ldb, ldc=C.stride(0), ld_xa=ld_xa, ld_lb=lb.stride(0) if lb is not None else 0,
        N=N, R=R, lora_scale=float(scale), _pad=0,
        lora_xk=xk.data_ptr() if xk is not None else None, lora_bk=bk.data_ptr() if bk is not None else None,
        ld_xk=xk.stride(0) if xk is not None else 0, ld_bk=bk.stride(0) if bk is not None else 0,
        Rk=xk.shape[1] if xk is not None else 0, _pad2=0, bias=bias.data_ptr() if bias is not None else None)


def _use_gemm256(M, K, Ns):
    """`Ns`: output widths of the groups of one launch."""
    if GEMM256_MODE == "off" or K % 64:
        return False
    if GEMM256_MODE == "on":
        return True
    cols = sum((n + 255) // 256 for n in Ns)
    # 256 x 256 tiles when they fill the chip, else the same kernel family's 128 x 256 tiles (csrc/gemm256.hip picks
    # the height); below that the 128 x 128 register-staged kernel
    return ((M + 255) // 256) * cols >= GEMM256_MIN_TILES or ((M + 127) // 128) * cols >= GEMM256_MIN_TILES


# The 256-tile kernels address every operand through 32-bit byte offsets from its base (csrc/gemm256.hip refuses a launch
# whose A, XK or B would span 4 GiB). A per-row operand past that span -- A = h or [df | de] with ld = 2 I + 64 from ~57 K
# tokens at Qwen2-7B widths, ~75 K at Llama-3-8B's -- is launched as row chunks (NT / NN) or contraction chunks (TN,
# dense_dw) that each stay below it. The limit is applied conservatively to every kernel of _launch_gemm: the 128-tile
# uamd_gemm_nt / uamd_gemm_nt_nf4 (64-bit addressing, no span guard) and the fp32 XA only the 128-tile prologue reads are
# counted too -- at most a few extra launches at sizes no 128-tile launch reaches. A weight B past the span is not split
# (still refused by the kernel's guard). Module attribute: tests lower it to force chunking at small shapes.
GEMM_SPAN_LIMIT = 1 << 32


def _chunk_rows(row_bytes, align):
    """The most rows, a multiple of `align`, whose operand spans less than GEMM_SPAN_LIMIT bytes."""
    rows = (GEMM_SPAN_LIMIT - 1) // max(row_bytes, 1) // align * align
    if rows < align:
        raise RuntimeError(f"unsloth_amd: a GEMM operand row of {row_bytes} bytes leaves no whole {align}-row chunk "
                           f"below the {GEMM_SPAN_LIMIT}-byte span limit")
    return rows


def _row_spans(M, row_bytes, align):
    """[(first row, rows)] of the launches over M operand rows of `row_bytes` bytes: one below GEMM_SPAN_LIMIT, else
    `_chunk_rows` steps (multiples of `align`, the last one short)."""
    if M * row_bytes < GEMM_SPAN_LIMIT:
        return [(0, M)]
    step = _chunk_rows(row_bytes, align)
    return [(r0, min(step, M - r0)) for r0 in range(0, M, step)]


def _launch_gemm(X2d, groups, nf4, accumulate=False, nn=False):
    """`nn`: the groups' B (and rank-block BK) are [K, N] row-major, C = A @ B (uamd_gemm_nn_256); callers check
    `_use_gemm256` first -- only the 256-tile kernel family has that form.
    A launch whose per-row operands (A, the rank block XK, the fp32 XA) span GEMM_SPAN_LIMIT bytes or more is issued as
    row chunks of a multiple of 256 rows (whole tiles of every kernel); below the limit it is exactly one launch."""
    M, K = X2d.shape
    # a LoRA term given as (fp32 XA, LB) -- no rank block -- is the register prologue of the 128 x 128 kernels only
    prologue_lora = any(g.lora_xa and not g.lora_xk for g in groups)
    if nn:
        name = "uamd_gemm_nn_256"
    elif nf4:
        name = "uamd_gemm_nt_nf4"
    elif _use_gemm256(M, K, [g.N for g in groups]) and not prologue_lora:
        name = "uamd_gemm_nt_256"
    else:
        name = "uamd_gemm_nt"
    item = X2d.element_size()
    row_bytes = X2d.stride(0) * item
    for g in groups:
        if g.lora_xk:
            row_bytes = max(row_bytes, g.ld_xk * item)
        if g.lora_xa:
            row_bytes = max(row_bytes, g.ld_xa * 4)
    for r0, rows in _row_spans(M, row_bytes, 256):
        chunk = []
        for g in groups:
            c = GemmGroup.from_buffer_copy(g)
            if r0:                             # C is in the activation dtype; XA is fp32
                c.C += r0 * c.ldc * item
                if c.lora_xk:
                    c.lora_xk += r0 * c.ld_xk * item
                if c.lora_xa:
                    c.lora_xa += r0 * c.ld_xa * 4
            chunk.append(c)
        arr = (GemmGroup * len(chunk))(*chunk)
        _lib.call(name, X2d, ctypes.c_void_p(X2d.data_ptr() + r0 * X2d.stride(0) * item), X2d.stride(0), rows, K, arr,
                  len(chunk), int(accumulate), _lib.dtype_code(X2d.dtype), _lib.stream_of(X2d))
    return name


def _aligned_rows(W):
    """Can the kernels read W [rows, cols] in place? Unit column stride, a row stride of whole 16-byte vectors and a
    16-byte aligned start (what every A / B / XK / BK operand of the C entry points must have)."""
    return W.stride(1) == 1 and W.stride(0) % 8 == 0 and W.data_ptr() % 16 == 0


def _aligned_copy(W, dtype=None):
    """W [rows, cols] in `dtype` (default: its own), dense, in fresh storage. `.contiguous()` alone returns a dense view
    that starts off the 16-byte grid as it is; a new allocation is aligned."""
    Wc = W.to(dtype if dtype is not None else W.dtype).contiguous()
    return Wc.clone() if Wc.data_ptr() % 16 else Wc


def _rows2d(X):
    X2d = X.reshape(-1, X.shape[-1])
    return X2d if _aligned_rows(X2d) else _aligned_copy(X2d)


def _out2d(C, M, N, dtype, name):
    """The caller's output buffer `name` as the [M, N] matrix the GEMM epilogue addresses through `ldc = stride(0)`: the
    activation dtype, unit column stride (any row stride and alignment: the epilogue has a scalar form). Leading dimensions
    are folded when they are dense ([batch, seq, N] as matmul_lora's callers pass it). Anything else is refused here: the
    kernel looks at the pointer and `ldc` alone and would write somewhere else."""
    if not isinstance(C, torch.Tensor) or not C.is_cuda or C.dtype != dtype:
        raise ValueError(f"{name}: expected a {dtype} tensor on the GPU, got {getattr(C, 'dtype', type(C))}")
    C2 = C
    if C.dim() != 2 and C.dim() >= 1 and C.shape[-1] == N and C.numel() == M * N:
        try:
            C2 = C.view(M, N)
        except RuntimeError:
            raise ValueError(f"{name}: shape {tuple(C.shape)} with strides {C.stride()} is no [{M}, {N}] row-major matrix") \
                from None
    if C2.dim() != 2 or tuple(C2.shape) != (M, N):
        raise ValueError(f"{name}: shape {tuple(C.shape)}, expected [{M}, {N}]")
    if N > 1 and C2.stride(1) != 1:
        raise ValueError(f"{name}: column stride {C2.stride(1)}, the GEMM writes rows of unit column stride")
    return C2


# LoRA factors are fp32 parameters used in the activation dtype (utils.py:1166-1167). A training step reads each
# factor up to 3 times (forward, checkpoint recompute, backward): convert once per parameter UPDATE instead of
# once per use. An entry is valid while (a) the parameter object, its _version and its storage are unchanged and
# (b) no optimizer has stepped since (fused optimizers update in place WITHOUT bumping _version, so a global
# optimizer post-step hook and every top-level model forward advance an epoch that invalidates everything).
import weakref
from collections import namedtuple
_CAST_CACHE = {}     # id(param) -> _CastCopies
_CAST_EPOCH = [0]


def invalidate_cast_cache(*_a, **_k):
    _CAST_EPOCH[0] += 1


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_hook
    _reg_hook(invalidate_cast_cache)
except Exception:  # pragma: no cover
    pass


def _stamp(P):
    """What a copy of the factor P was made from -- the object, its _version, its storage and the epoch. The copy is current
    while this is unchanged: the one validity rule of every cache of factor copies (here and kernels/decode.py lora_a_rows)."""
    return (id(P), P._version, P.data_ptr(), _CAST_EPOCH[0])


def _stack_tag(kind, others):
    """Tag of a copy stacked from several factors and cached on the first of them: the stamps of the others."""
    return (kind,) + tuple(_stamp(A) for A in others)


# The copies of one factor in _CAST_CACHE, which is keyed on id(P): `ref` (a weakref) guards against a recycled id, `stamp` is
# the `_stamp` they were made at, `copies` = {(tag, dtype): tensor}.
class _CastCopies:
    __slots__ = ("ref", "stamp", "copies")

    def __init__(self, P, pid):
        self.ref, self.stamp, self.copies = weakref.ref(P, lambda _: _CAST_CACHE.pop(pid, None)), _stamp(P), {}


# The copies of one factor in _PreparedFactors.params (keyed on id(P) too): row-major `rm`, transposed `tr` and, with
# `pad` = (buffer, offset, scale, transposed), a scaled one inside a rank-block BK buffer. `stamp`: the `_stamp` of the last
# uamd_lora_prepare launch that wrote them (None: to be written).
class _Prepared:
    __slots__ = ("ref", "stamp", "rm", "tr", "pad")

    def __init__(self, P, ref, dtype):
        self.ref, self.stamp, self.pad = ref, None, None
        self.rm = torch.empty(P.shape, dtype=dtype, device=P.device)
        self.tr = torch.empty((P.shape[1], P.shape[0]), dtype=dtype, device=P.device)


# The descriptor table of the last multi-factor uamd_lora_prepare launch: the descriptor bytes, the two device tensors the
# kernel reads, its tile count, and the identity key of the entries it was built from.
_PrepTable = namedtuple("_PrepTable", "sig descs prefix tiles key")


class _PreparedFactors:
    """Per (device, dtype): activation-dtype row-major + transposed copies of every LoRA factor seen so far,
    refreshed by ONE `uamd_lora_prepare` launch per optimizer step (epoch)."""

    def __init__(self, device, dtype):
        self.device, self.dtype = device, dtype
        self.params = {}        # id -> _Prepared
        self.pad_bufs = {}      # key -> zero-initialised [rows, width] buffer (rank-block BK operands of the GEMM)
        self.epoch = -1
        self.table = None       # _PrepTable

    @staticmethod
    def _tiles(P):
        return ((P.shape[0] + 31) // 32) * ((P.shape[1] + 31) // 32)

    _DESC = [("src", "<u8"), ("rm", "<u8"), ("tr", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("pad", "<u8"),
             ("pad_ld", "<i8"), ("pad_scale", "<f4"), ("pad_t", "<i4")]          # uamd_lora_prep_desc

    def _launch(self, ents):
        import numpy as np                  # ents: [(P, its _Prepared)]
        # the table only changes when a factor / copy / pad buffer moves: a cheap identity key first, the numpy
        # descriptor build (1.2 ms of host time for 448 factors -- visible at 2048 tokens per step, where the host is
        # barely ahead of the GPU) only on a miss
        key = tuple((P.data_ptr(), P.shape[0], P.shape[1], e.rm.data_ptr(), e.tr.data_ptr(),
                     None if e.pad is None else (e.pad[0].data_ptr(), e.pad[0].stride(0)) + tuple(e.pad[1:]))
                    for (P, e) in ents) if len(ents) > 1 else None
        tab = self.table
        if key is None or tab is None or tab.key != key:
            descs = np.zeros(len(ents), dtype=np.dtype(self._DESC))
            assert descs.dtype.itemsize == 56
            prefix, tot = np.zeros(len(ents), dtype=np.int32), 0
            for i, (P, e) in enumerate(ents):
                pad = (0, 0, 0.0, 0)
                if e.pad is not None:
                    buf, col, scale, transposed = e.pad
                    pad = (buf.data_ptr() + col * buf.element_size(), buf.stride(0), scale, int(transposed))
                descs[i] = (P.data_ptr(), e.rm.data_ptr(), e.tr.data_ptr(), P.shape[0], P.shape[1]) + pad
                prefix[i] = tot
                tot += self._tiles(P)
            sig = descs.tobytes()
            if tab is None or tab.sig != sig:
                d = torch.from_numpy(descs.view(np.uint8).copy()).to(self.device)
                pf = torch.from_numpy(prefix).to(self.device)
                tab = _PrepTable(sig, d, pf, tot, key)
            else:                                   # same descriptors under a new identity key
                tab = tab._replace(key=key)
            if len(ents) > 1:                       # (a single-entry launch never matches the stored table's bytes)
                self.table = tab
        any_p = ents[0][0]
        # the table tensors must outlive the launch: stream-ordered free is fine for torch's caching allocator
        _lib.call("uamd_lora_prepare", any_p, _lib.ptr(tab.descs), _lib.ptr(tab.prefix), len(ents), tab.tiles,
                  _lib.dtype_code(self.dtype), _lib.stream_of(any_p))

    def _forget(self, pid):
        self.params.pop(pid, None)
        for k in [k for k in self.pad_bufs if pid in k[0]]:
            self.pad_bufs.pop(k, None)

    def _entry(self, P, padspec=None):
        """Registers P (and, optionally, its padded/scaled third copy) and makes every copy current."""
        pid = id(P)
        ent = self.params.get(pid)
        with torch.no_grad():
            if ent is None or ent.ref() is not P or ent.rm.shape != P.shape:
                ent = self.params[pid] = _Prepared(P, weakref.ref(P, lambda _, pid=pid: self._forget(pid)), self.dtype)
            if padspec is not None:
                old = ent.pad
                if old is None or old[0] is not padspec[0] or old[1:] != padspec[1:]:
                    ent.pad, ent.stamp = padspec, None         # this entry must be (re)written
            if self.epoch != _CAST_EPOCH[0]:
                live = []
                for e in list(self.params.values()):
                    Q = e.ref()
                    if Q is not None:
                        live.append((Q, e))
                        e.stamp = _stamp(Q)
                self._launch(live)
                self.epoch = _CAST_EPOCH[0]
            elif ent.stamp != _stamp(P):                        # registered (or modified in place) mid-epoch
                self._launch([(P, ent)])
                ent.stamp = _stamp(P)
        return ent

    def get(self, P, tag):
        ent = self._entry(P)
        return ent.rm if tag == "rowmajor" else ent.tr

    def get_pad(self, members, rows, width, transposed, by_rows=False):
        """members: [(P, off, scale)] written into ONE zero-initialised [rows, width] buffer: scale * P
        (transposed=False) or scale * P^T (transposed=True), side by side at COLUMN `off` (by_rows=False) or stacked
        at ROW `off` (by_rows=True). Returns the buffer: the BK operand of the GEMM's rank-block K tiles
        ([N, Rk] for the NT form, [Rk, N] for the NN form)."""
        key = (tuple(id(P) for P, _, _ in members), rows, width, bool(transposed), bool(by_rows))
        buf = self.pad_bufs.get(key)
        if buf is None:
            buf = self.pad_bufs[key] = torch.zeros((rows, width), dtype=self.dtype, device=self.device)
        for P, off, scale in members:
            self._entry(P, (buf, int(off) * (width if by_rows else 1), float(scale), bool(transposed)))
        return buf


_PREPARED = {}


def _preparable(P, dtype):
    """The factors `uamd_lora_prepare` keeps current: fp32 CUDA Parameters (the training case) used in a 16-bit dtype."""
    return (isinstance(P, torch.nn.Parameter) and P.is_cuda and P.dtype == torch.float32 and P.dim() == 2
            and P.is_contiguous() and dtype in (torch.bfloat16, torch.float16))


def _prepared_for(device, dtype):
    g = _PREPARED.get((device, dtype))
    if g is None:
        g = _PREPARED[(device, dtype)] = _PreparedFactors(device, dtype)
    return g


def _cached_cast(P, tag, dtype, build):
    if not isinstance(P, torch.nn.Parameter):
        return build()
    if tag in ("rowmajor", "T") and _preparable(P, dtype):
        return _prepared_for(P.device, dtype).get(P, tag)
    pid = id(P)
    ent = _CAST_CACHE.get(pid)
    if ent is None or ent.ref() is not P or ent.stamp != _stamp(P):
        ent = _CAST_CACHE[pid] = _CastCopies(P, pid)
    key = (tag, dtype)
    out = ent.copies.get(key)
    if out is None:
        with torch.no_grad():
            out = build()
        ent.copies[key] = out
    return out


def rank_block_bk(members, rows, width, transposed, dtype, by_rows=False):
    """BK operand of the GEMM's rank-block K tiles: a zero [rows, width] buffer with scale * P (or scale * P^T when
    `transposed`) at columns col_off.. for every member (P, col_off, scale). When the factors are fp32 CUDA
    Parameters (the training case) the buffer is persistent and kept current by the once-per-step
    uamd_lora_prepare launch; otherwise it is built here."""
    if not all(_preparable(P, dtype) for P, _, _ in members):
        # plain tensors (tests, ad-hoc calls of matmul_lora): built per call with torch ops
        with torch.no_grad():
            buf = torch.zeros((rows, width), dtype=dtype, device=members[0][0].device)
            for P, off, scale in members:
                src = P.detach().t() if transposed else P.detach()
                val = (src.float() * float(scale)).to(dtype)
                if by_rows:
                    buf[off:off + src.shape[0], :src.shape[1]] = val
                else:
                    buf[:, off:off + src.shape[1]] = val
        return buf
    return _prepared_for(members[0][0].device, dtype).get_pad(members, rows, width, transposed, by_rows)


def cast_lora(P, dtype):
    """P.to(dtype) (row-major, contiguous), converted once per parameter version."""
    return _cached_cast(P, "rowmajor", dtype, lambda: P.to(dtype).contiguous())


def cast_lora_t(P, dtype):
    """P.to(dtype).t() as a contiguous [cols, rows] matrix, converted once per parameter version."""
    return _cached_cast(P, "T", dtype, lambda: P.to(dtype).t().contiguous())


def _pad_rank(B, Rp, dtype):
    """LoRA B [N, r] -> contiguous [N, Rp] in the activation dtype (B.to(dtype), utils.py:1167)."""
    N, r = B.shape
    if r == Rp:
        return cast_lora(B, dtype)
    out = torch.zeros((N, Rp), dtype=dtype, device=B.device)
    out[:, :r] = B
    return out


def _features(W, q):
    """(N, K) = (out, in) features of a projection: off the quant state when the weight is packed NF4."""
    shape = q.shape if q is not None else W.shape
    return shape[0], shape[1]


# The rank term of one projection, forward (P = X A^T) or backward (P = dY B). `P`: fp32 [M, Rp] view, unit column stride;
# `xk`: the 16-bit zero-padded rank block P was also written to (the XK operand the 256-tile GEMMs contract as extra K tiles)
# or None; `col`: P's first column in it.
RankTerm = namedtuple("RankTerm", "P xk col", defaults=(None, 0))


# ------------------------------------------------------------------------------------------------
# rank columns: which launches form the P of the factors of one block, and where they land
def _pad8(r):                           # every factor's P takes whole 8-rank blocks of columns
    return (r + 7) // 8 * 8


def _rank_width(r):                     # columns of a rank block: whole K tiles of the GEMM
    return (r + 63) // 64 * 64


def _streams(r):
    """A rank the streaming kernels (uamd_lora_xa2 / xa2k, the fused gated activations) take: unpadded, one launch."""
    return 0 < r <= LORA_XA2_MAX_RANKS and r == _pad8(r)


def _share_block(ranks):
    """Ranks whose P the streaming kernel can write side by side into ONE rank block: one launch's worth of padded columns, or
    up to three launches' worth of whole unpadded factors."""
    Rt = sum(_pad8(r) for r in ranks)
    return Rt <= LORA_XA2_MAX_RANKS or (Rt <= LORA_XA_MAX_RANKS and all(_streams(r) for r in ranks))


# One launch of a plan. entry: uamd_lora_xa | uamd_lora_xa2 | uamd_lora_xa2k; members: the factors whose stacked rows it reads
# (indices into the plan's ranks); col: the first rank column it writes, of P and of the rank block; cols: rank columns;
# k_cols: (uamd_lora_xa2k, else None) rank-block columns written from `col` on -- `cols`, then zeros.
XaLaunch = namedtuple("XaLaunch", "entry members col cols k_cols")
# ranks: as given (None: a projection without an adapter); widths: padded columns of each P (None likewise); starts: first rank
# column of each; total: rank columns of all; shared: the Ps are column blocks of ONE fp32 buffer; launches: XaLaunch in launch
# order; block: columns of the ONE rank block the launches write (0: none); casts: [(members, width)] -- a padded cast of their
# P columns into a rank block of their own follows.
RankPlan = namedtuple("RankPlan", "ranks widths starts total shared launches block casts")


@functools.lru_cache(maxsize=None)
def _rank_plan(ranks, K, want_k, one_input=True, v2=True):
    """The X @ A^T (forward) or dY @ B (backward) launches of one block. Pure -- tuples in, no tensors, no launches, no module
    switches (`v2` is LORA_XA_V2) -- so every distinct block of a model is planned once.
    `one_input` (forward): the factors share an input of K columns, their Ps sit side by side and one launch may take
    several of them. Else (backward) factor i has an input of K[i] columns and a launch of its own; rank None = no adapter.
    `want_k`: the GEMM will take a rank block. The streaming kernel writes it when the ranks can share one (_share_block) -- in
    the backward only when the Ps share a buffer too, or there is just one; else a padded cast per unit follows."""
    n = len(ranks)
    Ks = (K,) * n if one_input else K
    widths = [None if r is None else _pad8(r) for r in ranks]
    idx = [i for i in range(n) if ranks[i] is not None]
    starts = [sum(w or 0 for w in widths[:i]) for i in range(n)]
    Rt = sum(w or 0 for w in widths)
    span = lambda g: sum(widths[i] for i in g)
    shared = one_input or (n > 1 and len(idx) == n and all(r == _pad8(r) for r in ranks))
    units = [idx] if one_input else [[i] for i in idx]          # the factors a launch may take together
    block = (want_k and bool(idx) and _share_block([ranks[i] for i in idx])
             and ((v2 and K >= 8) if one_input else (shared or len(idx) == 1)))
    launches, width = [], _rank_width(Rt) if block else 0
    if block:
        # <= LORA_XA2_MAX_RANKS rank columns per launch: whole factors in greedy groups, each launch writing its own columns
        # of the shared buffers, the last one zero-filling the block's padding
        groups = []
        for i in idx:
            if one_input and groups and span(groups[-1]) + widths[i] <= LORA_XA2_MAX_RANKS:
                groups[-1].append(i)
            else:
                groups.append([i])
        for g in groups:
            col, cols = starts[g[0]], span(g)
            launches.append(XaLaunch("uamd_lora_xa2k", tuple(g), col, cols, width - col if g is groups[-1] else cols))
    else:
        # one launch per unit; past LORA_XA_MAX_RANKS (r = 128 on gate|up or q|k|v) in chunks of its stacked rows
        for u in units:
            for o in range(0, span(u), LORA_XA_MAX_RANKS):
                cols = min(LORA_XA_MAX_RANKS, span(u) - o)
                name = "uamd_lora_xa2" if (v2 and cols <= LORA_XA2_MAX_RANKS and Ks[u[0]] >= 8) else "uamd_lora_xa"
                launches.append(XaLaunch(name, tuple(u), starts[u[0]] + o, cols, None))
    casts = [(tuple(u), _rank_width(span(u))) for u in units] if (want_k and not block) else []
    return RankPlan(ranks, tuple(widths), tuple(starts), Rt, shared, tuple(launches), width, tuple(casts))


def _padded_cast(P, width, dtype):
    """P (fp32 [M, R]) as a rank block of its own, with torch ops: where the streaming kernel writes none (_rank_plan)."""
    xk = torch.zeros((P.shape[0], width), dtype=dtype, device=P.device)
    xk[:, :P.shape[1]] = P
    return xk


def _stacked_rows(plan, members, rows, params, X2d):
    """[sum widths, K] in the activation dtype: the rows of the factors `members`, each zero-padded to its width."""
    exact = all(plan.ranks[i] == plan.widths[i] for i in members)
    if len(members) == 1 and exact:
        return rows(members[0], False)

    def build():
        if exact:
            return torch.cat([rows(i, False) for i in members], dim=0)
        buf = torch.zeros((sum(plan.widths[i] for i in members), X2d.shape[1]), dtype=X2d.dtype, device=X2d.device)
        for i in members:
            o = plan.starts[i] - plan.starts[members[0]]
            buf[o:o + plan.ranks[i]] = rows(i, True)
        return buf
    if params is not None and all(isinstance(params[i], torch.nn.Parameter) for i in members):
        return _cached_cast(params[members[0]], _stack_tag("cat", [params[i] for i in members[1:]]), X2d.dtype, build)
    return build()


def _rank_terms(plan, Xs, rows, params=None, out=None, xk=None):
    """Executes `plan`: [RankTerm | None] per factor. Xs[i]: the 2-D input of factor i; rows(i, padded): its [r, K] rows in the
    activation dtype (A.to(dtype), utils.py:1166) or, when `padded`, in any, to be copied into a zero-padded stack; `params`:
    the factors when a stack of Parameters may be cached on the first; `out` / `xk`: the caller's shared P buffer / rank block."""
    if not plan.total:
        return [None] * len(plan.widths)
    X0 = Xs[plan.launches[0].members[0]]
    M, dtype, dev = X0.shape[0], X0.dtype, X0.device
    if plan.block and xk is None:
        xk = torch.empty((M, plan.block), dtype=dtype, device=dev)
    if not plan.shared:
        Ps = [None if w is None else torch.empty((M, w), dtype=torch.float32, device=dev) for w in plan.widths]
    else:
        if out is None:
            out = torch.empty((M, plan.total), dtype=torch.float32, device=dev)
        else:
            assert out.dtype == torch.float32 and tuple(out.shape) == (M, plan.total) and out.stride(1) == 1 and out.stride(0) % 4 == 0
        Ps = [None if w is None else out[:, c:c + w] for c, w in zip(plan.starts, plan.widths)]
    of = None
    for entry, members, col, cols, k_cols in plan.launches:
        X2d, P = Xs[members[0]], Ps[members[0]]
        if members != of:
            S, of = _stacked_rows(plan, members, rows, params, X2d), members
            if S.shape[0] > LORA_XA_MAX_RANKS and not _aligned_rows(S):         # read in row chunks: each from an aligned start
                S = _aligned_copy(S)
        o = col - plan.starts[members[0]]
        args = [_lib.ptr(X2d), X2d.stride(0), ctypes.c_void_p(S.data_ptr() + o * S.stride(0) * S.element_size()), S.stride(0),
                ctypes.c_void_p(P.data_ptr() + 4 * o), P.stride(0)]
        if k_cols is not None:
            args += [ctypes.c_void_p(xk.data_ptr() + col * xk.element_size()), xk.stride(0), k_cols]
        _lib.call(entry, X2d, *args, M, X2d.shape[1], cols, cols, _lib.dtype_code(dtype), _lib.stream_of(X2d))
    if not plan.casts:
        return [None if P is None else RankTerm(P, xk, c) for P, c in zip(Ps, plan.starts)]
    terms = list(Ps)
    for members, width in plan.casts:
        c0, last = plan.starts[members[0]], members[-1]
        own = _padded_cast(out[:, c0:plan.starts[last] + plan.widths[last]] if plan.shared else Ps[last], width, dtype)
        for i in members:
            terms[i] = RankTerm(Ps[i], own, plan.starts[i] - c0)
    return terms


def _factor_rows(A_list, dtype):
    return lambda i, padded: A_list[i] if padded else cast_lora(A_list[i], dtype)


def lora_xa(X2d, A_list, out=None, out_k=None, k_cols=0):
    """XA_g = X @ A_g^T for every projection sharing X, ONE launch (one per LORA_XA_MAX_RANKS rank columns past
    that width). fp32, each block of columns padded to a multiple of 8. Returns (buffer, [(col_offset, R_padded)]).
    `out`: optional fp32 [M, sum Rp] destination with unit column stride (e.g. a column slice of a wider buffer). `out_k`
    (activation dtype, unit column stride) additionally receives the sums rounded to the activation dtype, zero-filled up to
    `k_cols` columns: the XK operand of the GEMM's rank-block K tiles."""
    plan = _rank_plan(tuple(A.shape[0] for A in A_list), X2d.shape[1], False, v2=LORA_XA_V2)
    if out_k is not None:
        assert plan.total <= LORA_XA2_MAX_RANKS and out_k.dtype == X2d.dtype and out_k.stride(1) == 1 and k_cols >= plan.total
        plan = plan._replace(launches=(XaLaunch("uamd_lora_xa2k", tuple(range(len(A_list))), 0, plan.total, k_cols),))
    if out is None:
        out = torch.empty((X2d.shape[0], plan.total), dtype=torch.float32, device=X2d.device)
    _rank_terms(plan, [X2d] * len(A_list), _factor_rows(A_list, X2d.dtype), A_list, out=out, xk=out_k)
    return out, list(zip(plan.starts, plan.widths))


def _xa_and_rank_block(X2d, A_list, want_k):
    """[RankTerm] of X @ A_g^T for the projections sharing X: column blocks of one fp32 [M, sum Rp] buffer and, when `want_k`,
    of one rank block (the same sums in the activation dtype, zero-padded to a multiple of 64 columns)."""
    plan = _rank_plan(tuple(A.shape[0] for A in A_list), X2d.shape[1], bool(want_k), v2=LORA_XA_V2)
    return _rank_terms(plan, [X2d] * len(A_list), _factor_rows(A_list, X2d.dtype), A_list)


def _fused_nf4(q, M, K):
    """Does a forward launch of M rows decode this weight inside the GEMM (uamd_gemm_nt_nf4)? Part of
    _forward_wants_rank_block, where lora_linear_forward and the kernel that prepares its rank block (glu_fwd_xa) agree."""
    return q is not None and FUSED_NF4 and M < FUSED_NF4_MAX_M and q.blocksize == 64 and K % 64 == 0


def _forward_wants_rank_block(M, K, projs):
    """Does the forward launch of `projs` on an [M, K] input take its LoRA terms as a rank block? Its dense groups (NF4 not
    decoded in the GEMM) go to the 256x256 kernel when the launch is large enough: there the LoRA term rides along as extra K
    tiles. lora_linear_forward launches by this answer; glu_fwd_xa, which hands it X A^T, writes the rank block by the same."""
    dense = [_features(p[0], p[1])[0] for p in projs if not _fused_nf4(p[1], M, K)]
    return bool(dense) and _use_gemm256(M, K, dense)


def _dx_wants_rank_block(M, projs):
    """Should the producers of the dX rank terms (lora_dx_terms, glu_bwd_terms, glu_bwd_tn) also write a rank block? When the
    dX GEMM of every projection could run on the 256-tile family, asked at a nominal 64 output features. _dx_gemm, which has
    the real dY in hand, takes the block when `_use_gemm256(M, N, [Kin])` holds for it: with a dY whose width N is no multiple
    of 64 the block is written here and not used there (the 128-tile prologue runs)."""
    return all(_use_gemm256(M, 64, [_features(p[0], p[1])[1]]) for p in projs)


def _decoded_as(Wd, dtype):
    if Wd.dtype != dtype:
        raise TypeError(f"quant_state.dtype {Wd.dtype} != activation dtype {dtype}: the dequantised weight would be "
                        "misread by the GEMM (set quant_state.dtype to the compute dtype)")
    return Wd


def _forward_weight_operands(projs, M, K, dtype, device):
    """Per projection of ONE forward launch, the twin of _dx_weight: None -- NF4 decoded inside the GEMM (_fused_nf4) -- or the
    dense [N, K] operand: the member of the mirror group when every projection keeps a mirror, else its scratch slot (8 + its
    index) filled by ONE grouped decode launch or a launch of its own, or the dense weight as is or as an aligned copy."""
    Ws, qs = [p[0] for p in projs], [p[1] for p in projs]
    fused = [_fused_nf4(q, M, K) for q in qs]
    if len(projs) > 1 and not any(fused) and all(q is not None and _nf4.mirror_wanted(q) for q in qs):
        return list(_nf4.resident_group(Ws, qs)[1])
    decoded = {}
    todo = [gi for gi, q in enumerate(qs) if q is not None and not fused[gi]]
    if len(todo) > 1 and all(qs[gi].dtype == dtype and qs[gi].quant_type == "nf4" for gi in todo):
        slots = [_nf4.scratch(device, qs[gi].shape[0] * qs[gi].shape[1], dtype, slot=8 + gi).view(tuple(qs[gi].shape))
                 for gi in todo]
        _nf4.dequantize_nf4_group([Ws[gi] for gi in todo], [qs[gi] for gi in todo], slots)
        decoded = dict(zip(todo, slots))

    def own(gi, W, q):
        if q is not None:
            return _decoded_as(_nf4.dequantize_nf4(W, q, use_global_buffer=True, slot=8 + gi), dtype)
        return W if (W.dtype == dtype and _aligned_rows(W)) else _aligned_copy(W, dtype)
    return [None if fused[gi] else decoded[gi] if gi in decoded else own(gi, Ws[gi], qs[gi]) for gi in range(len(projs))]


def _forward_rank_term(term, B, s, N, fused, dtype):
    """`_group` keywords of the rank term s (X A^T) B^T of one forward group, the twin of _dx_rank_term: BK = T(s B) at the
    term's columns of its rank block, or -- no block, or NF4 decoded in the GEMM (`fused`) -- LB = T(B) for the prologue."""
    P, xk = term.P, term.xk
    if xk is not None and not fused:
        return dict(xa=P, ld_xa=P.stride(0), R=P.shape[1], scale=s, xk=xk,
                    bk=rank_block_bk([(B, term.col, s)], N, xk.shape[1], False, dtype))
    return dict(xa=P, ld_xa=P.stride(0), R=P.shape[1], scale=s, lb=_pad_rank(B, P.shape[1], dtype))


def lora_linear_forward(X, projs, outs=None, return_xa=False, pre_xa=None):
    """Y_g = X @ W_g^T + s_g * (X @ A_g^T) @ B_g^T for projections `projs` = [(W, W_quant, A, B, s)]
    that share X. Returns a list of [.., N_g] tensors. This is matmul_lora (utils.py:1128-1170)
    for q/k/v or gate/up at once. `pre_xa`: the [RankTerm] of the adapters when the kernel that produced X formed them
    (glu_fwd_xa). `return_xa`: also the fp32 [M, Rp] views of X @ A_g^T (None without adapter), kept for d_B = s dY^T (X A^T)."""
    _refuse_fp8(projs)
    _lib.require_gpu(X)
    dtype = X.dtype
    if dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError("the MFMA GEMM path takes bf16/fp16 activations")
    X2d = _rows2d(X)
    M, K = X2d.shape
    factors = [p[2] for p in projs if p[2] is not None]
    want_k = _forward_wants_rank_block(M, K, projs)
    if factors and (pre_xa is None or (pre_xa[0].xk is not None) != want_k):
        # (a handed-over X A^T must come with its rank block iff this launch wants it)
        pre_xa = _xa_and_rank_block(X2d, factors, want_k)
    terms = iter(pre_xa or ())
    operands = _forward_weight_operands(projs, M, K, dtype, X.device)
    results, views, dense_groups, nf4_groups, keep = [], [], [], [], []
    for gi, (p, Wd) in enumerate(zip(projs, operands)):
        W, W_quant, A, B, s = p[:5]
        N = _features(W, W_quant)[0]
        assert W_quant is None or W_quant.shape[1] == K, "weight/in_features mismatch"
        C = _out2d(outs[gi], M, N, dtype, f"outs[{gi}]") if outs is not None else torch.empty((M, N), dtype=dtype, device=X.device)
        kw = {}
        # a projection may carry the base layer's bias as a 6th element (get_lora_parameters_bias order): it is added in the
        # GEMM epilogue, in fp32, before the single rounding (Qwen2's q/k/v; the reference leaves such layers un-fused)
        if len(p) > 5 and p[5] is not None:
            bias = p[5].detach()
            if bias.dtype != dtype or not bias.is_contiguous():
                bias = bias.to(dtype).contiguous()
            assert bias.numel() == N
            kw["bias"] = bias
        term = next(terms) if A is not None else None
        views.append(term.P if term is not None else None)
        if term is not None:
            kw.update(_forward_rank_term(term, B, s, N, Wd is None, dtype))
        keep += [kw, Wd]                # (the groups hold addresses only)
        if Wd is None:
            nf4_groups.append(_group(W, C, N, 0, absmax=_nf4.absmax_f32(W_quant), **kw))
        else:
            dense_groups.append(_group(Wd, C, N, Wd.stride(0), **kw))
        results.append(C.view(*X.shape[:-1], N))
    if nf4_groups:
        _launch_gemm(X2d, nf4_groups, nf4=True)
    if dense_groups:
        _launch_gemm(X2d, dense_groups, nf4=False)
    return (results, views) if return_xa else results


def lora_dx_terms(dYs, projs):
    """The RankTerm of P_g = dY_g @ B_g for every projection with an adapter (None otherwise): the rank-r factor shared by
    dX += s (dY B) A and by d_A = s (dY B)^T X (fast_lora.py:172-189). All P_g sit side by side in ONE buffer when possible:
    lora_linear_dx can then hand them to a single K-concatenated GEMM. With their rank block by _dx_wants_rank_block."""
    dY2 = [_rows2d(dY) for dY in dYs]
    M, dtype = dY2[0].shape[0], dY2[0].dtype
    want_k = dtype in (torch.bfloat16, torch.float16) and LORA_XA_V2 and _dx_wants_rank_block(M, projs)
    plan = _rank_plan(tuple(None if p[2] is None else p[2].shape[0] for p in projs), tuple(dY.shape[1] for dY in dY2), want_k,
                      one_input=False, v2=LORA_XA_V2)
    return _rank_terms(plan, dY2, lambda i, padded: cast_lora_t(projs[i][3], dtype))         # rows of B^T [r, N]


def _adjacent_columns(ts):
    """The 2-D views `ts` are consecutive column blocks of one row-major buffer -> the [M, sum N] view, else None."""
    t0 = ts[0]
    off = 0
    for t in ts:
        if (t.dim() != 2 or t.stride(1) != 1 or t.stride(0) != t0.stride(0) or t.shape[0] != t0.shape[0]
                or t.dtype != t0.dtype or t.device != t0.device
                or t.data_ptr() != t0.data_ptr() + off * t0.element_size()):
            return None
        off += t.shape[1]
    if off > t0.stride(0):
        return None
    return torch.as_strided(t0, (t0.shape[0], off), (t0.stride(0), 1))


def _dx_weight(projs, nn, dtype):
    """The weight operand of ONE dX launch over `projs`: [sum N, Kin], the rows as the forward decodes them (`nn`), or
    its transpose [Kin, sum N] (NT form). Several projections (the K-concatenated launch; all NF4 in the activation
    dtype, the caller checked) are stacked in that order: the mirror group when every member keeps a mirror, else decoded
    into scratch slot 2. One projection: its mirror / the per-device decode buffer, or the dense weight as is or cast."""
    Ws, qs = [p[0] for p in projs], [p[1] for p in projs]
    if len(projs) > 1:
        Kin = qs[0].shape[1]
        ends = [0]
        for q in qs:
            ends.append(ends[-1] + q.shape[0])
        if nn and all(_nf4.mirror_wanted(q) for q in qs):
            # (the group is keyed on the members in THIS order; the forward of gate|up caches it as [gate, up] while the
            # MLP backward asks for [up, gate] -- a second stacked mirror. Ordering the members here, in this one place, is
            # the fix; it changes memory with mirrors on and so is not part of a behaviour-preserving change)
            Wd, _ = _nf4.resident_group(Ws, qs)
        elif nn:
            Wd = _nf4.scratch(Ws[0].device, ends[-1] * Kin, dtype, slot=2).view(ends[-1], Kin)
            _nf4.dequantize_nf4_group(Ws, qs, [Wd[a:b] for a, b in zip(ends, ends[1:])])
        else:
            Wd = _nf4.scratch(Ws[0].device, Kin * ends[-1], dtype, slot=2).view(Kin, ends[-1])
            for W, q, a, b in zip(Ws, qs, ends, ends[1:]):
                _nf4.dequantize_nf4(W, q, out=Wd[:, a:b], transpose=True)             # [Kin, n] at column `a`
    elif qs[0] is not None:
        Wd = _nf4.dequantize_nf4(Ws[0], qs[0], transpose=not nn, use_global_buffer=True)
    elif nn:
        W = Ws[0]
        Wd = W if (W.dtype == dtype and _aligned_rows(W)) else _aligned_copy(W, dtype)
    else:
        Wd = Ws[0].to(dtype).t().contiguous()
    return _decoded_as(Wd, dtype)


def _dx_rank_term(members, xa, xk, nn, Kin, dtype):
    """`_group` keywords of the rank term xa @ [s_1 A_1; s_2 A_2; ...] of a dX launch. `members` = [(A, column of its
    P = dY B in `xa` / `xk`, s)]. With the rank block `xk` (the 256-tile kernels' extra K tiles) BK holds s A at its rank
    rows (NN form) or s A^T at its rank columns (NT); without it the fp32 `xa` and LB = [A_1^T | A_2^T | ...] go to the
    128-tile kernels' prologue, which has one scale per launch: None when the members' scales differ."""
    kw = dict(xa=xa, ld_xa=xa.stride(0), R=xa.shape[1])
    if xk is not None:
        if nn:
            bk = rank_block_bk(members, xk.shape[1], Kin, False, dtype, by_rows=True)      # [Rk, Kin]
        else:
            bk = rank_block_bk(members, Kin, xk.shape[1], True, dtype)                     # [Kin, Rk]
        # (the scales are in BK; only the prologue reads the group's own)
        return dict(kw, scale=members[0][2] if len(members) == 1 else 1.0, xk=xk, bk=bk)
    scales = {float(s) for _, _, s in members}
    if len(scales) != 1:
        return None
    A_list = [A for A, _, _ in members]
    if len(A_list) > 1:
        lb = _cached_cast(A_list[0], _stack_tag("catT", A_list[1:]), dtype,
                          lambda: torch.cat([cast_lora_t(A, dtype) for A in A_list], dim=1).contiguous())
    elif A_list[0].shape[0] == xa.shape[1]:
        lb = cast_lora_t(A_list[0], dtype)                                                 # A^T [Kin, r]
    else:
        lb = _pad_rank(A_list[0].to(dtype).t(), xa.shape[1], dtype)
    return dict(kw, lb=lb, scale=scales.pop())


def _dx_gemm(dY2d, projs, terms, xa, out, accumulate):
    """out (+)= dY2d @ [W_1; W_2; ...] + xa @ [s_1 A_1; s_2 A_2; ...]: one GEMM over the (concatenated) output features
    of `projs`. `terms` = per projection its RankTerm (P = dY B) or None, `xa` = the [M, sum r] view of all the Ps (None
    without an adapter). The NN form of the 256-tile family (no transposed copy of any weight) when the launch is large enough
    for it and every rank term has its rank block, else a transposed decode and the NT form. The producers of the terms wrote
    the blocks by _dx_wants_rank_block's guess of the answer given here. Returns `out`, or None when the rank term cannot go in
    one launch."""
    M, N = dY2d.shape
    dtype = dY2d.dtype
    Kin = _features(*projs[0][:2])[1]
    if out is not None:
        out = _out2d(out, M, Kin, dtype, "out")
    lora = [(p[2], p[4], t) for p, t in zip(projs, terms) if p[2] is not None]
    have_xk = all(t.xk is not None and t.xk is lora[0][2].xk for _, _, t in lora)      # ONE block shared by all of them
    use256 = _use_gemm256(M, N, [Kin])
    nn = use256 and Kin % 8 == 0 and have_xk
    Wd = _dx_weight(projs, nn, dtype)
    if out is None:
        out = torch.empty((M, Kin), dtype=dtype, device=dY2d.device)
    kw = {}
    if lora:
        block = lora[0][2].xk if (have_xk and use256) else None
        members = [(A, t.col if block is not None else 0, s) for A, s, t in lora]
        kw = _dx_rank_term(members, xa, block, nn, Kin, dtype)
        if kw is None:
            return None
    _launch_gemm(dY2d, [_group(Wd, out, Kin, Wd.stride(0), **kw)], nf4=False, accumulate=accumulate, nn=nn)
    return out


def _lora_linear_dx_merged(dYs, projs, out, terms):
    """dX = [dY_1 | dY_2 | ...] @ [W_1; W_2; ...] + s [P_1 | P_2 | ...] @ [A_1; A_2; ...] as ONE GEMM when the
    incoming gradients are column blocks of one buffer (the attention backward writes dQ, dK, dV that way): the
    contraction simply runs over the concatenated output features. Saves the read-modify-write of dX per extra
    projection and the short-K launches (k_proj / v_proj: K = 1024). Returns None when the shapes do not allow it."""
    if len(dYs) < 2 or any(p[1] is None or p[2] is None for p in projs) or any(t is None for t in terms):
        return None
    dYcat = _adjacent_columns([_rows2d(dY) for dY in dYs])
    Pcat = _adjacent_columns([t.P for t in terms])
    if dYcat is None or Pcat is None or dYcat.shape[1] % 64 or dYcat.stride(0) % 8:
        return None
    Kin = projs[0][1].shape[1]
    if any(q.shape[1] != Kin or q.dtype != dYcat.dtype for (_, q, _, _, _) in projs):
        return None
    return _dx_gemm(dYcat, projs, terms, Pcat, out, False)


def lora_linear_dx(dYs, projs, out=None, terms=None):
    """dX = sum_g dY_g @ W_g + s_g * (dY_g @ B_g) @ A_g   (fast_lora.py:193-204, 497-517, 639-647): one GEMM over all
    projections when they allow it (_lora_linear_dx_merged), else one per projection, each after the first accumulating.
    `out` (e.g. the saved X, reference's inplace=True) receives the result. `terms` = lora_dx_terms(dYs, projs) when the
    caller already has them."""
    projs = [tuple(p[:5]) for p in projs]
    _refuse_fp8(projs)
    if terms is None:
        terms = lora_dx_terms(dYs, projs)
    merged = _lora_linear_dx_merged(dYs, projs, out, terms)
    if merged is not None:
        return merged
    for gi, (dY, proj, t) in enumerate(zip(dYs, projs, terms)):
        out = _dx_gemm(_rows2d(dY), [proj], [t], t.P if t is not None else None, out, accumulate=gi > 0)
    return out


# ------------------------------------------------------------------------------------------------
# LoRA gradient products  G = s * P^T @ Z  (csrc/lora_side.hip)
def lora_tn_supported(Zs):
    return all(Z.is_cuda and Z.dtype in (torch.bfloat16, torch.float16) and Z.shape[-1] % 8 == 0 for Z in Zs)


# Gradient sinks: id(parameter) -> object with .grad_view(p) (contiguous fp32 tensor of p's shape that ACCUMULATES
# the gradient, e.g. a slice of dp.LoRAGradArena) and .ready(p) (called once the kernel that adds into it has been
# enqueued). With a sink the fused LoRA-gradient kernel adds straight into the arena: no per-parameter
# AccumulateGrad kernel, no temporary.
GRAD_SINKS = {}


def grad_sink(param):
    """The live sink that owns `param`'s gradient, or None. Entries hold WEAK references to their arena: an arena that
    is alive keeps its parameters alive, so a hit can never belong to a dead parameter whose id() was recycled."""
    if not GRAD_SINKS:
        return None
    ref = GRAD_SINKS.get(id(param))
    if ref is None:
        return None
    sink = ref()
    if sink is None:
        GRAD_SINKS.pop(id(param), None)
    return sink


def lora_tn(problems, targets=None):
    """problems: [(P fp32 [M, >=R] with unit column stride, Z [M, N], R, out_nr, scale)].
    Returns the fp32 products, [R, N] (out_nr False: lora_A.grad layout) or [N, R] (True: lora_B.grad layout).
    `targets[i]` (optional): contiguous fp32 tensor of that shape to ACCUMULATE into instead of allocating.
    One launch per 8 sixteen-rank problems; deterministic."""
    if not problems:
        return []
    M = problems[0][1].shape[0]
    dev = problems[0][1].device
    dtype = problems[0][1].dtype
    outs, descs, keep = [], [], []
    for pi, (P, Z, R, out_nr, scale) in enumerate(problems):
        Z2 = _rows2d(Z)
        if P.dim() != 2 or P.shape[0] != M or P.shape[1] < R or P.dtype != torch.float32:
            raise ValueError(f"lora_tn: problem {pi}: P must be fp32 [{M}, >= {R}], got {P.dtype} {tuple(P.shape)}")
        if Z2.shape[0] != M:
            raise ValueError(f"lora_tn: problem {pi}: Z has {Z2.shape[0]} rows, P {M}")
        if P.stride(1) != 1 or P.stride(0) % 4 or P.data_ptr() % 16:
            # the kernel fetches P in 16-byte pieces: a row stride of whole float4s from an aligned start, else a copy (its
            # width padded to whole float4s, which the fetch of the last ranks reads and drops)
            Pc = torch.zeros((M, (R + 3) // 4 * 4), dtype=torch.float32, device=P.device)
            Pc[:, :R] = P[:, :R]
            P = Pc
            keep.append(P)
        N = Z2.shape[1]
        tgt = targets[pi] if targets is not None else None
        if tgt is not None:
            assert (tgt.dtype == torch.float32 and tgt.is_contiguous() and tgt.device == dev
                    and tuple(tgt.shape) == ((N, R) if out_nr else (R, N)))
            out = tgt
        else:
            out = torch.empty((N, R) if out_nr else (R, N), dtype=torch.float32, device=dev)
        outs.append(out)
        keep.append(Z2)
        for r0 in range(0, R, 16):
            rc = min(16, R - r0)
            optr = out.data_ptr() + (4 * r0 if out_nr else 4 * r0 * N)
            descs.append(_lib.LoraTnProblem(P=P.data_ptr() + 4 * r0, Z=Z2.data_ptr(), out=optr, ldp=P.stride(0),
                                            ldz=Z2.stride(0), ldo=(R if out_nr else N), N=N, R=rc,
                                            out_nr=int(bool(out_nr)) | (2 if tgt is not None else 0),
                                            scale=float(scale)))
    S = (M + 127) // 128            # upper bound on the row chunks the kernel may choose
    for i in range(0, len(descs), 8):
        chunk = descs[i:i + 8]
        need = sum(S * 16 * ((d.N + 127) // 128) * 128 for d in chunk)
        ws = _nf4.scratch(dev, need, torch.float32, slot=40)
        arr = (_lib.LoraTnProblem * len(chunk))(*chunk)
        _lib.call("uamd_lora_tn", ws, arr, len(chunk), M, _lib.ptr(ws), need, _lib.dtype_code(dtype), _lib.stream_of(ws))
    return outs


# the gated activation fused with the LoRA skinny products (csrc/glu.hip glu_xa_kernel). Measured at Llama-3-8B MLP widths,
# 8192 tokens, in the step (profiles/r03ab_bench_kernel_stats.csv, after the tile loop lost its per-iteration vmcnt drain):
# backward 281 us against 217 + 2 x ~65 us for the separate launches, forward 157 us against 108 + 57 us; whole step +0.3-0.5 %
# with the forward fused too (profiles/r03ab_bench_ab.txt). At 2048 tokens 128 blocks left half the chip idle (118 vs 109 us,
# profiles/r03j_glu_fused_bench.jsonl) and rounds 3-4 fused from 4096 tokens on; with the columns of a row group split over
# adjacent workgroups (round 5, csrc/glu.hip launch_xa) the fused kernels win there too -- 38 vs 55 us forward, 79 vs 109 us
# backward at 2048 tokens, 139 vs 153 / 252 vs 325 us at 8192; batch-1 step -1.7 % (profiles/r05_glu_fused_bench.txt) -- so both
# directions are fused from 2048 tokens on.
# GLU_FUSED (module attribute; tools/glu_*.py set "all"): "both" | "bwd" (backward only, round 3's first default) | "all" (both, any
# size) | False.
GLU_FUSED = "both"
GLU_FUSED_MIN_ROWS = 2048
_GLU_ACTS = {"swiglu": 0, "geglu_exact": 1, "geglu_approx": 2}


# Rows of a whole number of 4 KiB pages (14336 or 28672 bf16 columns: the gated-MLP intermediates) read as the A operand of a
# GEMM -- 256 rows x 128 bytes per K tile -- put every line of a tile on the same few memory channels: the same GEMM with 128
# bytes of row padding measured +4.3 % (NT, K = 14336), +2.7 % (NN), tools/gemm_pad_probe.py / profiles/r06_gemm_row_padding.jsonl.
# alloc_rows gives such buffers a row stride of N + ROW_PAD elements (ROW_PAD = 0: plain).
ROW_PAD = 64


def alloc_rows(M, N, dtype, device, ld=None):
    """A [M, N] row-major buffer; `ld` = forced row stride (elements), default N (+ ROW_PAD for page-multiple rows >= 16 KiB)."""
    if ld is None:
        item = torch.empty((), dtype=dtype).element_size()
        ld = N + ROW_PAD if (ROW_PAD and N * item >= 16384 and (N * item) % 4096 == 0) else N
    buf = torch.empty((M, ld), dtype=dtype, device=device)
    return buf if ld == N else buf[:, :N]


def _same_rows(ts):
    """2-D row-major views with ONE row stride (a multiple of 8 elements) and 16-byte aligned starts: what the gated-activation
    kernels take through their single `ld`"""
    t0 = ts[0]
    return all(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) == t0.stride(0) and t.stride(0) % 8 == 0
               and t.data_ptr() % 16 == 0 and t.shape == t0.shape for t in ts)


def _glu_fusable(dtype, tensors, ranks, backward):
    K = tensors[0].shape[-1]
    mode = GLU_FUSED if GLU_FUSED is not True else "all"
    if not mode or (mode == "bwd" and not backward) or (mode in ("bwd", "both") and tensors[0].shape[0] < GLU_FUSED_MIN_ROWS):
        return False
    return (LORA_XA_V2 and dtype in (torch.bfloat16, torch.float16) and K % 8 == 0
            and all(t.is_cuda and t.dtype == dtype for t in tensors) and _same_rows(tensors)
            and all(r is not None and _streams(r) for r in ranks))


_GLU_WS = {}        # (device index, stream) -> (fp32 partials, int32 arrival counters): the column-split kernels' workspace


def _glu_workspace(t, n_products, max_rank):
    """Per device and stream (two launches in flight on different streams must not share it), grown on demand. The counters
    are zero when a launch starts and the kernel leaves them zero (the last workgroup of a row group resets its counter)."""
    M, K = t.shape
    need = int(_lib.lib().uamd_glu_xa_workspace(M, K, n_products, max_rank))
    groups = (M + 15) // 16
    key = (t.device.index, int(torch.cuda.current_stream(t.device).cuda_stream))
    ent = _GLU_WS.get(key)
    if ent is None or ent[0].numel() < need or ent[1].numel() < groups:
        part = torch.empty(max(need, ent[0].numel() if ent else 0), dtype=torch.float32, device=t.device)
        counters = torch.zeros(max(groups, ent[1].numel() if ent else 0), dtype=torch.int32, device=t.device)
        ent = _GLU_WS[key] = (part, counters)
    return ent


def glu_fwd_xa(act, e, g, down, n_out_cols_hint=None):
    """h = act(e) * g AND the down projection's X A^T (fp32 [M, r]) + rank block, in ONE pass over e and g
    (uamd_glu_fwd_xa). `down` = (W, W_quant, A, B, s[, bias]). Returns (h, [RankTerm]) as lora_linear_forward(pre_xa=) takes
    it -- the rank block by _forward_wants_rank_block, which that launch asks too -- or None when the shapes do not allow the
    fusion (the caller then runs the plain activation kernel and lets lora_linear_forward compute X A^T itself)."""
    A = down[2]
    # SwiGLU only (the hot path's activation): its fused arithmetic is bit-identical to the plain kernel, which is pinned
    # bit for bit to the reference's Triton kernel; the GeGLU instantiations differ from theirs in the last place in fp16
    if act != "swiglu" or A is None or not _glu_fusable(e.dtype, [e, g], [A.shape[0]], False):
        return None
    M, K = e.shape
    dtype = e.dtype
    r = A.shape[0]
    want_k = _forward_wants_rank_block(M, K, [down])
    Ac = cast_lora(A, dtype)
    h = alloc_rows(M, K, dtype, e.device, ld=e.stride(0))          # (one `ld` for e, g and h)
    xa = torch.empty((M, r), dtype=torch.float32, device=e.device)
    xk = torch.empty((M, _rank_width(r)), dtype=dtype, device=e.device) if want_k else None
    with _lib.device_ctx(e):
        part, counters = _glu_workspace(e, 1, r)
        rc = _lib.lib().uamd_glu_fwd_xa_ws(_GLU_ACTS[act], _lib.ptr(e), _lib.ptr(g), _lib.ptr(h), M, K, e.stride(0), _lib.ptr(Ac),
                                           Ac.stride(0), r, _lib.ptr(xa), xa.stride(0), r,
                                           _lib.ptr(xk) if xk is not None else None, xk.stride(0) if xk is not None else 0,
                                           xk.shape[1] if xk is not None else 0, _lib.ptr(part), part.numel(), _lib.ptr(counters),
                                           _lib.dtype_code(dtype), _lib.stream_of(e))
    if rc != 0:
        counters.zero_()                 # a launch that did not complete may leave arrival counts behind (include/unsloth_amd.h)
    _lib.check(rc, "uamd_glu_fwd_xa_ws")
    return h, [RankTerm(xa, xk, 0)]


def glu_bwd_terms(act, DW, e, g, up, gate):
    """The in-place activation backward (DW <- h, e <- df, g <- de) AND P_up = df @ B_up, P_gate = de @ B_gate -- the
    lora_dx_terms([df, de], [up, gate]) of fast_lora.mlp_backward -- in ONE pass (uamd_glu_bwd_xa). Returns
    (h, df, de, [p_up, p_gate] as RankTerms) or None when the shapes do not allow the fusion."""
    (Au, Bu), (Ag, Bg) = (up[2], up[3]), (gate[2], gate[3])
    if act != "swiglu" or Au is None or Ag is None or not _glu_fusable(e.dtype, [DW, e, g], [Au.shape[0], Ag.shape[0]], True):
        return None
    M, K = e.shape
    dtype = e.dtype
    ru, rg = Au.shape[0], Ag.shape[0]
    want_k = _dx_wants_rank_block(M, (up, gate))
    But, Bgt = cast_lora_t(Bu, dtype), cast_lora_t(Bg, dtype)                        # [r, K]
    shared = torch.empty((M, ru + rg), dtype=torch.float32, device=e.device)
    xk = torch.empty((M, _rank_width(ru + rg)), dtype=dtype, device=e.device) if want_k else None
    pu, pg = shared[:, :ru], shared[:, ru:]
    with _lib.device_ctx(e):
        part, counters = _glu_workspace(e, 2, max(ru, rg))
        rc = _lib.lib().uamd_glu_bwd_xa_ws(
            _GLU_ACTS[act], _lib.ptr(DW), _lib.ptr(e), _lib.ptr(g), M, K, e.stride(0),
            _lib.ptr(But), But.stride(0), ru, _lib.ptr(pu), shared.stride(0), ru,
            _lib.ptr(xk), xk.stride(0) if want_k else 0, ru if want_k else 0,
            _lib.ptr(Bgt), Bgt.stride(0), rg, _lib.ptr(pg), shared.stride(0), rg,
            _lib.ptr(xk[:, ru:]) if want_k else None, xk.stride(0) if want_k else 0, (xk.shape[1] - ru) if want_k else 0,
            _lib.ptr(part), part.numel(), _lib.ptr(counters), _lib.dtype_code(dtype), _lib.stream_of(e))
    if rc != 0:
        counters.zero_()
    _lib.check(rc, "uamd_glu_bwd_xa_ws")
    return DW, e, g, [RankTerm(pu, xk, 0), RankTerm(pg, xk, ru)]


# The SwiGLU backward that also forms the MLP's three wide LoRA gradients (csrc/glu.hip glu_tn_kernel): glu_bwd_terms writes h
# only for uamd_lora_tn to read it, df and de back; here the contraction over tokens happens while the tiles are on chip.
# GLU_TN = False switches fast_lora.mlp_backward back to glu_bwd_terms + the six-problem lora_tn launch.
GLU_TN = True
_GLU_TN_WS = {}     # (device index, stream) -> the fp32 partials of glu_tn_kernel (uamd_glu_tn_workspace bytes)


def glu_tn_takes(act, DW, e, g, up, gate, down):
    """Does glu_bwd_tn take this backward? SwiGLU on a shape the fused activation kernels take (GLU_FUSED, GLU_FUSED_MIN_ROWS),
    all three adapters present, every rank 8 or 16."""
    if not GLU_TN or act != "swiglu" or any(p[2] is None or p[3] is None for p in (up, gate, down)):
        return False
    ranks = [p[2].shape[0] for p in (up, gate, down)]
    return (all(r <= 16 and r % 8 == 0 for r in ranks) and _glu_fusable(e.dtype, [DW, e, g], ranks, True)
            and lora_tn_supported([DW, e, g]))


def _tn_factor(P, R):
    """P (fp32 [M, >= R]) as glu_tn_kernel fetches it: unit column stride, rows of whole float2s from an 8-byte aligned start"""
    if P.dtype == torch.float32 and P.stride(1) == 1 and P.stride(0) % 2 == 0 and P.data_ptr() % 8 == 0:
        return P
    return P[:, :R].float().contiguous()


def glu_bwd_tn(act, DW, e, g, up, gate, down, p_d, xa_u, xa_g, targets=None):
    """The in-place SwiGLU backward (e <- df, g <- de; DW is left as it is: h is never written) AND, in the same pass,
        p_up = df @ B_up, p_gate = de @ B_gate                 (fp32 [M, r] + the dX GEMM's rank block, as glu_bwd_terms)
        dA_down = s (p_d^T h), dB_up = s (df^T xa_u), dB_gate = s (de^T xa_g)      (fp32, as lora_tn returns them)
    with p_d = dY @ B_down, xa_u = X @ A_up^T, xa_g = X @ A_gate^T (fp32 [M, >= r]). `targets`: three contiguous fp32 tensors
    (or None each) to ACCUMULATE dA_down / dB_up / dB_gate into. Returns (df, de, [p_up, p_gate] as RankTerms, [dA_down, dB_up, dB_gate]),
    or None -- nothing launched, nothing touched -- when the shape is not taken (glu_tn_takes)."""
    if not glu_tn_takes(act, DW, e, g, up, gate, down):
        return None
    M, K = e.shape
    dtype, dev = e.dtype, e.device
    ru, rg, rd = up[2].shape[0], gate[2].shape[0], down[2].shape[0]
    if any(P.dim() != 2 or P.shape[0] != M or P.shape[1] < r for P, r in ((p_d, rd), (xa_u, ru), (xa_g, rg))):
        raise ValueError("glu_bwd_tn: p_d / xa_u / xa_g must be fp32 [M, >= rank]")
    want_k = _dx_wants_rank_block(M, (up, gate))
    But, Bgt = cast_lora_t(up[3], dtype), cast_lora_t(gate[3], dtype)                # [r, K]
    p_d, xa_u, xa_g = _tn_factor(p_d, rd), _tn_factor(xa_u, ru), _tn_factor(xa_g, rg)
    shapes = [(rd, K), (K, ru), (K, rg)]
    targets = list(targets) if targets is not None else [None] * 3
    grads, acc = [], 0
    for i, (tgt, shp) in enumerate(zip(targets, shapes)):
        if tgt is not None:
            assert tgt.dtype == torch.float32 and tgt.is_contiguous() and tgt.device == dev and tuple(tgt.shape) == shp
            acc |= 1 << i
        grads.append(tgt if tgt is not None else torch.empty(shp, dtype=torch.float32, device=dev))
    shared = torch.empty((M, ru + rg), dtype=torch.float32, device=dev)
    xk = torch.empty((M, _rank_width(ru + rg)), dtype=dtype, device=dev) if want_k else None
    with _lib.device_ctx(e):
        need = int(_lib.lib().uamd_glu_tn_workspace(M, K))
        key = (dev.index, int(torch.cuda.current_stream(dev).cuda_stream))
        ws = _GLU_TN_WS.get(key)
        if need >= 0 and (ws is None or ws.numel() < need):
            ws = _GLU_TN_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        rc = -2 if need < 0 else _lib.lib().uamd_glu_bwd_tn_ws(
            _lib.ptr(DW), _lib.ptr(e), _lib.ptr(g), M, K, e.stride(0),
            _lib.ptr(But), But.stride(0), ru, _lib.ptr(Bgt), Bgt.stride(0), rg,
            _lib.ptr(shared), shared.stride(0), _lib.ptr(xk), xk.stride(0) if want_k else 0, xk.shape[1] if want_k else 0,
            _lib.ptr(p_d), p_d.stride(0), rd, _lib.ptr(xa_u), xa_u.stride(0), _lib.ptr(xa_g), xa_g.stride(0),
            _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(grads[2]), float(down[4]), float(up[4]), float(gate[4]), acc,
            _lib.ptr(ws), ws.numel(), _lib.dtype_code(dtype), _lib.stream_of(e))
    if rc in _lib._ERR:         # one of the library's own codes: rejected before any launch -- "not supported", not "failed"
        return None
    _lib.check(rc, "uamd_glu_bwd_tn_ws")
    return e, g, [RankTerm(shared[:, :ru], xk, 0), RankTerm(shared[:, ru:], xk, ru)], grads


def dense_dw(dY, X, out=None, accumulate=False):
    """dW[out, in] (+)= dY[T, out]^T @ X[T, in]: the weight gradient of a trainable dense projection (full fine-tuning;
    torch.nn.Linear's `grad_output.t().mm(input)`). `dY` may be several projections' gradients side by side in one buffer
    ([T, sum out_g]: dQ | dK | dV as the attention backward writes them) -- then `out` is their stacked gradient
    [sum out_g, in]. One uamd_gemm_tn_256 launch (token chunks past GEMM_SPAN_LIMIT), both operands read in place; a token
    count that is not a multiple of 64 is zero-padded (zero rows add nothing)."""
    dY2d, X2d = _rows2d(dY), _rows2d(X)
    _lib.require_gpu(X2d)
    T, N_out = dY2d.shape
    assert X2d.shape[0] == T and X2d.dtype == dY2d.dtype
    dtype = X2d.dtype
    if dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError("the MFMA GEMM path takes bf16/fp16 activations")
    N_in = X2d.shape[1]
    if N_out % 8 or N_in % 8:
        raise NotImplementedError(f"dense_dw: out {N_out} / in {N_in} features must be multiples of 8")
    if T % 64:
        pad = 64 - T % 64
        dY2d = torch.nn.functional.pad(dY2d, (0, 0, 0, pad))
        X2d = torch.nn.functional.pad(X2d, (0, 0, 0, pad))
        T += pad
    if out is None:
        out = torch.empty((N_out, N_in), dtype=dtype, device=X2d.device)
        accumulate = False
    if out.dtype != dtype or tuple(out.shape) != (N_out, N_in) or out.stride(1) != 1:
        raise ValueError(f"dense_dw: out must be a {dtype} [{N_out}, {N_in}] matrix of unit column stride, got {out.dtype} "
                         f"{tuple(out.shape)} with strides {out.stride()}")
    # both operands have the contracted token dimension as rows: past GEMM_SPAN_LIMIT the tokens go in chunks (multiples of
    # 64), each launch after the first accumulating into `out` -- one more rounding of a 16-bit `out` per extra chunk
    item = X2d.element_size()
    for t0, rows in _row_spans(T, max(dY2d.stride(0), X2d.stride(0)) * item, 64):
        g = _group(X2d, out, N_in, X2d.stride(0))
        g.B += t0 * X2d.stride(0) * item
        _lib.call("uamd_gemm_tn_256", X2d, ctypes.c_void_p(dY2d.data_ptr() + t0 * dY2d.stride(0) * item), dY2d.stride(0),
                  N_out, rows, (GemmGroup * 1)(g), 1, int(bool(accumulate) or t0 > 0), _lib.dtype_code(dtype),
                  _lib.stream_of(X2d))
    return out


def matmul_lora(X, W, W_quant, A, B, s, out=None):
    """utils.py:1128-1170: out = X @ dequant(W).T (+ s * (X @ A.T) @ B.T).
    `W` may be the transposed packed storage (`W.t()`, shape [1, n/2]) or a transposed dense view,
    as LoRA_MLP.backward passes it (fast_lora.py:156); then the product is X @ W and A/B arrive
    already swapped and transposed ([in? r] layout), exactly like the reference."""
    reshape = X.dim() == 3
    if reshape:
        batch, seq_len, _ = X.shape
    transposed = (W_quant is not None and W.shape[0] == 1) or (
        W_quant is None and W.dim() == 2 and W.stride(0) == 1 and W.stride(1) != 1)
    if not transposed:
        res = lora_linear_forward(X, [(W, W_quant, A, B, s)], outs=None if out is None else [out])[0]
    else:
        Wn = W.t()
        # reference call: matmul_lora(dY, W.t(), q, B.t(), A.t(), s) -> our (A, B) are (B_lora^T, A_lora^T)
        proj = (Wn, W_quant, None if B is None else B.t(), None if A is None else A.t(), s)
        res = lora_linear_dx([X], [proj], out=out)
    return res.view(batch, seq_len, -1) if reshape else res


def fast_linear_forward(proj, X, temp_lora=None, out=None):
    """utils.py:1082-1125, the decode-time linear. X [bsz, q_len, in]: a single token of a single sequence goes through
    the GEMV kernels (csrc/decode.hip: NF4 decoded in the kernel, LoRA and bias folded into its reduction -- the
    reference's cdequantize_blockwise_fp32 + cgemm_4bit_inference_naive + mv + addmv); everything else through
    matmul_lora like the reference's q_len != 1 / bsz > 1 branches. `temp_lora` is accepted and unused (the A x
    products of a launch land in one fp32 vector of their own)."""
    from . import decode as _dk
    W, W_quant, A, B, s, bias = get_lora_parameters_bias(proj)
    _refuse_fp8([(W,)])
    bsz, q_len, in_dim = X.shape
    n_out = int(_features(W, W_quant)[0])
    if bsz == 1 and q_len == 1 and in_dim <= 16384 and X.dtype in (torch.bfloat16, torch.float16) \
            and (W_quant is not None or W.dtype == X.dtype):
        flat = out.view(-1) if out is not None else None
        (y,) = _dk.linear_group(X.reshape(-1), [(W, W_quant, A, B, s, bias)], out=flat)
        return y.view(1, 1, n_out)
    y = matmul_lora(X, W, W_quant, A, B, s, out=out)
    if bias is not None:
        y += bias
    return y


def fast_gemv(X, W, quant_state, out=None):
    """utils.py:872-977: out[1, 1, N] = X[1, 1, K] @ W^T for an NF4 weight (or a plain matmul when quant_state is None,
    :880-881). One uamd_gemv launch; the nested absmax is decoded inside it."""
    from . import decode as _dk
    _refuse_fp8([(W,)])
    if quant_state is None:
        return torch.matmul(X, W, out=out)
    N = int(quant_state.shape[0])
    flat = out.view(-1) if out is not None else None
    (y,) = _dk.linear_group(X.reshape(-1), [(W, quant_state, None, None, None)], out=flat)
    return y.view(1, 1, N)
