"""Helpers of the LoRA block route tests (tests/test_lora_block_inputs.py on the host, tests/test_gpu_lora_block_routes.py on the
GPU): a table of small cases that between them reach every dispatch route of LoRA_MLP / LoRA_QKV / LoRA_W
(unsloth_amd/kernels/fast_lora.py, unsloth_amd/kernels/utils.py), an fp64 autograd truth, a model of what a correct 16-bit
implementation rounds away, and an error per token row / rank row / rank column. Nothing here runs a kernel: the case builder,
the truth and the model are CPU code (the NF4 weights are quantised with the oracle's numpy quantiser).

A case is judged slice by slice: err(kernel, truth64) <= factor x err(rounding model, truth64), both errors taken on the same
slice, so the bound is a multiple of the reference side's own error and a wrong row or a dropped rank shows at full size."""
import functools
import zlib

import numpy as np
import torch

from oracle import ref_ops as R

H, I, HKV = 256, 704, 128                       # the widths of tests/test_gpu_lora_blocks.py; H and I are multiples of 64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
PROJS = {"mlp": ("gate", "up", "down"), "qkv": ("q", "k", "v"), "w": ("o",)}
SHAPES = {"gate": (I, H), "up": (I, H), "down": (H, I), "q": (H, H), "k": (HKV, H), "v": (HKV, H), "o": (H, H)}   # [out, in]
OUTPUTS = {"mlp": ("out",), "qkv": ("Q", "K", "V"), "w": ("out",)}
SCALE = 2.0

# short names of the library entry points the route assertions speak of
GEMM = {"uamd_gemm_nt": "nt", "uamd_gemm_nt_nf4": "nt_nf4", "uamd_gemm_nt_256": "nt_256", "uamd_gemm_nn_256": "nn_256",
        "uamd_gemm_tn_256": "tn_256"}
XA = {"uamd_lora_xa": "xa", "uamd_lora_xa2": "xa2", "uamd_lora_xa2k": "xa2k"}
DECODE = ("uamd_nf4_dequantize", "uamd_nf4_dequantize_multi")
OTHER = ("uamd_lora_tn", "uamd_glu_fwd_xa_ws", "uamd_glu_bwd_xa_ws", "uamd_glu_bwd_tn_ws")
ENTRIES = tuple(GEMM) + tuple(XA) + DECODE + OTHER
PY_ROUTES = ("glu_fwd_xa", "glu_bwd_tn", "glu_bwd_terms", "lora_tn", "_lora_grads")       # names in kernels/fast_lora.py

OFF, ON = {"GEMM256_MODE": "off"}, {"GEMM256_MODE": "on"}
PLAIN, FUSED = {"GLU_FUSED": False}, {"GLU_FUSED": "all"}
CASES = {}


def _case(name, block, M, ranks, knobs, fwd, bwd, n_bwd, xa, py, *, quant=True, dtype="bf16", kind="swiglu", scales=None,
          bias=None, merged=False, inplace=True, params=True, zero_row=False, decode=False):
    """One row of the table. `ranks`: per projection of PROJS[block], None = no adapter. `knobs`: module attributes of
    unsloth_amd.kernels.utils for the case. What the case means to reach, all asserted exactly by the GPU test:
      fwd / bwd   the GEMM entry points of the forward / the backward (short names of GEMM)
      n_bwd       GEMM launches of the backward (MLP: 1 for DW + 1 merged or 2 per-projection dX; q|k|v: 1 merged or 3)
      xa          the X @ A^T / dY @ B entry points of both directions (short names of XA)
      py          which of PY_ROUTES ran and took the shape
      decode      the forward decodes NF4 into scratch (else: inside the GEMM, or dense weights)
    `merged`: dQ | dK | dV arrive as column blocks of one buffer. `bias`: None | "frozen" | "train" on q/k/v (through the
    autograd Function). `params`: the factors are fp32 nn.Parameters (the prepared-copies path) or plain tensors."""
    assert name not in CASES and len(ranks) == len(PROJS[block])
    knobs = dict(knobs)
    CASES[name] = dict(name=name, block=block, M=M, ranks=tuple(ranks), knobs=knobs, fwd=set(fwd), bwd=set(bwd), n_bwd=n_bwd,
                       xa=set(xa), py=set(py), quant=quant, dtype=dtype, kind=kind,
                       scales=tuple(scales) if scales else (SCALE,) * len(ranks), bias=bias, merged=merged, inplace=inplace,
                       params=params, zero_row=zero_row, decode=decode)


def _k(*ds, **kw):
    out = {}
    for d in ds:
        out.update(d)
    out.update(kw)
    return out


N3 = (None, None, None)
TN = ("glu_fwd_xa", "glu_bwd_tn", "lora_tn")
TERMS = ("glu_fwd_xa", "glu_bwd_terms", "lora_tn")

# ---- LoRA_MLP: (gate, up, down) -------------------------------------------------------------------------------------------
# the three SwiGLU backward routes at the existing shape (M = 150 = 2 x 75), NF4 decoded inside the 128-tile GEMM
_case("mlp-r16-plain", "mlp", 150, (16, 16, 16), _k(OFF, PLAIN), ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], zero_row=True)
_case("mlp-r16-terms", "mlp", 150, (16, 16, 16), _k(OFF, FUSED, GLU_TN=False), ["nt_nf4"], ["nt"], 2, ["xa2"], TERMS)
_case("mlp-r16-tn", "mlp", 150, (16, 16, 16), _k(OFF, FUSED, GLU_TN=True), ["nt_nf4"], ["nt"], 2, ["xa2"], TN, inplace=False)
_case("mlp-r16-tn-dense", "mlp", 150, (16, 16, 16), _k(OFF, FUSED), ["nt"], ["nt"], 3, ["xa2"], TN, quant=False)
# the 256-tile family: rank block on the NT forward, NN dX
_case("mlp-r16-256-tn-dense", "mlp", 150, (16, 16, 16), _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, ["xa2k"], TN, quant=False,
      zero_row=True)
_case("mlp-r16-256-nf4", "mlp", 150, (16, 16, 16), _k(ON, FUSED), ["nt_nf4"], ["nn_256"], 2, ["xa2", "xa2k"], TN)
_case("mlp-r16-256-decode", "mlp", 150, (16, 16, 16), _k(ON, FUSED, FUSED_NF4=False), ["nt_256"], ["nn_256"], 2, ["xa2k"], TN,
      decode=True)
# either side of FUSED_NF4_MAX_M, lowered to 128
_case("mlp-r16-m127-maxm", "mlp", 127, (16, 16, 16), _k(OFF, PLAIN, FUSED_NF4_MAX_M=128), ["nt_nf4"], ["nt"], 3, ["xa2"],
      ["lora_tn"])
_case("mlp-r16-m129-maxm", "mlp", 129, (16, 16, 16), _k(OFF, PLAIN, FUSED_NF4_MAX_M=128), ["nt"], ["nt"], 3, ["xa2"],
      ["lora_tn"], decode=True)
# both GeGLU kinds: the plain activation kernels whatever GLU_FUSED says
_case("mlp-r16-geglu-exact", "mlp", 150, (16, 16, 16), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"],
      kind="geglu_exact")
_case("mlp-r16-geglu-approx-256-dense", "mlp", 150, (16, 16, 16), _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, ["xa2k"],
      ["lora_tn"], kind="geglu_approx", quant=False)
# ranks
_case("mlp-r4", "mlp", 150, (4, 4, 4), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"])
_case("mlp-r4-256-dense", "mlp", 150, (4, 4, 4), _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, ["xa2", "xa2k"], ["lora_tn"],
      quant=False)
_case("mlp-r8-tn", "mlp", 150, (8, 8, 8), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 2, ["xa2"], TN)
_case("mlp-r12", "mlp", 150, (12, 12, 12), _k(OFF, PLAIN), ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], params=False)
_case("mlp-r12-m300-256-dense", "mlp", 300, (12, 12, 12), _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, ["xa2", "xa2k"],
      ["lora_tn"], quant=False)
_case("mlp-r32-terms", "mlp", 150, (32, 32, 32), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 2, ["xa2"], TERMS)
_case("mlp-r64-terms", "mlp", 150, (64, 64, 64), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 2, ["xa", "xa2"], TERMS)
# r = 64 on gate|up with a rank block: total rank 128, one X @ A^T launch per 64 ranks
_case("mlp-r64-256-dense", "mlp", 150, (64, 64, 64), _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, ["xa2k"], TERMS, quant=False)
# r = 128: gate|up stack 256 rank columns (two X @ A^T launches: 192 + 64); nothing fused takes the width
_case("mlp-r128", "mlp", 150, (128, 128, 128), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, ["xa", "xa2"], ["lora_tn"])
_case("mlp-r128-256-dense", "mlp", 150, (128, 128, 128), _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, ["xa", "xa2"], ["lora_tn"],
      quant=False)
_case("mlp-r8-16-64", "mlp", 150, (8, 16, 64), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 2, ["xa2"], TERMS)
_case("mlp-r8-16-64-m257-256-dense", "mlp", 257, (8, 16, 64), _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, ["xa2k"], TERMS,
      quant=False, inplace=False)
# adapter sets: with a projection missing the fused routes and the merged dX decline
# (without down's adapter the forward's activation is the plain kernel on flat copies of e and g: df | de are not one buffer)
_case("mlp-gate-up-only", "mlp", 150, (16, 16, None), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, ["xa2"],
      ["glu_bwd_terms", "lora_tn"])
_case("mlp-down-only", "mlp", 150, (None, None, 16), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, ["xa2"], ["glu_fwd_xa", "lora_tn"])
_case("mlp-up-only", "mlp", 150, (None, 16, None), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"])
_case("mlp-none", "mlp", 150, N3, _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, [], [])
_case("mlp-none-256-dense", "mlp", 150, N3, _k(ON, FUSED), ["nt_256"], ["nn_256"], 3, [], [], quant=False)
# rows (one row: a [1, N] view carries no row stride to compare, so _adjacent_columns and with it the merged dX decline)
_case("mlp-r16-m1-tn", "mlp", 1, (16, 16, 16), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 3, ["xa2"], TN)
_case("mlp-r16-m257-tn", "mlp", 257, (16, 16, 16), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 2, ["xa2"], TN)
_case("mlp-r16-m300-256-terms-dense", "mlp", 300, (16, 16, 16), _k(ON, FUSED, GLU_TN=False), ["nt_256"], ["nn_256"], 3,
      ["xa2k"], TERMS, quant=False)
# the first-version X @ A^T kernel; with it no rank block is written beside P = dY B, so the dX GEMM keeps the prologue
_case("mlp-r16-xa1", "mlp", 150, (16, 16, 16), _k(OFF, FUSED, LORA_XA_V2=False), ["nt_nf4"], ["nt"], 3, ["xa"], ["lora_tn"])
_case("mlp-r16-xa1-256-dense", "mlp", 150, (16, 16, 16), _k(ON, FUSED, LORA_XA_V2=False), ["nt_256"], ["nt"], 3, ["xa"],
      ["lora_tn"], quant=False)
# fp16
_case("mlp-r16-fp16-tn", "mlp", 150, (16, 16, 16), _k(OFF, FUSED), ["nt_nf4"], ["nt"], 2, ["xa2"], TN, dtype="fp16")
_case("mlp-r4-m129-fp16-256-dense", "mlp", 129, (4, 4, 4), _k(ON, PLAIN), ["nt_256"], ["nn_256"], 3, ["xa2", "xa2k"],
      ["lora_tn"], quant=False, dtype="fp16")

# ---- LoRA_QKV: (q, k, v) --------------------------------------------------------------------------------------------------
_case("qkv-r16", "qkv", 150, (16, 16, 16), OFF, ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], zero_row=True)
# dQ | dK | dV as column blocks of one buffer: ONE K-concatenated dX GEMM
_case("qkv-r16-merged", "qkv", 150, (16, 16, 16), OFF, ["nt_nf4"], ["nt"], 1, ["xa2"], ["lora_tn"], merged=True)
# ... refused by the prologue, which has one scale per launch; taken by the rank block, whose BK carries the scales
_case("qkv-r16-merged-scales", "qkv", 150, (16, 16, 16), OFF, ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], merged=True,
      scales=(2.0, 1.0, 0.5))
_case("qkv-r16-merged-scales-256", "qkv", 150, (16, 16, 16), ON, ["nt_nf4"], ["nn_256"], 1, ["xa2", "xa2k"], ["lora_tn"],
      merged=True, scales=(2.0, 1.0, 0.5), inplace=False)
_case("qkv-r16-merged-dense", "qkv", 150, (16, 16, 16), OFF, ["nt"], ["nt"], 3, ["xa2"], ["lora_tn"], merged=True, quant=False)
_case("qkv-r16-m129-maxm", "qkv", 129, (16, 16, 16), _k(OFF, FUSED_NF4_MAX_M=128), ["nt"], ["nt"], 3, ["xa2"], ["lora_tn"],
      decode=True)
_case("qkv-r16-m127-maxm", "qkv", 127, (16, 16, 16), _k(OFF, FUSED_NF4_MAX_M=128), ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"])
# r = 64 on q|k|v: total rank 192, the grouped launch (one per 64 ranks) behind a rank block; one 192-rank launch without
_case("qkv-r64", "qkv", 150, (64, 64, 64), OFF, ["nt_nf4"], ["nt"], 3, ["xa", "xa2"], ["lora_tn"])
_case("qkv-r64-256-dense", "qkv", 150, (64, 64, 64), ON, ["nt_256"], ["nn_256"], 3, ["xa2k"], ["lora_tn"], quant=False)
_case("qkv-r64-256-merged", "qkv", 150, (64, 64, 64), _k(ON, FUSED_NF4=False), ["nt_256"], ["nn_256"], 1, ["xa2k"], ["lora_tn"],
      merged=True, decode=True)
_case("qkv-r32-m129-256-dense", "qkv", 129, (32, 32, 32), ON, ["nt_256"], ["nn_256"], 3, ["xa2k"], ["lora_tn"], quant=False)
# r = 128: 384 rank columns, two 192-rank launches; the merged dX keeps the prologue (no shared rank block past 64 per member)
_case("qkv-r128-merged", "qkv", 150, (128, 128, 128), OFF, ["nt_nf4"], ["nt"], 1, ["xa"], ["lora_tn"], merged=True)
_case("qkv-r128-256-dense", "qkv", 150, (128, 128, 128), ON, ["nt_256"], ["nn_256"], 3, ["xa"], ["lora_tn"], quant=False)
_case("qkv-r128-m129-256-merged", "qkv", 129, (128, 128, 128), _k(ON, FUSED_NF4=False), ["nt_256"], ["nt"], 1, ["xa"],
      ["lora_tn"], merged=True, decode=True)
# rank_pattern and ranks that are no multiple of 8: no shared P buffer, so no merged dX
_case("qkv-r16-8-4-merged", "qkv", 150, (16, 8, 4), OFF, ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], merged=True)
_case("qkv-r16-8-4-m257-256-dense", "qkv", 257, (16, 8, 4), ON, ["nt_256"], ["nn_256"], 3, ["xa2", "xa2k"], ["lora_tn"],
      quant=False)
_case("qkv-r4", "qkv", 150, (4, 4, 4), OFF, ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], params=False)
_case("qkv-r12-m300-256-dense", "qkv", 300, (12, 12, 12), ON, ["nt_256"], ["nn_256"], 3, ["xa2", "xa2k"], ["lora_tn"],
      quant=False)
_case("qkv-r8-m1", "qkv", 1, (8, 8, 8), OFF, ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], merged=True)     # (as mlp-r16-m1-tn)
# adapter sets
_case("qkv-q-v-only-merged", "qkv", 150, (16, None, 16), OFF, ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], merged=True)
_case("qkv-q-only-256-dense", "qkv", 150, (16, None, None), ON, ["nt_256"], ["nn_256"], 3, ["xa2k"], ["lora_tn"], quant=False)
_case("qkv-none-merged", "qkv", 150, N3, OFF, ["nt_nf4"], ["nt"], 3, [], [], merged=True)
# biases in the GEMM epilogue (through the autograd Function: d_bias only where the bias trains)
_case("qkv-r16-bias-frozen", "qkv", 150, (16, 16, 16), OFF, ["nt_nf4"], ["nt"], 3, ["xa2"], ["lora_tn"], bias="frozen")
_case("qkv-r16-bias-train-256-dense", "qkv", 129, (16, 16, 16), ON, ["nt_256"], ["nn_256"], 3, ["xa2k"], ["lora_tn"],
      bias="train", quant=False)
# fp16
_case("qkv-r16-fp16-merged", "qkv", 150, (16, 16, 16), OFF, ["nt_nf4"], ["nt"], 1, ["xa2"], ["lora_tn"], merged=True,
      dtype="fp16")
_case("qkv-r64-m129-fp16-256-dense", "qkv", 129, (64, 64, 64), ON, ["nt_256"], ["nn_256"], 3, ["xa2k"], ["lora_tn"],
      quant=False, dtype="fp16")

# ---- LoRA_W: (o,) ---------------------------------------------------------------------------------------------------------
_case("w-r16", "w", 150, (16,), OFF, ["nt_nf4"], ["nt"], 1, ["xa2"], ["lora_tn"], zero_row=True)
_case("w-r4-m129-256-dense", "w", 129, (4,), ON, ["nt_256"], ["nn_256"], 1, ["xa2k"], ["lora_tn"], quant=False)
_case("w-r64-m1", "w", 1, (64,), OFF, ["nt_nf4"], ["nt"], 1, ["xa2"], ["lora_tn"])
_case("w-r128-m300", "w", 300, (128,), OFF, ["nt_nf4"], ["nt"], 1, ["xa"], ["lora_tn"])
_case("w-r128-256-dense", "w", 150, (128,), ON, ["nt_256"], ["nn_256"], 1, ["xa"], ["lora_tn"], quant=False)
_case("w-none", "w", 150, (None,), OFF, ["nt_nf4"], ["nt"], 1, [], [])
_case("w-r16-fp16-256-decode", "w", 150, (16,), _k(ON, FUSED_NF4=False), ["nt_256"], ["nn_256"], 1, ["xa2k"], ["lora_tn"],
      dtype="fp16", decode=True)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def quantize_nf4_cpu(W):
    """bitsandbytes NF4 of W [out, in] with blocksize 64 and nested statistics, on the CPU: the oracle's numpy quantiser for the
    first level, the product's own (plain torch) quantiser of the statistics. Returns the pieces of the quant state as CPU
    tensors; `quant_state` assembles them on a device."""
    from unsloth_amd import nf4
    packed, absmax = R.nf4_quantize_np(W.float().numpy().reshape(-1), 64)
    absmax = torch.from_numpy(absmax)
    offset = absmax.mean()
    code2 = nf4.create_dynamic_map()
    q, absmax2 = nf4._quantize_blockwise_8bit(absmax - offset, code2, 256)
    return dict(packed=torch.from_numpy(packed).view(-1, 1), absmax=q, absmax2=absmax2, code2=code2, offset=offset,
                code=torch.tensor(np.asarray(R.NF4_CODE), dtype=torch.float32), shape=tuple(W.shape), dtype=W.dtype)


def quant_state(pieces, device="cpu"):
    """(packed, QuantState) of `quantize_nf4_cpu`'s pieces on `device`: a fresh state per call (the product caches on it)."""
    from unsloth_amd import nf4
    to = lambda t: t.clone().to(device)
    state2 = nf4.QuantState(absmax=to(pieces["absmax2"]), code=to(pieces["code2"]), blocksize=256, dtype=torch.float32,
                            quant_type=None)
    qs = nf4.QuantState(absmax=to(pieces["absmax"]), shape=pieces["shape"], dtype=pieces["dtype"], blocksize=64,
                        code=to(pieces["code"]), quant_type="nf4", offset=to(pieces["offset"]), state2=state2)
    return to(pieces["packed"]), qs


@functools.lru_cache(maxsize=None)
def _weight(proj, quant, dtype_name):
    """(the weight every reference multiplies by, the NF4 pieces or None): randn * 0.03 in the activation dtype, and for
    NF4 what the format decodes to (R.nf4_dequantize_state, as tests/test_gpu_lora_blocks.py `_mk`)."""
    dtype = DTYPES[dtype_name]
    W = (torch.randn(SHAPES[proj], generator=_gen("W", proj)) * 0.03).to(dtype)
    if not quant:
        return W, None
    pieces = quantize_nf4_cpu(W)
    return R.nf4_dequantize_state(*quant_state(pieces)), pieces


@functools.lru_cache(maxsize=None)
def _factors(proj, r):
    out_f, in_f = SHAPES[proj]
    return (torch.randn(r, in_f, generator=_gen("A", proj, r)) * 0.05, torch.randn(out_f, r, generator=_gen("B", proj, r)) * 0.05)


def case_inputs(name):
    """The inputs of a case, seeded, on the CPU: X and one dY per output in the activation dtype, and per projection
    (W as every reference uses it, NF4 pieces or None, A fp32 or None, B fp32 or None, s, bias or None)."""
    c = CASES[name]
    dtype = DTYPES[c["dtype"]]
    projs = {}
    for p, r, s in zip(PROJS[c["block"]], c["ranks"], c["scales"]):
        W, pieces = _weight(p, c["quant"], c["dtype"])
        A, B = _factors(p, r) if r is not None else (None, None)
        bias = (torch.randn(SHAPES[p][0], generator=_gen("bias", p)) * 0.1).to(dtype) if c["bias"] else None
        projs[p] = (W, pieces, A, B, s, bias)
    first, last = PROJS[c["block"]][0], PROJS[c["block"]][-1]
    X = (torch.randn(c["M"], SHAPES[first][1], generator=_gen("X", name)) * 0.5).to(dtype)
    widths = [SHAPES[p][0] for p in PROJS[c["block"]]] if c["block"] == "qkv" else [SHAPES[last][0]]
    dYs = {}
    for o, n in zip(OUTPUTS[c["block"]], widths):
        dY = torch.randn(c["M"], n, generator=_gen("dY", name, o)).to(dtype)
        if c["zero_row"]:
            dY[c["M"] // 2] = 0                     # a token whose gradient is exactly zero: its dX row must be, too
        dYs[o] = dY
    return X, dYs, projs


# ---- the fp64 truth and the rounding model ------------------------------------------------------------------------------------
def _act64(e, kind):
    if kind == "swiglu":
        return e * torch.sigmoid(e)
    return torch.nn.functional.gelu(e, approximate="tanh" if kind == "geglu_approx" else "none")


def _rounded(P, dtype):
    return None if P is None else P.to(dtype)


def truth64(name):
    """fp64 autograd of the block on the case's inputs: X, dY and the decoded weights as given, A and B rounded to the
    activation dtype first (cast_lora does that on the GPU), no intermediate rounded. {tensor name: fp64 tensor or None}: the
    outputs, dX, dA_<proj> / dB_<proj> (None without an adapter) and dbias_<proj> where a bias trains."""
    c = CASES[name]
    dtype = DTYPES[c["dtype"]]
    X, dYs, projs = case_inputs(name)
    x = X.double().requires_grad_(True)
    leaves, names, P = [x], ["dX"], {}
    for p, (W, _, A, B, s, bias) in projs.items():
        A64 = B64 = b64 = None
        if A is not None:
            A64, B64 = (_rounded(t, dtype).double().requires_grad_(True) for t in (A, B))
            leaves += [A64, B64]
            names += [f"dA_{p}", f"dB_{p}"]
        if bias is not None:
            b64 = bias.double().requires_grad_(c["bias"] == "train")
            if c["bias"] == "train":
                leaves.append(b64)
                names.append(f"dbias_{p}")
        P[p] = (W.double(), A64, B64, s, b64)

    def lin(t, p):
        W, A, B, s, b = P[p]
        y = t @ W.t()
        if A is not None:
            y = y + s * (t @ A.t()) @ B.t()
        return y if b is None else y + b

    if c["block"] == "mlp":
        outs = [lin(_act64(lin(x, "gate"), c["kind"]) * lin(x, "up"), "down")]
    else:
        outs = [lin(x, p) for p in PROJS[c["block"]]]
    grads = torch.autograd.grad(outs, leaves, [dYs[o].double() for o in OUTPUTS[c["block"]]])
    res = {o: y.detach() for o, y in zip(OUTPUTS[c["block"]], outs)}
    res.update(zip(names, grads))
    for p in projs:
        res.setdefault(f"dA_{p}", None)
        res.setdefault(f"dB_{p}", None)
    return res


def rounding_model(name, mutant=None):
    """The same block in fp32 on the CPU with the rounding points the product has -- the yardstick of the GPU tests, not a model
    of any kernel's schedule. Forward: R.lora_mlp_forward / R.matmul_lora as they are (a bias is added to the fp32 value of
    that and rounded). Backward: the formulas of kernels/fast_lora.py's header in fp32,
        dA = s (dY B)^T X      dB = s dY^T (X A^T)      dX = dY W + s (dY B) A,
    on the intermediates the kernels keep in 16 bits, rounded there: e, g, h, DW, df, de, dX, and the two rank-r factors
    P = dY B and X A^T wherever they are an operand (the rank block XK holds them in the activation dtype, the 128-tile prologue
    and uamd_lora_tn convert them on load: csrc/gemm256.hip, csrc/gemm.hip, csrc/lora_side.hip "rounded to the activation dtype
    where the reference holds a bf16 tensor"; R.matmul_lora rounds X A^T in the forward for the same reason). dA and dB stay
    fp32, as lora_tn returns them; a bias gradient is the fp32 column sum rounded to the bias dtype.

    `mutant`: None, or one of the deliberately wrong variants test_lora_block_inputs feeds to `judge` (see `mutants`)."""
    c = CASES[name]
    dt = DTYPES[c["dtype"]]
    X, dYs, projs = case_inputs(name)
    r = lambda t: R.rt(t, dt)
    kind, arg = mutant if mutant else (None, None)
    gen = _gen("mutant", name)
    P = {}
    for p, (W, _, A, B, s, bias) in projs.items():
        if kind == "drop_all":
            A = B = None
        elif A is not None and arg == p:
            if kind == "drop_term":
                A = B = None
            elif kind == "drop_last_rank":
                A, B = A[:-1], B[:, :-1]
            elif kind == "scale_once_less":
                s = 1.0
            elif kind == "scale_once_more":
                s = s * s
            elif kind == "pad_nonzero":
                pad = -A.shape[0] % 8
                A = torch.cat([A, torch.randn(pad, A.shape[1], generator=gen) * 0.05])
                B = torch.cat([B, torch.randn(B.shape[0], pad, generator=gen) * 0.05], dim=1)
        P[p] = (W, A, B, s, bias)

    def fwd(t, p):
        W, A, B, s, bias = P[p]
        y = R.matmul_lora(t, W, A, B, s)
        return y if bias is None else (y.float() + bias.float()).to(dt)

    def dx_of(dy, p, rows=None):
        """(dy W + s r(dy B) A, r(dy B)) in fp32; `rows` = the weight and factors of another projection (the swap mutant)"""
        W, A, B, s, _ = P[rows or p]
        d = dy @ W.float()
        if A is None:
            return d, None
        pb = r(dy @ r(B.float()))
        return d + s * pb @ r(A.float()), pb

    def grads_of(xin, dy, pb, p):
        W, A, B, s, _ = P[p]
        if A is None:
            return None, None
        return s * pb.t() @ xin, s * dy.t() @ r(xin @ r(A.float()).t())

    x = X.float()
    res = {}
    if c["block"] == "mlp":
        out, e, g, _ = R.lora_mlp_forward(X, *(P[p][:4] for p in ("gate", "up", "down")), c["kind"])
        dy = dYs["out"].float()
        DW, p_d = dx_of(dy, "down")
        h, df, de = (t.float() for t in R.glu_backward(DW.to(dt), e, g, c["kind"]))
        swap = kind == "swap_up_gate"
        dxu, p_u = dx_of(df, "up", "gate" if swap else None)
        dxg, p_g = dx_of(de, "gate", "up" if swap else None)
        if swap:                                      # (the rank products of the swapped dX belong to no gradient)
            _, p_u = dx_of(df, "up")
            _, p_g = dx_of(de, "gate")
        res["out"], res["dX"] = out, r(dxu + dxg)
        res["dA_down"], res["dB_down"] = grads_of(h, dy, p_d, "down")
        res["dA_up"], res["dB_up"] = grads_of(x, df, p_u, "up")
        res["dA_gate"], res["dB_gate"] = grads_of(x, de, p_g, "gate")
    else:
        dX = 0
        for p, o in zip(PROJS[c["block"]], OUTPUTS[c["block"]]):
            dy = dYs[o].float()
            res[o] = fwd(X, p)
            d, pb = dx_of(dy, p)
            dX = dX + d
            res[f"dA_{p}"], res[f"dB_{p}"] = grads_of(x, dy, pb, p)
            if c["bias"] == "train":
                res[f"dbias_{p}"] = dy.sum(0).to(dt)
        res["dX"] = r(dX)
    for p, (_, _, A0, B0, _, _) in projs.items():     # a mutant with another rank: back to the shapes of the case
        if A0 is not None and res[f"dA_{p}"] is not None and res[f"dA_{p}"].shape != A0.shape:
            dA, dB = torch.zeros(A0.shape), torch.zeros(B0.shape)
            n = min(A0.shape[0], res[f"dA_{p}"].shape[0])
            dA[:n], dB[:, :n] = res[f"dA_{p}"][:n], res[f"dB_{p}"][:, :n]
            res[f"dA_{p}"], res[f"dB_{p}"] = dA, dB
    if kind == "last_row_no_lora":                    # the LoRA term missing from the last token row only
        bare = rounding_model(name, ("drop_all", None))
        for t in OUTPUTS[c["block"]] + ("dX",):
            res[t] = res[t].clone()
            res[t][-1] = bare[t][-1]
    return res


def mutants(name):
    """[(kind, projection or None)]: the wrong variants of the rounding model that `judge` must reject on this case -- one
    projection's LoRA term dropped, its last rank dropped, its scale applied once too few / once too often (s^0, s^2), up and
    gate swapped in dX, the LoRA term missing from the last token row only, the rank padding columns non-zero."""
    c = CASES[name]
    with_lora = [p for p, r in zip(PROJS[c["block"]], c["ranks"]) if r is not None]
    out = []
    for p in {with_lora[0], with_lora[-1]} if with_lora else ():
        out += [("drop_term", p), ("drop_last_rank", p), ("scale_once_less", p), ("scale_once_more", p)]
        if dict(zip(PROJS[c["block"]], c["ranks"]))[p] % 8:
            out.append(("pad_nonzero", p))
    if with_lora:
        out.append(("last_row_no_lora", None))
    if c["block"] == "mlp":
        out.append(("swap_up_gate", None))
    return sorted(out, key=repr)


# ---- the error and the verdict ----------------------------------------------------------------------------------------------
def slices_of(tensor_name, M=None):
    """How a tensor is cut for `row_err`: a token row of an activation, a rank row of dA [r, in], a rank column of dB [out, r],
    a bias gradient as one vector. With M = 1 token a rank row of dA = s P^T X is ONE rounded number of P times X (a rank
    column of dB one of X A^T times dY): the error of a single rounding lies anywhere between nothing and half an ulp, and two
    correct implementations differ there by any factor. The smallest slice that holds enough roundings to compare is then the
    whole tensor (a dropped rank is still 1 / r of it)."""
    if tensor_name.startswith("dbias_") or (M == 1 and tensor_name[:3] in ("dA_", "dB_")):
        return "all"
    return "col" if tensor_name.startswith("dB_") else "row"


def row_err(got, ref, by="row"):
    """The L2 norm of got - ref per slice, fp64 [slices]: by="row" over the last axis (a token row of [M, N], a rank row of
    dA [r, in]), by="col" over the first (a rank column of dB [out, r]), by="all" over everything."""
    d = got.detach().double().cpu().reshape(ref.shape) - ref.detach().double().cpu()
    if by == "all":
        return d.flatten().norm()[None]
    d = d.reshape(-1, d.shape[-1])
    return d.norm(dim=0 if by == "col" else 1)


BOUND_FACTOR = 4        # the project's figure (tests/_attn_edges.py): a kernel slice may sit this far beyond the model's error
MAX_FACTOR = 8          # no per-tensor exception goes beyond this; a ratio above it is a finding
FACTORS = {}            # tensor name -> factor, where a healthy route needs more than BOUND_FACTOR (with the measured reason)


@functools.lru_cache(maxsize=None)
def build_case(name):
    """A case computed once per process and shared by every test that reads it (nothing in it is written to): the truth, the
    rounding model and the model's error per slice of every tensor."""
    truth, model = truth64(name), rounding_model(name)
    assert set(truth) == set(model), (sorted(truth), sorted(model))
    err = {t: None if truth[t] is None else row_err(model[t], truth[t], slices_of(t, CASES[name]["M"])) for t in truth}
    return dict(CASES[name], truth=truth, model=model, model_err=err)


def judge(case, tensor, got):
    """(err per slice of `got` against the fp64 truth, the rounding model's, the worst ratio, the verdict). A slice passes when
    its error is at most the tensor's factor x the model's error on that slice; a slice whose truth is exactly zero (the model
    is exact there too) therefore has to be exactly zero. 0 / 0 counts as ratio 0."""
    c = case if isinstance(case, dict) else build_case(case)
    ref, model = c["truth"][tensor], c["model_err"][tensor]
    by = slices_of(tensor, c["M"])
    err = row_err(got, ref, by)
    zero = row_err(ref, torch.zeros_like(ref), by) == 0
    assert not bool((model[zero] != 0).any()), "the rounding model is not exact where the truth is zero"
    ratio = torch.where(err == 0, torch.zeros_like(err), err / model)
    factor = FACTORS.get(tensor, BOUND_FACTOR)
    assert BOUND_FACTOR <= factor <= MAX_FACTOR
    return err, model, float(ratio.max()), bool((err <= factor * model).all())
