"""Helpers of the FP8 KV-cache tests (tests/test_kv_fp8_host.py on the host, tests/test_gpu_kv_fp8.py and
tests/test_gpu_decode_fp8.py on the GPU): the torch restatement of the stored format of include/unsloth_amd.h, the inputs of the
bitwise quantiser tests, and the decode edge-case table (tests/_decode_edges.py) over quantised caches. Nothing here imports the
product.

The format: a cache row x of D values (already rounded to the activation type, taken as fp32) is D e4m3fn codes and one fp32 scale:
amax = max |x_j|; scale = amax / 448 (IEEE fp32 division) when amax > 0, else 1; code_j = e4m3fn_rne(clamp(x_j / scale, -448, 448));
a row with a non-finite element has scale = NaN (codes unspecified). Dequantised: float(code_j) * scale, exactly."""
import functools

import torch

from tests import _decode_edges as E

FP8_MAX = 448.0
F8 = torch.float8_e4m3fn


def quantize_ref(x):
    """(codes float8_e4m3fn [..., D], scale fp32 [...]) of rows x [..., D] on the CPU. Both divisions are tensor / tensor in fp32
    (IEEE); torch's cast to float8_e4m3fn rounds to nearest even and keeps the sign of zero."""
    xf = x.detach().float().cpu()
    amax = xf.abs().amax(dim=-1)
    scale = torch.where(amax > 0, amax / torch.full_like(amax, FP8_MAX), torch.ones_like(amax))
    scale = torch.where(torch.isfinite(xf).all(dim=-1), scale, torch.full_like(amax, float("nan")))
    codes = (xf / scale[..., None]).clamp(-FP8_MAX, FP8_MAX).to(F8)
    return codes, scale


def dequantize_ref(codes, scale):
    """float(code) * scale in fp64: exact (a 4-bit significand times a 24-bit one)."""
    return codes.double() * scale.double()[..., None]


def round_trip(x):
    """x through the cache format and back, rounded once to x's type: what a 16-bit cache would hold if it had been FP8."""
    codes, scale = quantize_ref(x)
    return dequantize_ref(codes, scale).to(x.dtype)


def as_bytes(codes):
    return codes.view(torch.uint8)


def every_value_rows(dtype, D):
    """Every finite value of `dtype` (bf16 / fp16) with |x| <= 448, both zeros included, packed D - 1 to a row whose last element
    is 448: the row's scale is exactly 1 and its codes are the e4m3fn roundings of the values themselves. [rows, D]; the last
    row is filled up with zeros."""
    allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    keep = allv[torch.isfinite(allv.float()) & (allv.float().abs() <= FP8_MAX)]
    n = D - 1
    rows = (keep.numel() + n - 1) // n
    body = torch.zeros(rows * n, dtype=dtype)
    body[:keep.numel()] = keep
    out = torch.full((rows, D), FP8_MAX, dtype=dtype)
    out[:, :n] = body.view(rows, n)
    return out


# ---- the decode edge-case table over quantised caches ------------------------------------------------------------------------------
# The generator seed of a case here: the table's own (tests/_decode_edges.SEEDS, default 2000) unless the case misses the host
# conditions of tests/test_kv_fp8_host.py over the DEQUANTISED caches; then the first seed after it that meets them (found on the
# host, in fp64, without any kernel).
# d128_split16_counter: at the table's seed 2000 the bf16 reference over the dequantised caches lies 11.9 x model_err from the 16-bit
# one, the condition asks for 12 (3 GPU bounds); at 2001 it is 15.7 x (fp16: 120 x), least off-by-one shift 0.57.
SEEDS = dict(E.SEEDS, d128_split16_counter=2001)


@functools.lru_cache(maxsize=None)
def build_case(name, dtype_name):
    """A case of tests/_decode_edges.CASES with its caches in the FP8 format: the table's inputs (q, and kc / vc before
    quantisation), `k8` / `v8` = (codes, scale) of the reference quantiser, `kd` / `vd` the dequantised caches in fp64, `ref` the
    fp64 reference over THOSE (E.ref64), `model_err` the row error of that reference rounded once to the 16-bit type, and `ref16`
    the reference over the 16-bit caches. Computed once per process; nothing in it is written to."""
    case = E.CASES[name]
    D, Hq, Hk, split_keys, window, lens = case
    dtype = E.DTYPES[dtype_name]
    seed = SEEDS.get(name, 2000)
    if seed == E.SEEDS.get(name, 2000):
        c16 = E.build_case(name, dtype_name)
        q, kc, vc, ref16 = c16["q"], c16["kc"], c16["vc"], c16["ref"]
    else:
        q, kc, vc, lens = E.edge_inputs(case, dtype, seed)
        ref16 = E.ref64(q, kc, vc, lens, window, 1.0 / D ** 0.5, Hq, Hk)
    scale = 1.0 / D ** 0.5
    k8, v8 = quantize_ref(kc), quantize_ref(vc)
    kd, vd = dequantize_ref(*k8), dequantize_ref(*v8)
    ref = E.ref64(q, kd, vd, lens, window, scale, Hq, Hk)
    model = ref.to(dtype).double()
    return dict(D=D, Hq=Hq, Hk=Hk, B=len(lens), split_keys=split_keys, window=window, lens=tuple(lens), dtype=dtype,
                ranges=[E.key_range(L, window) for L in lens], q=q, kc=kc, vc=vc, k8=k8, v8=v8, kd=kd, vd=vd, scale=scale,
                ref=ref, ref16=ref16, model=model, model_err=E.row_err(model, ref))
