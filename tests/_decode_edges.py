"""Helpers of the decode-attention key-range tests (tests/test_decode_edge_inputs.py on the host, tests/test_gpu_decode_edges.py on
the GPU): caches whose softmax mass sits ON the two ends of the key range of a decode step, an fp64 reference over a plain slice
of the cache, the four off-by-one ranges, and the case table. Nothing here imports the product: the range is written from the words
of the launchers' header (include/unsloth_amd.h, uamd_attn_decode): a step over `len` keys, the new token included, attends keys
[max(0, len - window), len) of the cache, all of them when there is no window. The error measure and its factor are the attention
edge tests' (tests/_attn_edges.py): one definition, one factor."""
import functools
import math

import torch

from tests._attn_edges import BOUND_FACTOR, DTYPES, row_err  # noqa: F401  (re-exported to the two test files)

S_MAX = 512

# id -> (D, Hq, Hk, split_keys, window (0: none), lens): one launch on a [len(lens), Hk, S_MAX, D] cache; a batch row b attends
# lens[b] keys, the new token (slot lens[b] - 1) included. KPB, the keys of one block-load, is 16 at D = 128 and 32 at D = 64;
# a split is `split_keys` keys; the single-launch kernel walks a split in trips of 128 keys. Workgroups = S_MAX / split_keys x
# Hk x B: up to 256 the single-launch kernel combines through granules, above through its arrival counter.
CASES = {
    # ---- D = 128 -------------------------------------------------------------------------------------------------------------
    # no window. 1: the new token is slot 0 (nothing cached before it) and the stale slot 1 scores higher; 16 / 17: the last slot
    # of a block-load / the first slot of the next
    "d128_len_1_16_17":     (128, 4, 4, 128, 0, (1, 16, 17)),
    # 128 / 129: the new key is the last of split 0 / alone in split 1; 512: it sits in the cache's last slot, no slot `len`
    "d128_len_128_129_512": (128, 8, 2, 128, 0, (128, 129, 512)),
    # first = 204: no multiple of 16, inside split 1; 20: shorter than the window, first = 0
    "d128_win96":           (128, 8, 4, 128, 96, (300, 20)),
    # first = 128: the first slot of a split (G = 7: head passes of the odd group size)
    "d128_win129_g7":       (128, 7, 1, 128, 129, (257,)),
    # first = 127: split 0 holds ONE valid key, in the last slot of its last wave-load
    "d128_win130":          (128, 8, 2, 128, 130, (257,)),
    # first = 129: the second slot of split 1
    "d128_win128":          (128, 4, 4, 128, 128, (257,)),
    # len > window is false: first = 0, every key counts
    "d128_win200_len200":   (128, 8, 4, 128, 200, (200,)),
    # first = 1
    "d128_win199_len200":   (128, 8, 2, 128, 199, (200,)),
    # first = 384: splits 0 - 2 are wholly masked and enter the combine as (-inf, 0)
    "d128_win16_len400":    (128, 4, 4, 128, 16, (400,)),
    # first = 383: one valid key on either side of a split boundary
    "d128_win2_len385":     (128, 8, 4, 128, 2, (385,)),
    # only the new key counts, and the key before it (code(len - 2)) scores higher
    "d128_win1":            (128, 8, 2, 128, 1, (130, 1, 129)),
    # 32 x 8 x 2 = 512 workgroups: the arrival-counter combine; first = 260 (inside a 16-key split) and 1
    "d128_split16_counter": (128, 16, 8, 16, 40, (300, 41)),
    # first = 300: in the second 128-key trip of split 1 of the single-launch kernel's chunked loop
    "d128_split256":        (128, 8, 2, 256, 100, (400,)),
    # ---- D = 64: the same edges at the 32-key block-load ---------------------------------------------------------------------
    "d64_len_1_31_32":      (64, 4, 4, 128, 0, (1, 31, 32)),
    "d64_len_33_128_129":   (64, 14, 2, 128, 0, (33, 128, 129)),        # G = 7
    "d64_len_512":          (64, 8, 2, 128, 0, (512,)),
    # first = 31, 32, 33: the last slot of a block-load, the first and the second of the next
    "d64_win100_first31_33":   (64, 8, 4, 128, 100, (131, 132, 133)),
    # first = 127, 128, 129: around the boundary of splits 0 and 1
    "d64_win130_first127_129": (64, 14, 2, 128, 130, (257, 258, 259)),
    # first = 384: three wholly masked splits
    "d64_win16_len400":     (64, 4, 4, 128, 16, (400,)),
    "d64_win1":             (64, 8, 2, 128, 1, (130, 1, 129)),
    # 16 x 8 x 2 = 256 workgroups: the largest launch that still combines through granules
    "d64_split32_granules": (64, 16, 8, 32, 40, (300, 41)),
    # 16 x 8 x 3 = 384 workgroups: the arrival counter
    "d64_split32_counter":  (64, 16, 8, 32, 40, (300, 41, 73)),
    "d64_split256":         (64, 8, 2, 256, 100, (400,)),
}

# The generator seed of a case: 2000, or the first seed after it at which the case meets the host conditions of
# tests/test_decode_edge_inputs.py (a chance correlation between two +-1 codes can hand the mass of a row to the wrong key, and
# removing a row's edge key moves it by little more than 0.5 to begin with). Found on the host, in fp64, without any kernel.
SEEDS = {"d128_win129_g7": 2007, "d128_win16_len400": 2001, "d64_win130_first127_129": 2001, "d64_win16_len400": 2001}

A_EDGE, B_FORBIDDEN = 1.0, 1.3     # x sqrt(128 / D): amplitude of the allowed key's code / of its forbidden neighbour's in a query
ROLES = {0: "first", 1: "last", 2: "middle", 3: "diffuse"}


def key_range(L, window):
    """(first, L): the keys a step over L keys attends -- [max(0, L - window), L), all of them without a window."""
    return (max(0, L - window) if window else 0), L


def mutants(first, L, S):
    """The four off-by-one ranges of [first, L) as [(name, first', L')]; those that leave [0, S] or hold no key are left out."""
    out = []
    for name, f, e in (("first-1", first - 1, L), ("first+1", first + 1, L), ("len+1", first, L + 1), ("len-1", first, L - 1)):
        if f >= 0 and e <= S and f < e:
            out.append((name, f, e))
    return out


def edge_inputs(case, dtype, seed):
    """(q [B, Hq * D], kc, vc [B, Hk, S_MAX, D], lens) in `dtype`. Keys are rows of i.i.d. +-1 (exact in both types) at EVERY slot
    of the cache, the slots outside [first, len) included: what an earlier prompt or the keys older than the window left there.
    v is randn. Query head h plays role h % 4 on the keys of its KV head, with code(i) = 0 for i outside [0, S_MAX):
      0: a code(first) + b code(first - 1)                               the oldest allowed key carries the mass, its forbidden
                                                                         neighbour would carry more
      1: a code(len - 1) + b code(len)                                   the new token carries it, the stale slot after it would
      2: a code((first + len - 1) // 2) + b code(first - 1) + b code(len)      mass in the middle, both forbidden neighbours would
      3: randn                                                           the diffuse control
    plus 0.25 randn on every head; a = 1.0 sqrt(128 / D), b = 1.3 sqrt(128 / D): after the 1 / sqrt(D) scale the allowed key
    scores about 11.3, a forbidden one about 14.7, every other key about +-1.7."""
    D, Hq, Hk, _, window, lens = case
    B, G = len(lens), Hq // Hk
    gen = torch.Generator().manual_seed(seed)
    kc = (torch.randint(0, 2, (B, Hk, S_MAX, D), generator=gen) * 2 - 1).float()
    vc = torch.randn(B, Hk, S_MAX, D, generator=gen)
    a, b = A_EDGE * math.sqrt(128 / D), B_FORBIDDEN * math.sqrt(128 / D)
    q = torch.empty(B, Hq, D)
    for bi, L in enumerate(lens):
        first, _ = key_range(L, window)

        def code(i, kh):
            return kc[bi, kh, i] if 0 <= i < S_MAX else torch.zeros(D)

        for h in range(Hq):
            kh, role = h // G, h % 4
            if role == 0:
                x = a * code(first, kh) + b * code(first - 1, kh)
            elif role == 1:
                x = a * code(L - 1, kh) + b * code(L, kh)
            elif role == 2:
                x = a * code((first + L - 1) // 2, kh) + b * code(first - 1, kh) + b * code(L, kh)
            else:
                x = torch.randn(D, generator=gen)
            q[bi, h] = x + 0.25 * torch.randn(D, generator=gen)
    return q.flatten(1).to(dtype), kc.to(dtype), vc.to(dtype), tuple(lens)


def ref64_ranges(q, kc, vc, ranges, scale, Hq, Hk):
    """fp64 attention of one token per batch row over the slice ranges[b] = (first, end) of its caches: [B, Hq, D]."""
    B, D, G = q.shape[0], kc.shape[-1], Hq // Hk
    qd = q.detach().double().cpu().view(B, Hq, D)
    out = torch.empty(B, Hq, D, dtype=torch.float64)
    for b, (f, e) in enumerate(ranges):
        for h in range(Hq):
            k = kc[b, h // G, f:e].detach().double().cpu()
            v = vc[b, h // G, f:e].detach().double().cpu()
            out[b, h] = torch.softmax((k @ qd[b, h]) * scale, dim=0) @ v
    return out


def ref64(q, kc, vc, lens, window, scale, Hq, Hk):
    """The reference of a decode step: per (batch row, head) an fp64 softmax over keys [max(0, len - window), len) of the inputs
    as they are (already rounded to the 16-bit type), by plain slicing."""
    return ref64_ranges(q, kc, vc, [key_range(L, window) for L in lens], scale, Hq, Hk)


def edge_mass(q, kc, lens, window, scale, Hq, Hk):
    """{(b, h): softmax mass (fp64) the reference puts on the edge key of head h's role} for the heads in role 0 (key `first`) and
    role 1 (key len - 1)."""
    B, D, G = q.shape[0], kc.shape[-1], Hq // Hk
    qd = q.double().view(B, Hq, D)
    out = {}
    for b, L in enumerate(lens):
        first, _ = key_range(L, window)
        for h in range(Hq):
            if h % 4 in (0, 1):
                p = torch.softmax((kc[b, h // G, first:L].double() @ qd[b, h]) * scale, dim=0)
                out[(b, h)] = float(p[0] if h % 4 == 0 else p[-1])
    return out


def role_heads(Hq, role):
    return [h for h in range(Hq) if h % 4 == role]


def shift_of_rows(other, ref, b, heads):
    """row_err of `ref` with the rows (b, heads) replaced by `other`'s: how far those rows moved, in the units (and with the rms
    term over ALL rows of the case) in which the GPU tests hold the kernels."""
    got = ref.clone()
    got[b, heads] = other[b, heads].to(got.dtype)
    return row_err(got, ref)


@functools.lru_cache(maxsize=None)
def build_case(name, dtype_name):
    """One case of the table, computed once per process and shared by every test that reads it (nothing in it is written to): the
    inputs, the fp64 reference [B, Hq, D] and `model_err`, the row error of that reference rounded once to the 16-bit type -- the
    only rounding the kernels document for the decode output (fp32 scores, fp32 exp2, fp32 sums, one rounding at the store)."""
    case = CASES[name]
    D, Hq, Hk, split_keys, window, lens = case
    assert Hq % Hk == 0 and Hq >= 4 and S_MAX % split_keys == 0 and all(1 <= L <= S_MAX for L in lens)
    dtype = DTYPES[dtype_name]
    q, kc, vc, lens = edge_inputs(case, dtype, SEEDS.get(name, 2000))
    scale = 1.0 / math.sqrt(D)
    ref = ref64(q, kc, vc, lens, window, scale, Hq, Hk)
    model = ref.to(dtype).double()
    return dict(D=D, Hq=Hq, Hk=Hk, B=len(lens), split_keys=split_keys, window=window, lens=lens, dtype=dtype,
                ranges=[key_range(L, window) for L in lens], q=q, kc=kc, vc=vc, scale=scale, ref=ref, model=model,
                model_err=row_err(model, ref))


def judge(c, got):
    """(row_err of `got` [B, Hq * D] against the case's fp64 reference, the model's, whether the first is within BOUND_FACTOR x the
    second). A range of one key has model_err 0 -- the output IS that v row -- and the rule asks for equality."""
    err = row_err(got.detach().cpu().view(c["B"], c["Hq"], c["D"]), c["ref"])
    return err, c["model_err"], bool(err <= BOUND_FACTOR * c["model_err"])
