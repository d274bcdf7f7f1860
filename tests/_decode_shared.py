"""Helpers of the shared-prompt decode attention tests (tests/test_decode_shared_host.py on the host, tests/test_gpu_decode_shared.py
on the GPU): P prompts whose K / V are stored once, n rows per prompt that each own a suffix cache, the softmax mass placed ON the
ends of the key range and on the seam between the two caches, an fp64 reference, the off-by-one ranges and the case table. Nothing
here imports the product: the range is written from the words of the header (include/unsloth_amd.h, uamd_attn_decode_shared): row
r = p n + i attends the keys [max(0, total - window), total) of the concatenation prompt[:L_p] | suffix[:new], total = L_p + new,
all of them without a window. The reference concatenates exactly that into an ordinary per-row cache and calls the decode edge
tests' fp64 slice reference (tests/_decode_edges.ref64_ranges); error measure and factor are the attention edge tests'."""
import functools
import math

import torch

from tests._attn_edges import BOUND_FACTOR, DTYPES, row_err  # noqa: F401  (re-exported to the two test files)
from tests._decode_edges import A_EDGE, B_FORBIDDEN, judge, ref64_ranges, role_heads, shift_of_rows  # noqa: F401

S_P, S_N = 512, 256          # slots of a prompt cache / of a row's suffix cache

# id -> (D, Hq, Hk, n, split_keys, window (0: none), prompt lengths (one per prompt of the launch), new): `new` keys of every
# row's suffix count, the new token included -- one number, or one per row. KPB, the keys of a block-load, is 16 at D = 128 and
# 32 at D = 64; the prefix scan fills its LDS with 128 keys and walks them 32 at a time, a query tile is 16 rows of the R = n G.
CASES = {
    # ---- D = 128 -------------------------------------------------------------------------------------------------------------
    # R = 2 rows of a 16-row tile; the suffix holds the new key alone; prompts of 1 key, a whole block-load, one key more
    "d128_r2_new1":          (128, 4, 4, 2, 128, 0, (1, 16, 17), 1),
    # R = 21: a second tile of 5 rows; the prompt ends on the split seam / one key into split 1
    "d128_r21_split_seam":   (128, 7, 1, 3, 128, 0, (128, 129), 2),
    # R = 128: every wave two full tiles; both caches full to their last slots (no stale slot behind either)
    "d128_r128_last_slots":  (128, 8, 1, 16, 128, 0, (512,), 256),
    # the suffix ends on its split seam / crosses it
    "d128_suffix128":        (128, 8, 2, 8, 128, 0, (33, 200), 128),
    "d128_suffix129":        (128, 8, 2, 8, 128, 0, (33, 200), 129),
    # the two rows of one group at different suffix lengths (the engine never does this; the kernel reads new_len per row)
    "d128_rows_differ":      (128, 4, 2, 2, 128, 0, (40,), (1, 129)),
    # first = 204: no multiple of 16, inside prompt split 1
    "d128_win101_first204":  (128, 8, 2, 4, 128, 101, (300,), 5),
    # first = 127 / 128 / 129: the last key of prompt split 0, the first and the second of split 1
    "d128_win131_first127":  (128, 8, 2, 4, 128, 131, (257,), 1),
    "d128_win130_first128":  (128, 8, 2, 4, 128, 130, (257,), 1),
    "d128_win129_first129":  (128, 8, 2, 4, 128, 129, (257,), 1),
    # first = L_p - 1 (one prompt key left) / L_p (the prompt scan has nothing) / inside the suffix / only the new key
    "d128_win8_first_lp-1":  (128, 8, 4, 4, 128, 8, (130,), 7),
    "d128_win7_first_lp":    (128, 8, 4, 4, 128, 7, (130,), 7),
    "d128_win3_in_suffix":   (128, 8, 4, 4, 128, 3, (130,), 7),
    "d128_win1_new_key":     (128, 8, 4, 4, 128, 1, (130,), 7),
    # window >= total: first = 0, every key counts
    "d128_win400_total300":  (128, 8, 4, 4, 128, 400, (200,), 100),
    # ---- D = 64: the 32-key block-load -------------------------------------------------------------------------------------------
    "d64_r2_len_31_32_33":   (64, 4, 4, 2, 128, 0, (31, 32, 33), 1),
    "d64_g7_r21":            (64, 14, 2, 3, 128, 0, (128, 129), 33),
    # first = 31 / 32 / 33
    "d64_win100_first31":    (64, 8, 4, 4, 128, 100, (100,), 31),
    "d64_win99_first32":     (64, 8, 4, 4, 128, 99, (100,), 31),
    "d64_win98_first33":     (64, 8, 4, 4, 128, 98, (100,), 31),
    "d64_r128_last_slots":   (64, 16, 2, 16, 128, 0, (512,), 256),
}

# The generator seed of a case: 3000, or the first seed after it at which the case meets the host conditions of
# tests/test_decode_shared_host.py. Found on the host, in fp64, without any kernel.
SEEDS = {"d64_r2_len_31_32_33": 3001}


def geometry(case):
    """(P, B, per-row prompt index, per-row prompt length, per-row new, per-row (first, total)) of a case."""
    D, Hq, Hk, n, _, window, lens, new = case
    P = len(lens)
    B = P * n
    news = tuple(new) if isinstance(new, (tuple, list)) else (new,) * B
    assert len(news) == B
    rows_p = [r // n for r in range(B)]
    rows_L = [lens[p] for p in rows_p]
    ranges = []
    for r in range(B):
        total = rows_L[r] + news[r]
        ranges.append(((max(0, total - window) if window else 0), total))
    return P, B, rows_p, rows_L, news, ranges


def concat_caches(pk, pv, sk, sv, rows_p, prompt_keys, suffix_keys):
    """The ordinary per-row caches [B, Hk, S_P + 1 + S_N, D] (fp64; zeros behind): row r holds the first prompt_keys[r] slots of
    its prompt's cache followed by the first suffix_keys[r] slots of its own suffix cache."""
    B, Hk, _, D = sk.shape
    kc = torch.zeros(B, Hk, S_P + 1 + S_N, D, dtype=torch.float64)
    vc = torch.zeros_like(kc)
    for r in range(B):
        a, s = prompt_keys[r], suffix_keys[r]
        kc[r, :, :a], vc[r, :, :a] = pk[rows_p[r], :, :a].double(), pv[rows_p[r], :, :a].double()
        kc[r, :, a:a + s], vc[r, :, a:a + s] = sk[r, :, :s].double(), sv[r, :, :s].double()
    return kc, vc


def shared_inputs(case, dtype, seed):
    """(q [B, Hq * D], pk, pv [P, Hk, S_P, D], sk, sv [B, Hk, S_N, D]) in `dtype`. Keys are rows of i.i.d. +-1 (exact in both
    types) at EVERY slot of both caches, the stale ones included; v is randn. With cat(i) = key i of the row's concatenation
    prompt[:L_p] | suffix[:S_N] (so cat(total) is the stale suffix slot `new`; zero outside) and stale_p = prompt slot L_p -- the
    stale tail of the shared prompt cache -- query head h of row r plays role h % 4 on its KV head:
      0: a cat(first) + b cat(first - 1)                              the oldest allowed key carries the mass, its forbidden
                                                                      neighbour would carry more
      1: a cat(total - 1) + b cat(total)                              the new token carries it, the stale slot behind it would
      2: a cat(seam) + b cat(first - 1) + b cat(total) + b stale_p    seam = the last prompt key L_p - 1 on even rows, the first
                                                                      suffix slot L_p on odd ones (the middle of the range where
                                                                      that key is outside it); all three forbidden slots would
      3: randn                                                        the diffuse control
    plus the row's own 0.25 randn on every head, so the n rows of a group differ; a, b as in tests/_decode_edges.py."""
    D, Hq, Hk, n, _, window, lens, _ = case
    P, B, rows_p, rows_L, news, ranges = geometry(case)
    G = Hq // Hk
    gen = torch.Generator().manual_seed(seed)
    pk = (torch.randint(0, 2, (P, Hk, S_P, D), generator=gen) * 2 - 1).float()
    pv = torch.randn(P, Hk, S_P, D, generator=gen)
    sk = (torch.randint(0, 2, (B, Hk, S_N, D), generator=gen) * 2 - 1).float()
    sv = torch.randn(B, Hk, S_N, D, generator=gen)
    a, b = A_EDGE * math.sqrt(128 / D), B_FORBIDDEN * math.sqrt(128 / D)
    q = torch.empty(B, Hq, D)
    for r in range(B):
        p, L = rows_p[r], rows_L[r]
        first, total = ranges[r]

        def cat(i, kh):
            if 0 <= i < L:
                return pk[p, kh, i]
            return sk[r, kh, i - L] if L <= i < L + S_N else torch.zeros(D)

        for h in range(Hq):
            kh, role = h // G, h % 4
            if role == 0:
                x = a * cat(first, kh) + b * cat(first - 1, kh)
            elif role == 1:
                x = a * cat(total - 1, kh) + b * cat(total, kh)
            elif role == 2:
                x = a * cat(seam_key(r, L, first, total), kh) + b * cat(first - 1, kh) + b * cat(total, kh)
                if L < S_P:
                    x = x + b * pk[p, kh, L]
            else:
                x = torch.randn(D, generator=gen)
            q[r, h] = x + 0.25 * torch.randn(D, generator=gen)
    return q.flatten(1).to(dtype), pk.to(dtype), pv.to(dtype), sk.to(dtype), sv.to(dtype)


def seam_key(r, L, first, total):
    """The key (index in the concatenation) that carries the mass of row r's role-2 heads."""
    k = L - 1 if r % 2 == 0 else L
    return k if first <= k < total else (first + total - 1) // 2


def mutants(c):
    """The wrong key ranges a shared-prompt kernel can fall into, as [(name, roles that watch it, rows it applies to, (kc, vc,
    ranges))] over per-row concatenations built for it. The four off-by-one ends of tests/_decode_edges.py; the prompt cache read
    one slot too far (`prompt+1`: slot L_p, the stale tail) or one short (`prompt-1`: the seam key L_p - 1 is lost -- watched by
    the even rows, whose role-2 heads sit on it); and `shifted`: a prompt scan that places the window without the suffix, first' =
    max(0, L_p - window) -- a suffix scan that subtracts the prompt twice reads the same range."""
    B, rows_p, rows_L, news, ranges, window = c["B"], c["rows_p"], c["rows_L"], c["news"], c["ranges"], c["window"]
    base = concat_caches(c["pk"], c["pv"], c["sk"], c["sv"], rows_p, rows_L, [S_N] * B)
    out = []

    def add(name, roles, rows, caches, rng):
        rows = [r for r in rows if rng[r] is not None]
        if rows:
            out.append((name, roles, rows, caches, [rng[r] if rng[r] is not None else ranges[r] for r in range(B)]))

    rows = list(range(B))
    add("first-1", (0, 2), rows, base, [(f - 1, t) if f > 0 else None for f, t in ranges])
    add("first+1", (0,), rows, base, [(f + 1, t) if t - f > 1 else None for f, t in ranges])
    add("total+1", (1, 2), rows, base, [(f, t + 1) if news[r] < S_N else None for r, (f, t) in enumerate(ranges)])
    add("total-1", (1,), rows, base, [(f, t - 1) if t - f > 1 else None for f, t in ranges])
    longer = concat_caches(c["pk"], c["pv"], c["sk"], c["sv"], rows_p, [min(L + 1, S_P) for L in rows_L], news)
    add("prompt+1", (2,), rows, longer,
        [(f, t + 1) if rows_L[r] < S_P and f <= rows_L[r] else None for r, (f, t) in enumerate(ranges)])
    shorter = concat_caches(c["pk"], c["pv"], c["sk"], c["sv"], rows_p, [L - 1 for L in rows_L], news)
    add("prompt-1", (2,), [r for r in rows if r % 2 == 0], shorter,
        [(f, t - 1) if f <= rows_L[r] - 1 and t - 1 > f else None for r, (f, t) in enumerate(ranges)])
    if window:
        add("shifted", (0, 2), rows, base,
            [(max(0, rows_L[r] - window), t) if max(0, rows_L[r] - window) != f else None for r, (f, t) in enumerate(ranges)])
    return out


def rounding_model(q, kc, vc, ranges, scale, Hq, Hk, dtype):
    """The fp64 reference with the roundings uamd_attn_decode_shared documents for its prefix scan, applied to every key: P =
    exp2(s - max) rounded once to `dtype`, the sum taken over the ROUNDED P, and one rounding at the store. (The suffix scan keeps
    P in fp32; the model is the yardstick of what a correct kernel may lose, not a model of its schedule.) [B, Hq, D] fp64."""
    B, D, G = q.shape[0], kc.shape[-1], Hq // Hk
    qd = q.detach().double().view(B, Hq, D)
    out = torch.empty(B, Hq, D, dtype=torch.float64)
    for b, (f, e) in enumerate(ranges):
        for h in range(Hq):
            s = (kc[b, h // G, f:e] @ qd[b, h]) * (scale * math.log2(math.e))
            p = torch.exp2(s - s.max()).to(dtype).double()
            out[b, h] = ((p @ vc[b, h // G, f:e]) / p.sum()).to(dtype).double()
    return out


@functools.lru_cache(maxsize=None)
def build_case(name, dtype_name):
    """One case of the table, computed once per process and shared by every test that reads it (nothing in it is written to)."""
    case = CASES[name]
    D, Hq, Hk, n, split_keys, window, lens, _ = case
    P, B, rows_p, rows_L, news, ranges = geometry(case)
    assert Hq % Hk == 0 and Hq >= 4 and 2 <= n <= 16 and S_P % split_keys == 0 and S_N % split_keys == 0
    assert all(1 <= L <= S_P for L in lens) and all(1 <= m <= S_N for m in news)
    dtype = DTYPES[dtype_name]
    q, pk, pv, sk, sv = shared_inputs(case, dtype, SEEDS.get(name, 3000))
    scale = 1.0 / math.sqrt(D)
    kc, vc = concat_caches(pk, pv, sk, sv, rows_p, rows_L, news)
    ref = ref64_ranges(q, kc, vc, ranges, scale, Hq, Hk)
    model = rounding_model(q, kc, vc, ranges, scale, Hq, Hk, dtype)
    return dict(D=D, Hq=Hq, Hk=Hk, n=n, P=P, B=B, split_keys=split_keys, window=window, lens=tuple(lens), news=news,
                rows_p=rows_p, rows_L=rows_L, ranges=ranges, dtype=dtype, q=q, pk=pk, pv=pv, sk=sk, sv=sv, scale=scale,
                ref=ref, model=model, model_err=row_err(model, ref))


def cache_bytes(layers, Hk, D, itemsize, P, n, S_prompt, S_new, S_replicated):
    """(bytes of the shared layout, bytes of the replicated one): K and V of every layer."""
    per = 2 * layers * Hk * D * itemsize
    return per * (P * S_prompt + P * n * S_new), per * P * n * S_replicated
