"""Reference logic of prompt-lookup decoding for tests/test_lookup_host.py and tests/test_gpu_decode_lookup.py, written from the
rules in include/unsloth_amd.h (uamd_ngram_draft, uamd_accept_greedy) in plain python. Imports nothing of the product."""


def draft(hist, K, n_max):
    """(tok, n_draft): tok[0] = the last token, tok[1 .. n_draft] = what followed the LATEST earlier occurrence of the longest
    suffix n-gram (n = n_max .. 1) that has one, at most K tokens, then zeros up to K + 1 entries."""
    L = len(hist)
    found = []
    for n in range(min(n_max, L - 1), 0, -1):
        suffix = hist[L - n:]
        starts = [i for i in range(0, L - n) if hist[i:i + n] == suffix]       # i + n <= L - 1
        if starts:
            i = max(starts)
            found = hist[i + n:min(i + n + K, L)]
            break
    return [hist[-1] if L else 0] + list(found) + [0] * (K - len(found)), len(found)


def accept(tok, a, eos, remaining):
    """(m, done): a[j] is the model's token after tok[0 .. j]. m = leading drafts j = 1 .. K with tok[j] == a[j - 1]; nothing is
    accepted behind an a[j - 1] that is an eos id; m + 1 <= remaining. a[0 .. m] are emitted; done: an eos among them, or
    nothing remains."""
    K = len(tok) - 1
    m = 0
    stop = a[0] in eos
    while not stop and m < K and m + 1 < remaining and tok[m + 1] == a[m]:
        m += 1
        stop = a[m] in eos
    return m, bool(stop or remaining - (m + 1) <= 0)


def replay(seq, T, K, n_max, eos=(), max_new_tokens=None):
    """What the verify steps do when the model's greedy text is seq (prompt seq[:T], then the emitted tokens): the first
    token comes from prefill, then every step drafts from the tokens so far and keeps the drafts that equal the text. Returns
    (stats, tokens emitted per step, number of new tokens the steps account for). While the drafts so far matched, the model's
    arg-max behind draft j is the text's next token, so the text alone decides every step."""
    new = len(seq) - T
    max_new_tokens = new if max_new_tokens is None else max_new_tokens
    stats = dict(steps=0, drafted=0, accepted=0, tokens=0)
    per_step = []
    L, remaining = T + 1, max_new_tokens - 1
    done = seq[T] in eos or remaining <= 0
    while not done:
        tok, nd = draft(list(seq[:L]), K, n_max)
        # the arg-max rows: the text while the drafts agree with it; behind the first wrong draft they no longer matter
        a = [seq[L + j] if L + j < len(seq) else -1 for j in range(K + 1)]
        m, done = accept(tok, a, eos, remaining)
        assert L + m + 1 <= len(seq), "the text is shorter than what the steps emit"
        L, remaining = L + m + 1, remaining - (m + 1)
        stats["steps"] += 1
        stats["drafted"] += nd
        stats["accepted"] += m
        stats["tokens"] += m + 1
        per_step.append(m + 1)
    return stats, per_step, L - T


# hand-written cases: (name, hist, K, n_max, tok, n_draft)
DRAFT_CASES = [
    ("no match", [1, 2, 3, 4, 5], 3, 3, [5, 0, 0, 0], 0),
    ("n = 3 beats n = 1", [7, 1, 2, 3, 9, 5, 3, 8, 1, 2, 3], 3, 3, [3, 9, 5, 3], 3),
    ("the most recent match wins", [4, 5, 6, 4, 5, 7, 4, 5], 3, 2, [5, 7, 4, 5], 3),
    ("a continuation shorter than K", [1, 2, 3, 1, 2], 4, 2, [2, 3, 1, 2, 0], 3),
    ("a match overlapping the suffix", [1, 2, 1, 2, 1, 2, 1, 2], 3, 3, [2, 1, 2, 0], 2),
    ("len <= n", [5, 5], 2, 3, [5, 5, 0], 1),
    ("len 1", [9], 2, 2, [9, 0, 0], 0),
    ("K = 15, one token of context repeated", [3] * 40, 15, 2, [3] * 2 + [0] * 14, 1),
]

# (name, tok, a, eos, remaining, m, done)
ACCEPT_CASES = [
    ("m = K", [5, 6, 7, 8], [6, 7, 8, 9], [], 10, 3, False),
    ("first draft wrong", [5, 1, 7, 8], [6, 7, 8, 9], [], 10, 0, False),
    ("second draft wrong", [5, 6, 1, 8], [6, 7, 8, 9], [], 10, 1, False),
    ("eos at a[0]", [5, 2, 7, 8], [2, 7, 8, 9], [2], 10, 0, True),
    ("eos mid-draft", [5, 6, 2, 8], [6, 2, 8, 9], [4, 2], 10, 1, True),
    ("eos as the last emitted token", [5, 6, 7, 8], [6, 7, 8, 2], [2], 10, 3, True),
    ("remaining = 1", [5, 6, 7, 8], [6, 7, 8, 9], [], 1, 0, True),
    ("remaining = 3 cuts m = K", [5, 6, 7, 8], [6, 7, 8, 9], [], 3, 2, True),
    ("remaining = m + 1 exactly", [5, 6, 7, 8], [6, 7, 8, 9], [], 4, 3, True),
    ("zero slots are drafts too", [5, 6, 0, 0], [6, 0, 0, 3], [], 10, 3, False),
]


# ---- the span attention: R new tokens of one sequence, row j over keys [max(0, t_j - window), t_j), t_j = kv_len + j + 1 ---------
S_MAX = 512
SPLIT = 128

# id -> (Hq, Hk, R, window (0: none), kv_len); every case runs at head dim 64 and 128 and in both 16-bit types. A fill is 128
# keys, a score group 32, a split SPLIT keys; the R keys of the span sit at slots kv_len .. kv_len + R - 1.
SPAN_CASES = {
    "len0":          (4, 1, 4, 0, 0),         # row 0's only key is its own
    "len1":          (4, 1, 4, 0, 1),
    "len15":         (4, 1, 4, 0, 15),        # the span crosses the first 16-key half of a group
    "len16":         (4, 1, 4, 0, 16),
    "len17":         (4, 1, 4, 0, 17),
    "len31":         (4, 1, 4, 0, 31),        # ... and the group's end
    "len32":         (4, 1, 4, 0, 32),
    "len33":         (4, 1, 4, 0, 33),
    "len120_r16":    (4, 1, 16, 0, 120),      # rows straddle the split seam and the 128-key fill
    "len496_r16":    (4, 1, 16, 0, 496),      # the cache's last slots
    "g1":            (4, 4, 16, 0, 200),      # one 16-row tile holds all 16 tokens of a head
    "g7":            (7, 1, 5, 0, 130),       # tiles cut tokens in the middle of a group
    "g8_r16":        (8, 1, 16, 0, 250),      # 128 query rows: all 8 tiles
    "r1":            (4, 2, 1, 0, 77),
    "win100":        (4, 1, 4, 100, 200),     # every row's first key in the old cache
    "win3":          (4, 1, 4, 3, 200),       # first keys: old cache (j = 0, 1), kv_len itself (j = 2), a new key (j = 3)
    "win3_seam":     (8, 2, 16, 3, 121),      # the same across the split seam, two 16-row tiles per KV head
    "win1":          (4, 1, 4, 1, 129),       # only the row's own key
}


def span_ranges(R, window, kv_len):
    return [((max(0, kv_len + j + 1 - window) if window else 0), kv_len + j + 1) for j in range(R)]


def span_inputs(case, D, dtype, seed):
    """(q [R, Hq * D], kc, vc [1, Hk, S_MAX, D]) in `dtype`, built like tests/_decode_edges.edge_inputs: keys are +-1 codes at EVERY
    slot (stale slots behind the span included), v is randn, and the query of (token j, head h) plays role (h + j) % 4 on its own
    range [first, t): 0 -- mass on key `first`, the key before it would take more; 1 -- mass on the row's own key t - 1, key t
    (the NEXT token's, or the stale slot behind the span) would take more; 2 -- mass in the middle, both outside neighbours
    would take more; 3 -- diffuse."""
    import math
    import torch
    Hq, Hk, R, window, kv_len = case
    G = Hq // Hk
    gen = torch.Generator().manual_seed(seed)
    kc = (torch.randint(0, 2, (1, Hk, S_MAX, D), generator=gen) * 2 - 1).float()
    vc = torch.randn(1, Hk, S_MAX, D, generator=gen)
    a, b = 1.0 * math.sqrt(128 / D), 1.3 * math.sqrt(128 / D)
    q = torch.empty(R, Hq, D)
    for j, (first, t) in enumerate(span_ranges(R, window, kv_len)):
        for h in range(Hq):
            def code(i):
                return kc[0, h // G, i] if 0 <= i < S_MAX else torch.zeros(D)
            role = (h + j) % 4
            if role == 0:
                x = a * code(first) + b * code(first - 1)
            elif role == 1:
                x = a * code(t - 1) + b * code(t)
            elif role == 2:
                x = a * code((first + t - 1) // 2) + b * code(first - 1) + b * code(t)
            else:
                x = torch.randn(D, generator=gen)
            q[j, h] = x + 0.25 * torch.randn(D, generator=gen)
    return q.flatten(1).to(dtype), kc.to(dtype), vc.to(dtype)
