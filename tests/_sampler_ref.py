"""Host reference of the device sampler (csrc/sampler.hip, uamd_sample_f32), test-only: numpy, fp64 masses over the fp32 scaled
logits. Philox4x32-10, the kept set of temperature -> top-k -> top-p -> min-p by the rule the header states (ties stay or go as
a group), the CDF intervals of the kept tokens in vocabulary order, and the inputs the GPU tests use together with the margins
that make their kept sets independent of fp32-against-fp64 rounding (tests/test_sampler_ref_host.py asserts them)."""
import functools

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: 4 words, key: 2 words -> 4 words (Salmon et al., Random123)."""
    c0, c1, c2, c3 = (int(c) & MASK for c in ctr)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, draw, row):
    """The kernel's u for (seed, draw counter, row): fp32 (x0 >> 8) * 2^-24."""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    x0 = philox4x32_10((draw & MASK, draw >> 32, row, 0), (seed & MASK, seed >> 32))[0]
    return np.float32((x0 >> 8) * 2.0 ** -24)


def scaled(x, T):
    """z = x / T in fp32 (IEEE), -0 folded into +0."""
    with np.errstate(all="ignore"):
        z = np.asarray(x, np.float32) / np.float32(T)
    z[z == 0] = 0.0
    return z


def kept_set(z, top_k=0, top_p=1.0, min_p=0.0):
    """bool [V]: the kept set of fp32 scaled logits z. -inf, +inf and NaN are never kept."""
    z = np.asarray(z, np.float32)
    V = z.shape[0]
    fin = np.isfinite(z)
    keep = fin.copy()
    if not fin.any():
        return keep
    zd = z.astype(np.float64)
    zmax = zd[fin].max()
    if 0 < top_k < V and top_k <= int(fin.sum()):
        kth = np.sort(zd[fin])[::-1][top_k - 1]
        keep &= zd >= kth
    top_p = np.float32(top_p)
    if top_p < 1.0:
        idx = np.nonzero(keep)[0]
        order = idx[np.argsort(zd[idx], kind="stable")]                  # ascending
        zs = zd[order]
        cum = np.cumsum(np.exp(zs - zmax))
        at_or_below = cum[np.searchsorted(zs, zs, side="right") - 1]      # mass of everything with z <= own, ties included
        goes = at_or_below <= (1.0 - np.float64(top_p)) * cum[-1]
        goes[zs == zmax] = False
        keep[order[goes]] = False
    min_p = np.float32(min_p)
    if min_p > 0.0:
        keep &= zd >= zmax + np.log(np.float64(min(min_p, np.float32(1.0))))
    return keep


def cdf_intervals(z, keep):
    """(a, b) fp64 [V]: token j of the kept set is drawn for u in [a_j, b_j); NaN outside the kept set."""
    zd = np.asarray(z, np.float64)
    w = np.where(keep, np.exp(np.where(keep, zd, 0.0) - zd[keep].max()), 0.0)
    c = np.cumsum(w)
    a, b = (c - w) / c[-1], c / c[-1]
    a[~keep], b[~keep] = np.nan, np.nan
    return a, b


def bound(V):
    """The CDF tolerance of the GPU tests: an fp32 sum with at least 256 lanes per row plus exp at 2 ulp."""
    return (-(-V // 256) + 16) * 2.0 ** -24


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------
VOCABS = (1000, 1001, 4099, 70000, 128256)
# (temperature, top_k, m = tokens top-p is to keep (0: top-p off), min_p)
SETTINGS = ((1.0, 0, 1, 0.0), (1.0, 0, 2, 0.0), (0.7, 0, 17, 0.0), (1.5, 50, 30, 0.0), (1.0, 0, 100, 0.0), (1.0, 0, 0, 0.1),
            (1.5, 20, 0, 0.05), (0.8, 64, 40, 0.02))
MARGIN = 1e-4
# a case whose margins fail with its first seed takes the next one listed here (tests/test_sampler_ref_host.py)
SEED_OF = {(1000, 4): 4008, (1000, 7): 7007, (1001, 2): 2006, (1001, 4): 4008, (1001, 7): 7007, (4099, 7): 7112}


@functools.lru_cache(maxsize=None)
def case(V, si):
    """dict(x fp32 [V] logits = 4 randn, T, top_k, top_p (fp32), min_p, z, keep, margins) of vocabulary V and SETTINGS[si]."""
    T, k, m, min_p = SETTINGS[si]
    seed = SEED_OF.get((V, si), 1000 * si + V % 997)
    return build((4.0 * np.random.RandomState(seed).standard_normal(V)).astype(np.float32), T, k, m, min_p)


def build(x, T, k, m, min_p):
    """The case of logits x: top_p set halfway between the masses that keep m and m + 1 tokens, and the margins of every boundary."""
    V = x.shape[0]
    z = scaled(x, T)
    zd = np.sort(z.astype(np.float64))[::-1]
    margins = {}
    if 0 < k < V:
        margins["top_k_gap"] = zd[k - 1] - zd[k]
        zd = zd[:k]
    top_p = 1.0
    if m:
        p = np.exp(zd - zd[0])
        p /= p.sum()
        above = np.concatenate([[0.0], np.cumsum(p)])             # above[j]: mass strictly above the j-th most likely survivor
        top_p = 0.5 * (above[m - 1] + above[m])                    # the j-th stays iff top_p > above[j]: exactly m stay
        margins["top_p_half_gap"] = 0.5 * p[m - 1]
        zd = zd[:m]
    if min_p:
        t = zd[0] + np.log(min_p)
        margins["min_p_gap"] = np.abs(z.astype(np.float64) - t).min()
    top_p = np.float32(top_p)
    keep = kept_set(z, k, top_p, min_p)
    for a in (x, z, keep):
        a.setflags(write=False)
    return dict(V=V, x=x, T=T, top_k=k, top_p=float(top_p), min_p=min_p, z=z, keep=keep, m=m, margins=margins)


CASES = [(V, si) for V in VOCABS for si in range(len(SETTINGS))]
# everything disabled at vocabularies below one wave / one workgroup
TINY = (1, 7, 64)


@functools.lru_cache(maxsize=None)
def tiny_case(V):
    x = (4.0 * np.random.RandomState(77 + V).standard_normal(V)).astype(np.float32)
    z = scaled(x, 1.0)
    keep = kept_set(z)
    for a in (x, z, keep):
        a.setflags(write=False)
    return dict(V=V, x=x, T=1.0, top_k=0, top_p=1.0, min_p=0.0, z=z, keep=keep, m=0, margins={})


# 70,000 logits whose scaled values all lie in [16, 32): ONE first radix digit for the whole row, more entries than the kernel
# gathers into LDS (16,384), so digits 2-4 of its selections walk the row instead. Three tokens hold most of the mass.
CROWDED = ((0, 2), (3, 2), (3, 0))       # (top_k, m)


@functools.lru_cache(maxsize=None)
def crowded_case(k, m):
    x = (1.0 + 0.25 * np.random.RandomState(5).random_sample(70000)).astype(np.float32)
    x[[11, 40000, 69999]] = [1.95, 1.99, 1.9]
    return build(x, 0.0625, k, m, 0.0)
