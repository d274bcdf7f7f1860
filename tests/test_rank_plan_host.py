"""No GPU: utils._rank_plan, the one place that decides which X @ A^T / dY @ B launches form the rank terms of a block, against a
table written by hand from the three functions that each held a part of that decision before it (lora_xa: pad to 8, chunks of
192, streaming kernel for <= 64 columns of an input >= 8 wide; _xa_and_rank_block: <= 64 columns in one uamd_lora_xa2k launch,
65 .. 192 in greedy groups of whole factors with the last launch zero-filling, else first-version kernel + padded cast;
lora_dx_terms: one launch per adapter, a shared block only for Ps that share a buffer -- or a single one -- of <= 192 columns
and ranks <= 64). tests/test_gpu_lora_block_routes.py holds every case to the SET of entry points it reaches; this pins the
launch lists: entry point, factors read, first rank column, rank columns, rank-block columns written."""
import pytest

from unsloth_amd.kernels import utils as U

XA, XA2, XA2K = "uamd_lora_xa", "uamd_lora_xa2", "uamd_lora_xa2k"
K = 256


def _launches(plan):
    return [tuple(l) for l in plan.launches]


# ranks sharing one input: (padded widths, launches without a rank block, with one: (launches, block columns) or None = the
# launches without it + a padded cast, rank-block columns of that cast / of the cast the first-version route always needs)
FORWARD = {
    (16, 16, 16): ((16, 16, 16), [(XA2, (0, 1, 2), 0, 48, None)], ([(XA2K, (0, 1, 2), 0, 48, 64)], 64), 64),
    (4, 4, 4): ((8, 8, 8), [(XA2, (0, 1, 2), 0, 24, None)], ([(XA2K, (0, 1, 2), 0, 24, 64)], 64), 64),
    (12, 12, 12): ((16, 16, 16), [(XA2, (0, 1, 2), 0, 48, None)], ([(XA2K, (0, 1, 2), 0, 48, 64)], 64), 64),
    (16, 8, 4): ((16, 8, 8), [(XA2, (0, 1, 2), 0, 32, None)], ([(XA2K, (0, 1, 2), 0, 32, 64)], 64), 64),
    (32, 32, 32): ((32, 32, 32), [(XA, (0, 1, 2), 0, 96, None)],
                   ([(XA2K, (0, 1), 0, 64, 64), (XA2K, (2,), 64, 32, 64)], 128), 128),
    (64, 64): ((64, 64), [(XA, (0, 1), 0, 128, None)], ([(XA2K, (0,), 0, 64, 64), (XA2K, (1,), 64, 64, 64)], 128), 128),
    (64, 64, 64): ((64, 64, 64), [(XA, (0, 1, 2), 0, 192, None)],
                   ([(XA2K, (0,), 0, 64, 64), (XA2K, (1,), 64, 64, 64), (XA2K, (2,), 128, 64, 64)], 192), 192),
    (128, 128): ((128, 128), [(XA, (0, 1), 0, 192, None), (XA2, (0, 1), 192, 64, None)], None, 256),
    (128, 128, 128): ((128, 128, 128), [(XA, (0, 1, 2), 0, 192, None), (XA, (0, 1, 2), 192, 192, None)], None, 384),
    (64,): ((64,), [(XA2, (0,), 0, 64, None)], ([(XA2K, (0,), 0, 64, 64)], 64), 64),
    (128,): ((128,), [(XA, (0,), 0, 128, None)], None, 128),
}


@pytest.mark.parametrize("ranks", list(FORWARD))
@pytest.mark.parametrize("want_k", [False, True])
def test_forward_plan_with_the_streaming_kernel(ranks, want_k):
    widths, plain, blocked, cast = FORWARD[ranks]
    plan = U._rank_plan(ranks, K, want_k, v2=True)
    assert plan.widths == widths and plan.shared and plan.total == sum(widths)
    assert plan.starts == tuple(sum(widths[:i]) for i in range(len(widths)))
    if want_k and blocked is not None:
        assert (_launches(plan), plan.block, plan.casts) == (blocked[0], blocked[1], ())
    else:
        assert (_launches(plan), plan.block) == (plain, 0)
        assert plan.casts == (((tuple(range(len(ranks))), cast),) if want_k else ())


@pytest.mark.parametrize("ranks", list(FORWARD))
@pytest.mark.parametrize("want_k", [False, True])
@pytest.mark.parametrize("v2,k", [(False, K), (True, 4), (False, 4)])
def test_forward_plan_on_the_first_version_kernel(ranks, want_k, v2, k):
    """LORA_XA_V2 off, or an input of fewer than 8 columns: the same chunks, all on uamd_lora_xa, and never a rank block from the
    kernel -- a padded cast of the whole buffer when the GEMM wants one."""
    widths, plain, _, cast = FORWARD[ranks]
    plan = U._rank_plan(ranks, k, want_k, v2=v2)
    assert _launches(plan) == [(XA,) + l[1:] for l in plain] and plan.block == 0 and plan.widths == widths
    assert plan.casts == (((tuple(range(len(ranks))), cast),) if want_k else ())


# one input per factor: (ranks, rank block wanted) -> (P in one buffer, launches, block columns, casts)
BACKWARD = {
    # shared P and shared block: every launch its own columns, the last one zero-fills
    ((16, 16, 16), True): (True, [(XA2K, (0,), 0, 16, 16), (XA2K, (1,), 16, 16, 16), (XA2K, (2,), 32, 16, 32)], 64, ()),
    ((64, 64, 64), True): (True, [(XA2K, (0,), 0, 64, 64), (XA2K, (1,), 64, 64, 64), (XA2K, (2,), 128, 64, 64)], 192, ()),
    ((32, 32, 32), True): (True, [(XA2K, (0,), 0, 32, 32), (XA2K, (1,), 32, 32, 32), (XA2K, (2,), 64, 32, 64)], 128, ()),
    # one adapter: a block of its own from the kernel, odd rank included
    ((4,), True): (False, [(XA2K, (0,), 0, 8, 64)], 64, ()),
    ((16, None, None), True): (False, [(XA2K, (0,), 0, 16, 64)], 64, ()),
    # own padded block per term: odd ranks, a missing adapter, r = 128
    ((4, 4, 4), True): (False, [(XA2, (0,), 0, 8, None), (XA2, (1,), 8, 8, None), (XA2, (2,), 16, 8, None)], 0,
                        (((0,), 64), ((1,), 64), ((2,), 64))),
    ((16, 8, 4), True): (False, [(XA2, (0,), 0, 16, None), (XA2, (1,), 16, 8, None), (XA2, (2,), 24, 8, None)], 0,
                         (((0,), 64), ((1,), 64), ((2,), 64))),
    ((16, None, 16), True): (False, [(XA2, (0,), 0, 16, None), (XA2, (2,), 16, 16, None)], 0, (((0,), 64), ((2,), 64))),
    ((128,), True): (False, [(XA, (0,), 0, 128, None)], 0, (((0,), 128),)),
    ((128, 128, 128), True): (True, [(XA, (0,), 0, 128, None), (XA, (1,), 128, 128, None), (XA, (2,), 256, 128, None)], 0,
                              (((0,), 128), ((1,), 128), ((2,), 128))),
    # no block
    ((16, 16, 16), False): (True, [(XA2, (0,), 0, 16, None), (XA2, (1,), 16, 16, None), (XA2, (2,), 32, 16, None)], 0, ()),
    ((16, 8, 4), False): (False, [(XA2, (0,), 0, 16, None), (XA2, (1,), 16, 8, None), (XA2, (2,), 24, 8, None)], 0, ()),
    ((128, 128), False): (True, [(XA, (0,), 0, 128, None), (XA, (1,), 128, 128, None)], 0, ()),
    ((256,), False): (False, [(XA, (0,), 0, 192, None), (XA2, (0,), 192, 64, None)], 0, ()),
    ((None, None, None), False): (False, [], 0, ()),
    ((None, None, None), True): (False, [], 0, ()),
}


@pytest.mark.parametrize("ranks,want_k", list(BACKWARD))
def test_backward_plan(ranks, want_k):
    shared, launches, block, casts = BACKWARD[(ranks, want_k)]
    plan = U._rank_plan(ranks, (K, 128, 128)[:len(ranks)], want_k, one_input=False, v2=True)
    assert (plan.shared, _launches(plan), plan.block, plan.casts) == (shared, launches, block, casts)
    assert plan.widths == tuple(None if r is None else (r + 7) // 8 * 8 for r in ranks)


def test_backward_plan_on_the_first_version_kernel():
    """LORA_XA_V2 off (lora_dx_terms then never asks for a block) or a dY of fewer than 8 columns: uamd_lora_xa."""
    plan = U._rank_plan((16, 16, 16), (K, 128, 128), False, one_input=False, v2=False)
    assert _launches(plan) == [(XA, (0,), 0, 16, None), (XA, (1,), 16, 16, None), (XA, (2,), 32, 16, None)]
    plan = U._rank_plan((16, 16), (K, 4), False, one_input=False, v2=True)
    assert _launches(plan) == [(XA2, (0,), 0, 16, None), (XA, (1,), 16, 16, None)]


def test_the_fused_activations_and_the_plan_share_their_rank_predicates():
    assert [r for r in (0, 4, 8, 12, 16, 64, 72, 128) if U._streams(r)] == [8, 16, 64]
    assert U._share_block((4, 4, 4)) and U._share_block((64, 64, 64)) and U._share_block((60,))
    assert not U._share_block((64, 64, 64, 8)) and not U._share_block((128,)) and not U._share_block((60, 12))
