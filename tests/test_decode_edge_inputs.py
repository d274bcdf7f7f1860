"""Host checks of the decode key-range inputs (tests/_decode_edges.py; the GPU side is tests/test_gpu_decode_edges.py).

The GPU tests hold the decode attention to `row_err <= 4 x model_err` against an fp64 reference over keys [first, len). That bound
means something only if a range that is off by one key at either end moves the output by far more than it. Here, on the very
inputs the GPU tests use and in fp64: the edge key of every role-0 / role-1 row holds at least half of the row's softmax mass, every
off-by-one range moves the rows of the role that watches that edge by row_err >= 0.5, and 0.5 lies more than 20 x above the GPU
bound. These are conditions on the INPUTS -- a case that misses one gets another seed or other lengths, never another number."""
import math

import pytest
import torch

from tests import _decode_edges as E

BOUND_FACTOR = E.BOUND_FACTOR
assert BOUND_FACTOR == 4
MIN_EDGE_MASS = 0.5         # of a role-0 / role-1 row, on its edge key
MIN_SHIFT = 0.5             # row_err by which an off-by-one range moves the rows that watch the moved edge
# which roles watch which moved edge (role 3, the diffuse control, is not asked to notice anything)
WATCHERS = {"first-1": (0, 2), "first+1": (0,), "len+1": (1, 2), "len-1": (1,)}

CASE_DTYPE = [(n, d) for n in E.CASES for d in E.DTYPES]


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_the_edge_key_holds_at_least_half_of_the_mass(name, dtype_name):
    c = E.build_case(name, dtype_name)
    mass = E.edge_mass(c["q"], c["kc"], c["lens"], c["window"], c["scale"], c["Hq"], c["Hk"])
    assert len(mass) == c["B"] * (len(E.role_heads(c["Hq"], 0)) + len(E.role_heads(c["Hq"], 1)))
    print(name, dtype_name, "least edge mass", round(min(mass.values()), 4))
    assert min(mass.values()) >= MIN_EDGE_MASS, min(mass.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_every_off_by_one_range_moves_the_rows_that_watch_it(name, dtype_name):
    c = E.build_case(name, dtype_name)
    assert torch.isfinite(c["ref"]).all()
    # the distance between "right" and "off by one", explicit: the GPU bound is below 1 / 20 of the least shift asked for
    assert MIN_SHIFT > 20 * BOUND_FACTOR * c["model_err"], c["model_err"]
    seen = {}
    for b, (first, L) in enumerate(c["ranges"]):
        muts = E.mutants(first, L, E.S_MAX)
        # (first = 0 has no key before it, len = S_MAX no slot after it, a single key leaves nothing to pull in)
        assert [m[0] for m in muts] == [n for n in ("first-1", "first+1", "len+1", "len-1")
                                        if not (n == "first-1" and first == 0) and not (n == "len+1" and L == E.S_MAX)
                                        and not (n in ("first+1", "len-1") and L - first == 1)]
        for mname, f, e in muts:
            ranges = list(c["ranges"])
            ranges[b] = (f, e)
            other = E.ref64_ranges(c["q"], c["kc"], c["vc"], ranges, c["scale"], c["Hq"], c["Hk"])
            for role in WATCHERS[mname]:
                seen[(b, mname, role)] = E.shift_of_rows(other, c["ref"], b, E.role_heads(c["Hq"], role))
    assert seen
    print(name, dtype_name, "model_err %.3e" % c["model_err"], {k: round(v, 3) for k, v in seen.items()})
    for key, shift in seen.items():
        assert shift >= MIN_SHIFT, (key, shift)


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_the_rounding_model_is_the_reference_of_the_true_range(name, dtype_name):
    """model_err is the error of the reference rounded once. Where slot `len` exists, the role-1 rows of that rounded reference lie
    within model_err of their own range's fp64 value and at least MIN_SHIFT from that of the range with one more key: the yardstick
    was not taken from a wider range by mistake."""
    c = E.build_case(name, dtype_name)
    heads = E.role_heads(c["Hq"], 1)
    rows = [b for b, L in enumerate(c["lens"]) if L < E.S_MAX]            # (the full cache has no slot `len`)
    wider = E.ref64_ranges(c["q"], c["kc"], c["vc"], [(f, min(L + 1, E.S_MAX)) for f, L in c["ranges"]], c["scale"],
                           c["Hq"], c["Hk"])
    for b in rows:
        assert E.shift_of_rows(c["model"], c["ref"], b, heads) <= c["model_err"]
        assert E.shift_of_rows(c["model"], wider, b, heads) >= MIN_SHIFT
    if all(L - f == 1 for f, L in c["ranges"]):
        assert c["model_err"] == 0.0                                      # one key: the output is that v row, exactly


def test_ref64_on_a_hand_written_three_key_example():
    """D = 2, one head, scale 1, q = (ln 2, 0): keys (1, 0), (2, 0), (0, 5) score ln 2, 2 ln 2, 0, so exp gives 2, 4, 1.
    All three: weights 2/7, 4/7, 1/7. Window 2 (keys 1 .. 2): 4/5, 1/5. Two keys, no window (keys 0 .. 1): 1/3, 2/3."""
    q = torch.tensor([[math.log(2.0), 0.0]], dtype=torch.float64)
    kc = torch.tensor([[[[1.0, 0.0], [2.0, 0.0], [0.0, 5.0], [9.0, 9.0]]]], dtype=torch.float64)
    vc = torch.tensor([[[[7.0, 0.0], [0.0, 7.0], [14.0, 14.0], [1e6, 1e6]]]], dtype=torch.float64)
    got = E.ref64(q, kc, vc, (3,), 0, 1.0, 1, 1)
    assert got.shape == (1, 1, 2)
    torch.testing.assert_close(got[0, 0], torch.tensor([4.0, 6.0], dtype=torch.float64), rtol=1e-14, atol=0)
    got = E.ref64(q, kc, vc, (3,), 2, 1.0, 1, 1)
    torch.testing.assert_close(got[0, 0], torch.tensor([2.8, 8.4], dtype=torch.float64), rtol=1e-14, atol=0)
    got = E.ref64(q, kc, vc, (2,), 0, 1.0, 1, 1)
    torch.testing.assert_close(got[0, 0], torch.tensor([7.0 / 3, 14.0 / 3], dtype=torch.float64), rtol=1e-14, atol=0)
    got = E.ref64(q, kc, vc, (3,), 3, 1.0, 1, 1)                          # len > window is false: every key
    torch.testing.assert_close(got[0, 0], torch.tensor([4.0, 6.0], dtype=torch.float64), rtol=1e-14, atol=0)
    got = E.ref64(q, kc, vc, (3,), 1, 1.0, 1, 1)                          # the new key alone
    assert got[0, 0].tolist() == [14.0, 14.0]


def test_key_range_and_mutants_on_hand_written_ranges():
    assert E.key_range(300, 96) == (204, 300) and E.key_range(20, 96) == (0, 20) and E.key_range(200, 200) == (0, 200)
    assert E.key_range(200, 199) == (1, 200) and E.key_range(7, 0) == (0, 7) and E.key_range(1, 1) == (0, 1)
    assert E.mutants(5, 9, 16) == [("first-1", 4, 9), ("first+1", 6, 9), ("len+1", 5, 10), ("len-1", 5, 8)]
    assert E.mutants(0, 9, 16) == [("first+1", 1, 9), ("len+1", 0, 10), ("len-1", 0, 8)]           # no key before 0
    assert E.mutants(5, 16, 16) == [("first-1", 4, 16), ("first+1", 6, 16), ("len-1", 5, 15)]      # no slot after the last
    assert E.mutants(8, 9, 16) == [("first-1", 7, 9), ("len+1", 8, 10)]                            # one key: nothing to pull in
    assert E.mutants(0, 1, 1) == []


def test_the_table_sits_on_the_edges_it_names():
    """The geometry the comments of CASES claim, from the numbers alone."""
    firsts = {n: [E.key_range(L, c[4])[0] for L in c[5]] for n, c in E.CASES.items()}
    assert firsts["d128_win96"] == [204, 0] and firsts["d128_win129_g7"] == [128] and firsts["d128_win130"] == [127]
    assert firsts["d128_win128"] == [129] and firsts["d128_win200_len200"] == [0] and firsts["d128_win199_len200"] == [1]
    assert firsts["d128_win16_len400"] == [384] and firsts["d128_win2_len385"] == [383] and firsts["d128_split256"] == [300]
    assert firsts["d64_win100_first31_33"] == [31, 32, 33] and firsts["d64_win130_first127_129"] == [127, 128, 129]
    assert firsts["d64_win16_len400"] == [384]
    groups = {(c[0], c[1] // c[2]) for c in E.CASES.values()}
    assert {(128, 1), (128, 2), (128, 4), (128, 7), (64, 1), (64, 2), (64, 4), (64, 7)} <= groups
    blocks = {n: (E.S_MAX // c[3]) * c[2] * len(c[5]) for n, c in E.CASES.items()}
    over = sorted(n for n, k in blocks.items() if k > 256)               # the launches too large for the granule combine
    assert over == ["d128_split16_counter", "d64_split32_counter"] and blocks["d64_split32_granules"] == 256
    for n, c in E.CASES.items():
        assert c[3] % (2048 // c[0]) == 0 and len(c[5]) <= 3 and c[2] <= 8, n
