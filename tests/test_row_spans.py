"""CPU: kernels/utils._row_spans, the one place that splits the rows of a GEMM operand into launches that each span less
than GEMM_SPAN_LIMIT bytes (_launch_gemm: whole 256-row tiles; dense_dw: 64-token steps of the contraction)."""
import random

import pytest


def test_row_spans_tile_the_rows_below_the_span_limit():
    from unsloth_amd.kernels import utils as U
    rng = random.Random(20240611)
    seen = {"one": 0, "chunked": 0, "refused": 0}
    old = U.GEMM_SPAN_LIMIT
    try:
        for _ in range(400):
            align = rng.choice((64, 256))
            limit = (1 << rng.randint(12, 26)) + rng.choice((0, 0, rng.randint(-1000, 1000)))
            row_bytes = 2 * rng.randint(1, 1 << rng.randint(1, 14))
            M = rng.randint(1, 3 * (limit // row_bytes) + 300)
            U.GEMM_SPAN_LIMIT = limit
            if M * row_bytes < limit:
                assert U._row_spans(M, row_bytes, align) == [(0, M)]        # exactly one launch, whatever `align`
                seen["one"] += 1
                continue
            if align * row_bytes >= limit:                                  # not even one aligned chunk fits
                with pytest.raises(RuntimeError, match="span limit"):
                    U._row_spans(M, row_bytes, align)
                seen["refused"] += 1
                continue
            spans = U._row_spans(M, row_bytes, align)
            seen["chunked"] += 1
            assert len(spans) > 1
            nxt = 0
            for r0, rows in spans:                                          # in order, no gap, no overlap
                assert r0 == nxt and rows > 0
                assert rows * row_bytes < limit
                nxt = r0 + rows
            assert nxt == M
            assert all(rows % align == 0 for _, rows in spans[:-1])
    finally:
        U.GEMM_SPAN_LIMIT = old
    assert min(seen.values()) >= 20, seen                                   # the draws reach all three outcomes
