"""sgo_hypotheses_chunk (include/sgo.h): how many hypotheses of sgo_optimize_gn_hypotheses share one launch chain on a multifrontal
context, as a pure function -- no context, no GPU -- against a restatement over a grid of (bytes per hypothesis, budget, B)."""
import itertools

from sparse_gslam_amd import capi


def chunk(per, budget, B):
    """min(B, budget / per, 65535); 0 -- the sequential route -- below 2 or without a batched route (per <= 0)"""
    k = min(B, budget // per, 65535) if per > 0 else 0
    return k if k >= 2 else 0


PER = (0, -4096, 1, 255, 4096, 37 * 2 ** 20 + 512, 2 ** 30, 2 ** 40)
BUDGET = (0, 1, 4095, 4096, 8191, 8192, 3 * 4096, 2 ** 20, 65535 * 4096, 65536 * 4096 + 5, 2 ** 33, 2 ** 62)
COUNT = (0, 1, 2, 3, 7, 64, 256, 65535, 65536, 2 ** 31 - 1)


def test_chunk_matches_the_restatement_over_the_grid():
    seen = set()
    for per, budget, B in itertools.product(PER, BUDGET, COUNT):
        want = chunk(per, budget, B)
        assert capi.hypotheses_chunk(per, budget, B) == want, (per, budget, B)
        seen.add(want)
    assert {0, 2, 3, 7, 64, 256, 65535} <= seen


def test_the_named_cases():
    assert capi.hypotheses_chunk(0, 2 ** 40, 64) == 0                 # no batched route
    assert capi.hypotheses_chunk(4096, 8191, 64) == 0                 # budget < 2 per
    assert capi.hypotheses_chunk(4096, 8192, 64) == 2
    assert capi.hypotheses_chunk(4096, 2 ** 40, 1) == 0               # one hypothesis shares nothing
    assert capi.hypotheses_chunk(1, 2 ** 40, 2 ** 31 - 1) == 65535    # a grid's y dimension
    assert capi.hypotheses_chunk(4096, 3 * 4096, 7) == 3              # chains of 3 + 3 + 1
    assert capi.hypotheses_chunk(4096, -1, 7) == 0 and capi.hypotheses_chunk(4096, 2 ** 40, -3) == 0
