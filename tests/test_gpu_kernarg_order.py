"""A swapped pair of same-typed pointers in a kernel's parameter list compiles.  The kernels of the solve take the pointers of
their prologue as plain leading parameters (so that they arrive preloaded in SGPRs), their launch wrappers
pass them by position: every group of those kernels is run here on a graph of a few thousand poses, and what optimize(4)
returns has to equal, bit for bit, what the commit before the reordering returned (tests/golden/kernarg_order.npz, written by
scripts/make_golden_kernarg_order.py).  Graph replay, plain launches and the profile mode launch through the same wrappers and
have to give the same bits as well."""
import os

import numpy as np
import pytest

import kernarg_order_cases as kc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernarg_order.npz")


@pytest.fixture(scope="module")
def gold():
    return kc.load(GOLD)


def test_the_fixture_covers_every_case(gold):
    assert set(gold) == set(kc.CASES)
    assert os.path.getsize(GOLD) <= 200 * 1024


@pytest.mark.parametrize("name", list(kc.CASES))
def test_optimize_returns_the_recorded_bits_in_every_execution_mode(name, gold):
    for mode, opts in kc.MODES:
        r = kc.run(name, opts)
        for k, v in r.items():
            want = gold[name][k]
            assert v.dtype == want.dtype and np.array_equal(v, want), (name, mode, k, np.abs(v - want).max())
