"""row16_argmax (csrc/lane_ops.hpp) in two forms: the four-step (value, index) exchange and row-maximum-then-lowest-index on the
bit patterns.  Both are restated lane by lane in tests/row16_argmax_forms.py and must agree, on every lane, with each other and
with the first index of the maximum, over the sampler's domain: ratios >= +0 inside a head's window, -inf outside it."""
import itertools

import numpy as np
import pytest

from row16_argmax_forms import PARTNERS, bits, exchange_argmax, max_then_lowest_index

NINF = float('-inf')
# ties are the point: few distinct values, so that most rows hold their maximum several times
VALUES = [0.0, 0.0, 1e-30, 0.25, 0.5, 0.5, 3.0, 3.0, 3.0, float('inf')]
WINDOWS = [(start, sz) for start in range(15) for sz in range(1, 16 - start)]    # every [start, start + sz) of a packed head


def _rows_for(start, sz, rng):
    inside = range(start, start + sz)
    rows = [[0.0] * sz, [3.0] * sz, [float('inf')] * sz,                 # every real ratio 0 / all lanes tie / all infinite
            [0.0] * (sz - 1) + [0.5], [0.5] + [0.0] * (sz - 1),          # the winner in the last / first real lane
            [0.0] * (sz - 1) + [1e-45]]                                  # a denormal beats 0
    rows += [[VALUES[k] for k in rng.randint(0, len(VALUES), sz)] for _ in range(24)]
    for r in rows:
        lanes = [NINF] * 16
        for lane, v in zip(inside, r):
            lanes[lane] = v
        yield lanes


def test_partner_tables_are_involutions_that_reach_the_whole_row():
    for p in PARTNERS:
        assert sorted(p) == list(range(16)) and all(p[p[i]] == i for i in range(16))
    reach = [{i} for i in range(16)]
    for p in PARTNERS:
        reach = [reach[i] | reach[p[i]] for i in range(16)]
    assert all(r == set(range(16)) for r in reach)


def test_integer_order_equals_float_order_on_the_domain():
    dom = [NINF, 0.0, 1e-45, 1e-30, 0.25, 0.5, 1.0, 3.0, 3.4e38, float('inf')]
    for x, y in itertools.product(dom, dom):
        assert (np.float32(x) < np.float32(y)) == (bits(x) < bits(y))
        assert (np.float32(x) == np.float32(y)) == (bits(x) == bits(y))


@pytest.mark.parametrize('start', range(15))
def test_both_forms_agree_on_every_lane_for_every_window(start):
    rng = np.random.RandomState(start)
    for sz in range(1, 16 - start):
        for lanes in _rows_for(start, sz, rng):
            top = max(lanes)
            want = lanes.index(top)                                      # first index of the maximum
            assert start <= want < start + sz                            # a lane outside the window never wins
            b_old, i_old = exchange_argmax(lanes)
            b_new, i_new = max_then_lowest_index(lanes)
            assert i_old == [want] * 16 and i_new == [want] * 16, (start, sz, lanes)
            assert [bits(b) for b in b_old] == [bits(top)] * 16 and [bits(b) for b in b_new] == [bits(top)] * 16


def test_a_row_of_minus_infinity_only_names_lane_0_in_both_forms():
    lanes = [NINF] * 16
    assert exchange_argmax(lanes)[1] == [0] * 16 and max_then_lowest_index(lanes)[1] == [0] * 16


def test_window_list_is_every_packed_head():
    assert len(WINDOWS) == 120 and all(s + z <= 15 for s, z in WINDOWS)
