"""CPU: the NumPy restatement of the 0.01-grid median (tests/grid_restatement.py) equals the oracle's partition_stat_tp on every
array tests/test_grid_quantiles.py hands the device -- the selections and the deviations each MAD takes its median of.  The
oracle is pinned to the reference by tests/test_oracle_vs_ref.py; the device is held to the restatement with ==."""
import numpy as np
import pytest

import grid_cases
import grid_restatement as gr


@pytest.mark.parametrize("group", sorted(grid_cases.finite_groups()))
def test_restatement_equals_oracle(oracle_cls, group):
    O = oracle_cls()
    n = 0
    for case in grid_cases.finite_groups()[group]():
        for arr in case.oracle_arrays():
            got, cnt = gr.median(arr)
            exp = O.median(arr)
            assert cnt == arr.size
            assert got == exp, f"{case.name} (n={arr.size}): restatement {got!r} != oracle {exp!r}"
            n += 1
    assert n > 0


def test_restatement_edges():
    assert gr.median(np.zeros(0, np.float32)) == (0.0, 0)
    with pytest.raises(ValueError):
        gr.median(np.array([1.0, np.nan], np.float32))
    # the crossing is the first bucket whose running count reaches n // 2 (>=): 5 of 10 values in the first bucket
    assert gr.median(np.array([3.0] * 5 + [3.07] * 5, np.float32))[0] == float(np.float32(3.0))
    # below the grid step: the index-order mean
    x = np.array([2.0, 2.004, 2.009], np.float32)
    assert gr.median(x)[0] == ((float(x[0]) + float(x[1])) + float(x[2])) / 3
    # the MAD's deviations are rounded to float
    assert gr.abs_dev(np.array([1.0], np.float32), 0.1).dtype == np.float32
    assert gr.abs_dev(np.array([1.0], np.float32), 0.1)[0] == np.float32(0.9)


def test_case_builders_hit_their_targets():
    """The inputs are what their names say (the GPU test asserts which form ran on them)."""
    below, above = grid_cases.wide_edges()
    assert gr.span([0.0, below])[2] == gr.CAP and gr.span([0.0, above])[2] == gr.CAP + 1
    for case in grid_cases.counter_widths():
        arr = case.x if case.x is not None else case.xi
        assert arr.size in (grid_cases.PACK16_LAST, grid_cases.PACK16_LAST + 1, grid_cases.PACK16_OLD_LAST, grid_cases.PACK16_OLD_LAST + 1)
    for case in grid_cases.lds_window():
        s = gr.selected(case.x, case.mask)
        assert gr.span(s)[2] > grid_cases.KLDSBINS, case.name
    deg = grid_cases.degenerate()
    assert all(gr.span(gr.selected(c.x, c.mask))[2] is None for c in deg)
