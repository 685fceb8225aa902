"""The comparison the depression-inventory suites share (tests/test_gpu_depressions.py, tests/test_gpu_depressions_large.py,
tests/test_large_depression_fields.py)."""
import numpy as np


def same(res, want, stats=None):
    """{'label', 'table'} of calc_depressions against (label, table, quanta): the label raster and every column with array_equal, the
    fixed-point sums and what is formed from them as bytes, the quanta of `stats`"""
    label, table, quanta = want
    assert res['label'].dtype == np.int32 and np.array_equal(res['label'], label)
    assert res['table'].dtype == table.dtype and len(res['table']) == len(table)
    for col in table.dtype.names:
        assert np.array_equal(res['table'][col], table[col]), col
    for col in ('area', 'volume', 'spill_elev', 'max_depth', 'mean_depth'):
        assert res['table'][col].tobytes() == table[col].tobytes(), col
    if stats is not None:
        assert stats['quanta'] == quanta
