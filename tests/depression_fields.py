"""Designed surfaces for the depression inventory (tests/test_depressions_ref.py, tests/test_depressions_api.py,
tests/test_gpu_depressions.py): small builders, each returning a float64 elevation, and the spacing of the one tile whose cell
area varies by row."""
import numpy as np

import fill_fields as F


def checkerboard():
    """(64, 64): a tilted plane with a one-cell pit at every odd (row, col) of the interior, 1 to 5 below the plane (the lowest
    neighbour of a cell is 0.8 below it): 31 * 31 single-cell depressions, none touching another."""
    z = F.plane(64, 64)
    for r in range(1, 63, 2):
        for c in range(1, 63, 2):
            z[r, c] -= 1.0 + (7 * r + 3 * c) % 5
    return z


def diagonal_chain_cells():
    """the chain's cells: one per row, the column moving by one each row -- neighbours in the chain touch by a corner only.  It
    runs down the main diagonal through the corner where the blocks (0,0) (0,1) (1,0) (1,1) meet, turns, crosses the column seam
    32/31 again, turns, and crosses the row seam 63/64."""
    cells = []
    c = 10
    for r in range(10, 86):
        cells.append((r, c))
        c += 1 if (r < 40 or r >= 60) else -1
    return cells


def diagonal_chain():
    """(96, 96): a plateau at 100 with single cells at 48..50 that touch only by corners: ONE depression under 8-connectivity, 76
    under 4-connectivity.  Its only sill is (9, 10) at 60, above the chain's first cell, with a channel down to the border: every
    cell of the chain rises to 60."""
    z = np.full((96, 96), 100.0)
    for k, (r, c) in enumerate(diagonal_chain_cells()):
        z[r, c] = 50.0 - k % 3
    for r in range(10):
        z[r, 10] = 51.0 + r                     # (9, 10) = 60, the sill; 51 at the border
    return z


def ring_lake():
    """(70, 70): a plateau at 100, a ring lake (bed 80) around an island at 110 that has a lake of its own (bed 90): two
    depressions with the levels 100 and 110, the inner one inside the other's bounding box."""
    z = np.full((70, 70), 100.0)
    r, c = np.mgrid[0:70, 0:70]
    d = np.hypot(r - 35, c - 34)
    z[d <= 24] = 80.0
    z[d <= 12] = 110.0
    z[d <= 5] = 90.0 + d[d <= 5]
    return z


def comb():
    """(96, 96): a plateau at 100 with a lake made of a spine along row 70 and teeth rising from it to row 5 in every fourth
    column: the teeth enter the upper blocks from below, so inside such a block they are separate pieces -- one depression with
    several block-local roots per block."""
    z = np.full((96, 96), 100.0)
    r = np.arange(96)
    z[70, 5:91] = 50.0
    for c in range(6, 90, 4):
        z[5:70, c] = 50.0 + 0.1 * r[5:70]
    return z


def two_levels():
    """(40, 70): two lakes with the bed at 50, separated by a one-cell dam (column 30, 100).  The left one spills at 80 through
    (20, 9), the right one at 90 through (20, 51); each sill has a channel down to the border."""
    z = np.full((40, 70), 100.0)
    z[10:30, 10:30] = 50.0
    z[10:30, 31:51] = 50.0
    z[20, 0:10] = 71.0 + np.arange(10)          # (20, 9) = 80
    z[20, 51:70] = 90.0 - np.arange(19)         # (20, 51) = 90
    return z


def lake_nan_hole():
    """(40, 40): a lake (bed 50) in a plateau at 100 around a no-data hole whose rim lies at 70: the rim cells are open, the lake
    rises to them and spills into the hole -- every sill is an open cell."""
    z = np.full((40, 40), 100.0)
    z[10:31, 10:31] = 50.0
    z[18:23, 18:23] = 70.0
    z[19:22, 19:22] = np.nan
    return z


VARYING_SHAPE = (50, 45)


def varying_spacing():
    """a cone lake on a tilted plane; the tile's dX (and with it the cell area) varies by row: varying_spacing_kwargs()"""
    n, m = VARYING_SHAPE
    z = F.plane(n, m, 300.0, 0.25, 0.125)
    r, c = np.mgrid[0:n, 0:m]
    d = np.hypot(r - 24, c - 20)
    z[d <= 15] = 250.0 + 2.0 * d[d <= 15]
    return z


def varying_spacing_kwargs():
    """dX, dY, dX2, dY2 of the varying_spacing tile (dX per fence row, dX2 per cell row, as DEMProcessor takes them)"""
    n = VARYING_SHAPE[0]
    dX2 = 30.0 * np.cos(np.deg2rad(40.0 + 0.3 * np.arange(n)))
    return dict(dX=0.5 * (dX2[:-1] + dX2[1:]), dY=np.full(n - 1, 30.0), dX2=dX2, dY2=np.full(n, 30.0))


LIMITS_SHALLOW_BOTTOM = (32, 25)
LIMITS_DEEP_BOTTOM = (32, 70)
LIMITS_PIT = (32, 80)


def limits():
    """(64, 100): a plateau at 100 with a cone 10 deep (bottom 90 at (32, 25)) and a cone 40 deep (bottom 60 at (32, 70), slope 2
    per cell); inside the deep one, 10 cells from its bottom, a pit at 75 whose lowest neighbour lies at 78: 3 deep once the
    deep cone drains."""
    z = np.full((64, 100), 100.0)
    r, c = np.mgrid[0:64, 0:100]
    d = np.hypot(r - 32, c - 25)
    z[d <= 12] = 90.0 + 10.0 * d[d <= 12] / 12.0
    d = np.hypot(r - 32, c - 70)
    z[d <= 20] = 60.0 + 2.0 * d[d <= 20]
    z[LIMITS_PIT] = 75.0
    return z


def builders():
    """name -> builder of every field above"""
    return {'checkerboard': checkerboard, 'diagonal_chain': diagonal_chain, 'ring_lake': ring_lake, 'comb': comb,
            'two_levels': two_levels, 'lake_nan_hole': lake_nan_hole, 'varying_spacing': varying_spacing, 'limits': limits}


def spacing_kwargs(name):
    """the DEMProcessor spacing keywords of a field"""
    return varying_spacing_kwargs() if name == 'varying_spacing' else dict(dX=30.0, dY=30.0)


def row_area(name, n):
    """dX2 * dY2 per row of a field under spacing_kwargs(name)"""
    if name == 'varying_spacing':
        kw = varying_spacing_kwargs()
        return kw['dX2'] * kw['dY2']
    return np.ones(n) * 30.0 * (np.ones(n) * 30.0)
