"""Grids and case tables of the positive-layer tests (TEST INFRASTRUCTURE): tests/test_positive_layer_cpu.py holds the
census of what they contain, tests/test_gpu_positive_layer.py runs the device on them.

MAIN is tests/layered_soundings.py's GRID_REPLAY (40 x 3000, seed 11, 8 % NaN temperatures): stacked stable, neutral and
steep layers, so that 11-17 % of the columns have two to five positive layers.  Every value is a multiple of 1/64: a
float32 grid holds exactly the float64 numbers, and one restatement serves both dtypes.  COMPOSE is a 20 x 333 grid of the
same generator for the compositions with the humidity pass, the ground cut and the maximum-CAPE parcel; the small grids are
there for their shapes."""
import functools

import numpy as np

from tests import layered_soundings as ls
from tests import positive_layer_restatement as R

MAIN = ls.GRID_REPLAY
COMPOSE = (20, 333, 37)       # K >= 2 in 38 / 25 / 29 columns (surface / most-unstable / mixed-layer parcel)
SMALL = {'1x65': (1, 65, 3), '2x64': (2, 64, 4), '40x1': (40, 1, 11)}             # (the one column has K = 2 for the surface and the mixed-layer parcel)
PARCELS = ls.PARCELS
CHOICES = R.CHOICES
ORACLE_MOIST = {'exact': 'rk4', 'table': 'table'}
# numpy_api's positive_layer= names and MetPy's pairs, with the bits of xp_opts.flags each sets
FLAGS = {'envelope': 0 << 4, 'lowest': 1 << 4, 'highest': 2 << 4, 'deepest': 3 << 4, 'most_cape': 4 << 4}
PAIRS = {('bottom', 'top'): 'envelope', ('bottom', 'bottom'): 'lowest', ('top', 'top'): 'highest', ('wide', 'wide'): 'deepest',
         ('most_cape', 'most_cape'): 'most_cape'}
BAD_PAIRS = (('top', 'bottom'), ('bottom', 'wide'), ('wide', 'top'), ('most_cape', 'top'), ('bottom', None), (None, 'top'),
             ('lowest', 'lowest'))


def grid(spec=MAIN, dtype=np.float64):
    """(p, T, Td) of a grid (nlev, ncol, seed); shared, read-only."""
    return ls.grid(*spec, dtype=dtype)


@functools.lru_cache(maxsize=None)
def restated(parcel, moist='exact', spec=MAIN):
    """The restatement of a grid for one parcel, computed once per process."""
    p, t, td = grid(spec)
    return R.grid(p, t, td, parcel=parcel, moist=ORACLE_MOIST[moist])


def census(g):
    """What a restated grid holds: columns by K, columns where each choice moves the CAPE off the default's, where the deepest
    layer is not the one with the most CAPE, and the rules the events exercise."""
    K = g['K']
    default = g['oracle']['cape']
    out = {'K>=2': int((K >= 2).sum()), 'K>=3': int((K >= 3).sum()), 'Kmax': int(K.max())}
    for ch in CHOICES:
        out[ch] = int((g[ch]['cape'] != default).sum())
    out['deepest!=most_cape'] = int((g['deepest']['picked'] != g['most_cape']['picked']).sum())
    first_down = up_while_open = open_top = 0
    for c in g['columns']:
        ev = [e['kind'] for e in c['events']]
        first_down += bool(ev) and ev[0] == 'down'
        is_open = False
        for kind in ev:
            if kind == 'up' and is_open:
                up_while_open += 1
                break
            is_open = kind == 'up'
        open_top += bool(c['layers']) and c['layers'][-1]['open']
    out.update(first_down=first_down, up_while_open=up_while_open, open_top=open_top)
    return out
