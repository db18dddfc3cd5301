"""The inputs of the hydrostatic tests, shared by the census on the CPU (tests/test_hydrostatic_cpu.py) and the device tests
(tests/test_gpu_hydrostatic.py): the grids, the specific humidity that goes with the dewpoint, the base heights, the layers and
hand-built columns."""
import numpy as np

from oracle import thermo as O
from tests import hydrostatic_restatement as R
from xarray_parcel_amd import synth

# (nlev, ncol, seed) of every grid the device tests run; 65 columns: one wavefront plus one lane; one and two levels
GRIDS = {'12x640': (12, 640, 12), '40x640': (40, 640, 40), '7x65': (7, 65, 1), '24x300': (24, 300, 4), '1x70': (1, 70, 7),
         '2x130': (2, 130, 2)}
NAN = float('nan')
# 1000-500 hPa, 850-500 hPa, the lowest 150 hPa by depth, the open whole column: (kind, bottom, top) and as the array API takes them
LAYERS = ((R.PRESSURE, 1000.0, 500.0), (R.PRESSURE, 850.0, 500.0), (R.PRESSURE_DEPTH, NAN, 150.0), (R.PRESSURE, NAN, NAN))
API_LAYERS = ({'bottom': 1000.0, 'top': 500.0}, ('pressure', 850.0, 500.0), {'depth': 150.0}, {'bottom': None, 'top': None})
LAYER_NAMES = ('1000-500', '850-500', 'lowest 150', 'whole column')


def specific_humidity(p, td):
    """q = w / (1 + w) of the dewpoint's mixing ratio: the same moisture in the other vocabulary (NaN wherever Td is)."""
    w = O.mixing_ratio(O.saturation_vapor_pressure(td), p)
    return w / (1.0 + w)


def base_heights(ncol, seed):
    """A hashed draw in 0 ... 1500 m per column, about 3 % of them NaN."""
    u = synth.column_uniforms(ncol, seed + 3000)
    return np.where(u[1] < 0.03, np.nan, 1500.0 * u[0])


def inputs(nlev, ncol, seed, dtype=np.float64):
    """p, T, Td, q (nlev, ncol) and base (ncol,): synth.columns with missing levels, q derived from (the dtype's) p and Td."""
    p, t, td = (a.astype(dtype) for a in synth.columns(nlev, ncol, seed=seed, nan_fraction=0.1))
    q = specific_humidity(p.astype(np.float64), td.astype(np.float64)).astype(dtype)
    return tuple(np.ascontiguousarray(a) for a in (p, t, td, q)) + (base_heights(ncol, seed).astype(dtype),)


HAND_LAYERS = ((R.PRESSURE, 900.0, 500.0), (R.PRESSURE_DEPTH, NAN, 150.0), (R.PRESSURE, NAN, NAN), (R.PRESSURE, 930.0, 620.0))
HAND_API_LAYERS = (('pressure', 900.0, 500.0), {'depth': 150.0}, {'bottom': None, 'top': None}, {'bottom': 930.0, 'top': 620.0})


def hand_columns():
    """Hand-built columns (nlev 8, ncol 8) for HAND_LAYERS: p, T, Td.
      0: isothermal 250 K;  1: T linear in ln p;  2: all NaN;  3: one valid level;  4: column 1 with a NaN temperature at level
      3 (dropped: the trapezoid spans the gap);  5: column 1 with the pressure of level 3 repeated at level 4 (ST_BAD_PRESSURE:
      heights below it stay);  6: column 1 -- the bounds 900 and 500 hPa of the first layer lie exactly on levels 2 and 5;
      7: column 1 with those two levels moved off the bounds by less than np.isclose's tolerance (they stand in for them).
    The dewpoint lies 4 ... 18 K below the temperature."""
    lev = np.array([1000.0, 950.0, 900.0, 800.0, 650.0, 500.0, 350.0, 200.0])
    p = lev[:, None] * np.ones((1, 8))
    p[2, 7], p[5, 7] = 900.004, 499.997
    t = 288.0 + 40.0 * (np.log(p) - np.log(1000.0))
    t[:, 0] = 250.0
    t[:, 2] = NAN
    t[:, 3] = NAN
    t[4, 3] = 262.0
    t[3, 4] = NAN
    p[4, 5] = p[3, 5]
    td = t - (4.0 + 2.0 * np.arange(8.0)[:, None])
    return p, t, td
