"""The inputs of the isentropic-interpolation tests, shared by the census on the CPU (tests/test_isentropic_cpu.py) and the
device tests (tests/test_gpu_isentropic.py): the grids, the targets, two extra variables and hand-built columns."""
import numpy as np

from tests import isentropic_restatement as R
from xarray_parcel_amd import synth

# (nlev, ncol, seed) of every grid the device tests run; 65 columns: one wavefront plus one lane
GRIDS = {'12x640': (12, 640, 12), '40x640': (40, 640, 40), '7x65': (7, 65, 1), '24x300': (24, 300, 4)}
LEVELS = np.arange(285.0, 361.0, 5.0)                    # 16 targets, some below the surface theta, some above the column
LEVELS_64 = np.arange(280.0, 407.0, 2.0)                 # 64 targets
NAN = float('nan')


def inputs(nlev, ncol, seed, dtype=np.float64):
    """p, T and two extras (nlev, ncol): synth.columns with missing levels; the dewpoint (NaN wherever T is) and a hashed
    draw with its own NaNs sprinkled over a tenth of its points (on levels that stay valid)."""
    p, t, td = synth.columns(nlev, ncol, seed=seed, nan_fraction=0.1)
    rng = np.random.default_rng(seed + 2000)
    w = rng.uniform(-30.0, 30.0, p.shape) + 0.01 * p
    w = np.where(rng.uniform(size=p.shape) < 0.1, np.nan, w)
    return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (p, t, td, w))


def hand_columns():
    """Hand-built columns (nlev 6, ncol 7) and their targets: p, T, one extra, levels.
      0: theta increases strictly; the second target IS the theta of level 2, bit for bit;
      1: theta falls over the pair (2, 3): the first and the last crossing of 304 K differ;
      2: all NaN;  3: one valid level;  4: column 0 with a NaN temperature at level 2 (dropped, not interpolated through);
      5: dry adiabatic at 300 K (no crossing unless the target is that theta);  6: isothermal 250 K.
    Targets: 250.5 below every column's theta but the isothermal one's, 500 above all; the extra is NaN at level 4 of column 0."""
    p = np.array([1000.0, 900.0, 800.0, 650.0, 500.0, 300.0])[:, None] * np.ones((1, 7))
    x = np.log(p[:, 0])
    th0 = np.array([295.0, 298.0, 303.0, 309.0, 318.0, 335.0])
    th1 = np.array([296.0, 300.0, 308.0, 302.0, 310.0, 330.0])
    t = np.empty_like(p)
    for c, th in ((0, th0), (1, th1), (4, th0), (5, np.full(6, 300.0))):
        t[:, c] = th * np.exp(-R.KAPPA * (R.LN1000 - x))
    t[:, 2] = NAN
    t[:, 3] = NAN
    t[3, 3] = 270.0
    t[2, 4] = NAN
    t[:, 6] = 250.0
    v = 0.05 * p - np.arange(7.0)[None, :]
    v[4, 0] = NAN
    theta2 = float(R.theta_of(x[2], t[2, 0]))
    levels = np.array([250.5, theta2, 304.0, 312.5, 500.0])
    assert np.all(np.diff(levels) > 0)
    return p, t, v, levels
