"""The inputs of the sounding-indices tests, shared by the census on the CPU (tests/test_sounding_indices_cpu.py) and the device
tests (tests/test_gpu_sounding_indices.py): the grids, their winds, and hand-built columns."""
import numpy as np

from tests.test_gpu_dcape import inputs as dcape_inputs

KNOT = 1852.0 / 3600.0
# (nlev, ncol, seed) of every grid the device tests run
GRIDS = {'12x640': (12, 640, 12), '40x640': (40, 640, 40), '7x65': (7, 65, 1), '40x96': (40, 96, 8), '40x320': (40, 320, 11),
         '40x480': (40, 480, 5), '24x300': (24, 300, 4)}


def wind_from(speed_kt, direction):
    """(u, v) [m/s] of a wind of `speed_kt` knots FROM `direction` degrees."""
    r = np.deg2rad(direction)
    return -speed_kt * KNOT * np.sin(r), -speed_kt * KNOT * np.cos(r)


def winds(p, seed):
    """u, v [m/s] on the levels of p (nlev, ncol): speed and direction linear in ln p through a draw at 850 hPa (direction
    100 ... 280, 5 ... 40 kt) and one at 500 hPa (180 ... 340, 5 ... 60 kt) -- the SWEAT shear term is on in about a fifth of
    the columns.  A tenth of the columns has NaN winds sprinkled over its levels (wind-valid levels that differ from the
    thermodynamically valid ones), one in thirty no winds below 800 hPa (the wind levels do not span 850 hPa)."""
    rng = np.random.default_rng(seed + 1000)
    ncol = p.shape[1]
    d850, d500 = rng.uniform(100.0, 280.0, ncol), rng.uniform(180.0, 340.0, ncol)
    f850, f500 = rng.uniform(5.0, 40.0, ncol), rng.uniform(5.0, 60.0, ncol)
    with np.errstate(invalid='ignore'):
        s = (np.log(850.0) - np.log(p)) / (np.log(850.0) - np.log(500.0))
    u, v = wind_from(np.maximum(f850 + (f500 - f850) * s, 0.0), d850 + (d500 - d850) * s)
    sprinkle = (rng.uniform(size=ncol) < 0.1)[None, :] & (rng.uniform(size=p.shape) < 0.15)
    low = (rng.uniform(size=ncol) < 1.0 / 30.0)[None, :] & (p > 800.0)
    u, v = np.where(sprinkle | low, np.nan, u), np.where(sprinkle | low, np.nan, v)
    return u, v


def inputs(nlev, ncol, seed, dtype=np.float64):
    """p, T, Td, u, v (nlev, ncol): synth.columns with missing levels and test_gpu_dcape's elevated and truncated eighths (the
    columns that do not span 850 ... 500 hPa); a third eighth with a Gaussian inversion (8 ... 14 K, 40 ... 80 hPa wide, centred on the
    level nearest to a draw from 700 ... 820 hPa, the dewpoint depression below it at most 1.5 K: rt crosses T more than once
    there); the last column isothermal and dry (rt stays below T: no CCL); winds()."""
    p, t, td = (a.astype(np.float64) for a in dcape_inputs(nlev, ncol, seed))
    rng = np.random.default_rng(seed + 500)
    n = ncol // 8
    cols = np.arange(2 * n, 3 * n)
    amp, pc, w = rng.uniform(8.0, 14.0, n), rng.uniform(700.0, 820.0, n), rng.uniform(40.0, 80.0, n)
    near = np.abs(np.where(np.isnan(p[:, cols]), np.inf, p[:, cols]) - pc)
    pc = np.where(np.isfinite(near.min(axis=0)), p[near.argmin(axis=0), cols], pc)       # (ON a level: a coarse grid sees it too)
    t[:, cols] += amp * np.exp(-((p[:, cols] - pc) / w) ** 2)
    with np.errstate(invalid='ignore'):                       # (a moist layer under the inversion: the lowest crossing lies below it)
        moist = (p[:, cols] > pc + w) & (td[:, cols] < t[:, cols] - 1.5)
    td[:, cols] = np.where(moist, t[:, cols] - 1.5, td[:, cols])
    t[:, -1] = 300.0
    td[:, -1] = 290.0
    u, v = winds(p, seed)
    return tuple(a.astype(dtype) for a in (p, t, td, u, v))


def mandatory_columns():
    """Hand-built columns (nlev 6, ncol 3) with levels exactly at 850, 700 and 500 hPa: p, T, Td, u, v."""
    p = np.array([1000.0, 925.0, 850.0, 700.0, 500.0, 300.0])[:, None] * np.ones((1, 3))
    t = np.array([[299.3, 294.1, 288.7], [294.2, 290.4, 284.6], [289.9, 286.2, 281.3], [280.1, 277.7, 272.2], [262.4, 258.3, 254.9],
                  [231.0, 228.0, 226.5]])
    td = t - np.array([[3.1, 6.0, 1.2], [2.5, 7.5, 1.9], [2.0, 9.0, 14.5], [6.5, 12.0, 21.0], [14.0, 20.0, 30.0], [25.0, 28.0, 33.0]])
    u, v = wind_from(np.array([[8.0], [15.0], [25.0], [35.0], [45.0], [70.0]]) * np.ones((1, 3)),
                     np.array([[150.0], [165.0], [180.0], [215.0], [250.0], [265.0]]) + np.array([[0.0, 10.0, -30.0]]))
    return p, t, td, u, v
