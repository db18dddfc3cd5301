"""Layered soundings for the streaming CAPE / CIN kernels (TEST INFRASTRUCTURE, the counterpart of tests/component_cases.py).

xarray_parcel_amd.synth builds one constant lapse rate, at most one warm bump and a dewpoint depression that grows with height:
an ascent through it has at most two positive areas, and the most-unstable parcel is the surface or sits in the one bump.
layered() stacks random layers on the same background -- stable, neutral and steep ones, moist and dry ones, each one to
six levels deep -- so that the parcel-minus-environment curve changes sign up to nine times per column, the most-unstable
parcel starts anywhere in the lowest 300 hPa, and the lanes of a wavefront reach their LCL on widely different levels.

Every pressure, temperature and dewpoint is a multiple of 1/64, so a float32 grid holds exactly the float64 numbers and
both dtypes are compared with one oracle run's inputs.  No level but a saturated surface (3 % of the columns, as in synth)
can be saturated: the smallest depression is 0.25 K.

census() classifies what the C oracle makes of a grid; tests/test_layered_soundings_cpu.py holds its floors."""
import functools

import numpy as np

from xarray_parcel_amd import synth

SLOPES = np.array([+3.3, +5.0, 0.0, -1.0, -2.3, -6.5, -12.0, +1.0, -3.5, +2.8])      # K/km added to the background; > 0: more stable
DEPRESSIONS = np.array([0.25, 1.0, 3.0, 8.0, 15.0, 30.0, 2.0, 0.5])                   # K
MAX_HOLD = 6                                                                          # a layer is 1 ... 6 levels deep
PERT_CLIP = 6.0                                                                       # K
Q = 64.0                                                                              # every value is a multiple of 1 / Q

GRID_A = (48, 6007, 5)              # 6007 = 5 * 1024 + 13 * 64 + 55: last block, last wavefront, last 1024-column workgroup all ragged
GRID_B = (20, 6007, 6)
GRID_REPLAY = (40, 3000, 11)        # the kernels that replay the ascent (layer CAPE, effective inflow layer, NCAPE)
GRID_ORACLES = (30, 240, 9)         # NumPy oracle against C oracle
NAN_FRACTION = 0.08
PARCELS = ('surface', 'most_unstable', 'mixed_layer')
OPTION_SETS = [dict(), dict(virtual_temperature_correction=False, lcl_interp='linear'), dict(pos_cape_neg_cin=False),
               dict(post_zero_cin=True, lcl_interp='linear', virtual_temperature_correction=True),
               dict(pos_cape_neg_cin=False, post_zero_cin=True)]                      # O0 ... O3 = test_gpu_parity.MODES[:4], O4


def layered(nlev, ncol, seed, nan_fraction=0.0, dtype=np.float64):
    """(p, t, td), each (nlev, ncol): a pure function of the arguments."""
    rng = np.random.default_rng(seed)
    p, tb, _ = synth.columns(nlev, ncol, seed=seed)
    p = np.round(p * Q) / Q
    assert np.all(np.diff(p, axis=0) < 0), 'pressure no longer decreases strictly after rounding'
    z_km = 29.27e-3 * 260.0 * np.log(p[0] / p)
    kind = rng.integers(0, SLOPES.size, (nlev, ncol))                   # the draws, in this order
    dep = rng.integers(0, DEPRESSIONS.size, (nlev, ncol))
    hold = rng.integers(1, MAX_HOLD + 1, (nlev, ncol))
    slope = np.empty((nlev, ncol))
    depression = np.empty((nlev, ncol))
    left = np.zeros(ncol, dtype=np.int64)
    cur_s, cur_d = np.zeros(ncol), np.zeros(ncol)
    for j in range(nlev):
        new = left == 0                                                 # the layer is used up: level j's draw takes over
        cur_s = np.where(new, SLOPES[kind[j]], cur_s)
        cur_d = np.where(new, DEPRESSIONS[dep[j]], cur_d)
        left = np.where(new, hold[j], left) - 1
        slope[j], depression[j] = cur_s, cur_d
    pert = np.zeros((nlev, ncol))
    for j in range(nlev - 1):
        pert[j + 1] = np.clip(pert[j] + slope[j] * (z_km[j + 1] - z_km[j]), -PERT_CLIP, PERT_CLIP)
    t = np.round((tb + pert) * Q) / Q
    td = t - depression
    saturated = synth.column_uniforms(ncol, seed)[8] < 0.03
    td[0, saturated] = t[0, saturated]
    if nan_fraction > 0:
        _, tn, _ = synth.columns(nlev, ncol, seed=seed, nan_fraction=nan_fraction, saturate_some=False)
        blank = np.isnan(tn)
        t[blank] = np.nan
        td[blank] = np.nan
    out = tuple(np.ascontiguousarray(a.astype(dtype)) for a in (p, t, td))
    for a, b in zip(out, (p, t, td)):
        assert np.array_equal(a.astype(np.float64), b, equal_nan=True), 'the grid is not exact in %s' % np.dtype(dtype).name
    return out


@functools.lru_cache(maxsize=None)
def grid(nlev, ncol, seed, dtype=np.float64, nan_fraction=NAN_FRACTION):
    """layered(), computed once per process and read-only."""
    out = layered(nlev, ncol, seed, nan_fraction=nan_fraction, dtype=dtype)
    for a in out:
        a.setflags(write=False)
    return out


def sign_changes(diff):
    """Per column: the sign changes between adjacent nodes of a (nnode, ncol) parcel-minus-environment array.  A NaN node
    separates its neighbours, as it does in the reference's find_intersections."""
    with np.errstate(invalid='ignore'):
        s = np.sign(diff)
        return (s[1:] * s[:-1] < 0).sum(axis=0)


def census(ref):
    """What the C oracle's result `ref` (want_profile=True, default options) and its net-sum result hold, per column.
    Returns a dict of (ncol,) arrays."""
    prof = ref['profile']
    pp, lcl = prof['pressure'], ref['lcl_pressure']
    with np.errstate(invalid='ignore'):
        above = pp < lcl[None, :]
    diff = np.where(above, prof['virtual_temperature'] - prof['environment_virtual_temperature'], np.nan)
    with np.errstate(invalid='ignore', all='ignore'):
        first = np.where(np.isnan(pp).all(axis=0), np.nan, np.nanmax(np.where(np.isnan(pp), -np.inf, pp), axis=0))
    return {'changes': sign_changes(diff), 'zero_nodes': (diff == 0.0).sum(axis=0), 'lfc_is_lcl': ref['lfc_index'] == -2,
            'lcl_on_parcel': lcl == first, 'lfc_no_el': ~np.isnan(ref['lfc_pressure']) & np.isnan(ref['el_pressure'])}
