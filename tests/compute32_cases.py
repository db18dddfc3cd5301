"""The grids of the xp_opts.compute = XP_F32 tests (tests/test_compute32_cpu.py, tests/test_gpu_compute32.py) and the
NumPy census of their doubt columns: the columns in which the fp32 walk (csrc/xp_cape_f32.hpp) meets a node whose
parcel-minus-environment difference is smaller than XP_F32_GUARD and evaluates it again in fp64.

All grids are float32, and small: their column counts are no multiples of 64 or 256, they hold NaN, saturated,
many-crossing and single-level columns -- the smallest on which this kernel can go wrong in an interesting way."""
import functools
import os
import re

import numpy as np

from oracle import c_oracle as co
from tests import layered_soundings as ls
from xarray_parcel_amd import _lib, synth

HPP = os.path.join(_lib.SRC_DIR, 'xp_cape_f32.hpp')


def guard():
    """XP_F32_GUARD [K] as committed in csrc/xp_cape_f32.hpp."""
    with open(HPP) as fh:
        m = re.search(r'constexpr float XP_F32_GUARD = ([0-9.eE+-]+)f;', fh.read())
    assert m, 'XP_F32_GUARD not found in xp_cape_f32.hpp'
    return float(m.group(1))


def _freeze(arrs):
    arrs = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in arrs)
    for a in arrs:
        a.setflags(write=False)
    return arrs


EDGE_HIGH_SURFACE = (70, 73, 77, 85)     # the columns of `edges` whose surface, and LCL, lie above 1100 hPa (CAPE 0, 831, 3623, 10216 J/kg)


def edges(nlev=33, ncol=1000):
    """The columns that leave the family table, as tests/test_gpu_family_piece_walk.py holds the fp64 family kernel to them:
    every third column stretched above its middle level so that its top level lies at 12 hPa (the sounding below is left
    alone, with its CAPE; the upper levels are above the table's top at ~20 hPa: the dry continuation), four surfaces -- and LCLs -- above 1100 hPa (outside the table: flagged, redone by the RK4 launch),
    and in every seventh column one NaN pressure well above the LCL."""
    p, t, td = synth.columns(nlev=nlev, ncol=ncol, seed=77, dtype=np.float64)
    k = np.maximum(np.arange(nlev, dtype=np.float64) - nlev // 2, 0.0)[:, None] / (nlev - 1 - nlev // 2)
    p[:, ::3] = p[:, ::3] * (12.0 / p[-1, ::3])[None, :] ** k
    p[0, list(EDGE_HIGH_SURFACE)] = 1105.0
    td[0, list(EDGE_HIGH_SURFACE)] = t[0, list(EDGE_HIGH_SURFACE)] - 0.2
    p[nlev - 8, 5::7] = np.nan
    return p, t, td


@functools.lru_cache(maxsize=None)
def grid(name):
    """(p, t, td) float32, read-only, computed once per process."""
    if name == 'hashed64':
        return _freeze(synth.columns(64, 6007, seed=31, nan_fraction=0.1, dtype=np.float32))
    if name == 'hashed128':
        return _freeze(synth.columns(128, 6007, seed=32, dtype=np.float32))
    if name == 'layered48':
        return _freeze(ls.grid(*ls.GRID_A, dtype=np.float32))
    if name == 'one_level':
        return _freeze(a[:1] for a in synth.columns(8, 257, seed=33, dtype=np.float32))
    if name == 'two_levels':
        return _freeze(a[:2] for a in synth.columns(8, 257, seed=34, dtype=np.float32))
    if name == 'one_column':
        return _freeze(synth.columns(40, 1, seed=35, dtype=np.float32))
    if name == 'no_columns':
        return _freeze(a[:, :0] for a in synth.columns(40, 1, seed=35, dtype=np.float32))
    if name == 'edges':
        return _freeze(edges())
    raise KeyError(name)


GRIDS = ('hashed64', 'hashed128', 'layered48', 'edges', 'one_level', 'two_levels', 'one_column', 'no_columns')
CENSUS_GRIDS = ('hashed64', 'hashed128')


@functools.lru_cache(maxsize=None)
def oracle(name, moist='rk4'):
    """The C oracle on the float32-rounded inputs (as tests/test_gpu_parity.py feeds it), with the profile; computed once."""
    p, t, td = grid(name)
    return co.cape_cin_grid(p, t, td, parcel='surface', moist=moist, want_profile=True)


def census(name, g=None):
    """From the oracle's profile: {'doubt': columns with some profile node above node 0 whose |Tv_parcel - Tv_env| < g,
    'saturated': columns whose LCL lies on the parcel's own level}, boolean (ncol,) arrays."""
    g = guard() if g is None else g
    ref = oracle(name)
    prof = ref['profile']
    with np.errstate(invalid='ignore'):
        y = prof['virtual_temperature'] - prof['environment_virtual_temperature']
        doubt = (np.abs(y[1:]) < g).any(axis=0)
        saturated = ref['lcl_pressure'] == prof['pressure'][0]
    return {'doubt': doubt, 'saturated': saturated}
