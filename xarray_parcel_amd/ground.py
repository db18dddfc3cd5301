"""
CAPE / CIN of pressure-level data on DataArrays: isobaric levels (one set of isobars, values extrapolated below the terrain)
plus the surface as separate 2-D fields -- surface pressure, 2 m temperature, 2 m dewpoint -- as reanalyses and climate
archives deliver them.  Every column is cut at its surface pressure and lifted from there (XP_PARCEL_OVER_GROUND,
include/xparcel.h; numpy_api's ground=).  The reference takes model levels only and has no counterparts, so this lives
next to the mirror (parcel_functions.py) rather than in it, and is built from the mirror's plumbing, as layer_cape.py.
"""
import numpy as np

from . import numpy_api as _api
from ._xr import Dataset
from .parcel_functions import VERT, _Grid, _device, _moisture

_CAPE = 'J kg$^{-1}$'
_ATTRS = {
    'cape': {'long_name': 'Convective available potential energy', 'units': _CAPE},
    'cin': {'long_name': 'Convective inhibition', 'units': _CAPE},
    'lcl_pressure': {'long_name': 'Lifting condensation level pressure', 'units': 'hPa'},
    'lcl_temperature': {'long_name': 'Lifting condensation level temperature', 'units': 'K'},
    'lcl_virtual_temperature': {'long_name': 'Lifting condensation level virtual temperature', 'units': 'K'},
    'lfc_pressure': {'long_name': 'Level of free convection pressure', 'units': 'hPa'},
    'lfc_temperature': {'long_name': 'Level of free convection temperature', 'units': 'K'},
    'el_pressure': {'long_name': 'Equilibrium level pressure', 'units': 'hPa'},
    'el_temperature': {'long_name': 'Equilibrium level temperature', 'units': 'K'},
    'lfc_index': {'long_name': 'Interval of the LFC, counted from the surface row'},
    'el_index': {'long_name': 'Interval of the EL, counted from the surface row'},
    'status': {'long_name': 'Status bits'},
    'parcel_index': {'long_name': 'Source row of the parcel (0: the surface; 1 + j: the j-th level above the ground)'},
    'parcel_pressure': {'long_name': 'Parcel pressure', 'units': 'hPa'},
    'parcel_temperature': {'long_name': 'Parcel temperature', 'units': 'K'},
    'parcel_dewpoint': {'long_name': 'Parcel dewpoint', 'units': 'K'},
    'levels_below_ground': {'long_name': 'Isobaric levels at or below the surface pressure (dropped)'},
}


def levels_below_ground(pressure, surface_pressure):
    """k0 per column: the index of the first level whose pressure is below the surface pressure (a plain comparison: NaN
    compares false), nlev where there is none.  pressure: (nlev, ...) or the nlev isobars, vertical first."""
    p, ps = np.asarray(pressure), np.asarray(surface_pressure)
    p = p.reshape(p.shape[0], -1)
    with np.errstate(invalid='ignore'):
        above = p < ps.reshape(1, -1)
    return np.where(above.any(axis=0), above.argmax(axis=0), p.shape[0]).astype(np.int32).reshape(ps.shape)


def _inputs(pressure, temperature, dewpoint, surface, vert_dim, kwargs):
    g = _Grid(temperature, vert_dim)
    return g, g.values(pressure), g.values(temperature), _moisture(g, dewpoint, kwargs), tuple(g.values(x) for x in surface)


def _dataset(g, res, p, ps, suffix=''):
    out = {k + suffix: g.horiz(v, k + suffix, _ATTRS.get(k)) for k, v in res.items()}
    out['levels_below_ground'] = g.horiz(levels_below_ground(p, ps), 'levels_below_ground', _ATTRS['levels_below_ground'])
    return out


def _cape_cin(parcel, depth, pressure, temperature, dewpoint, surface, vert_dim, kwargs):
    g, p, t, td, sfc = _inputs(pressure, temperature, dewpoint, surface, vert_dim, kwargs)
    res = _device(_api.cape_cin_columns, p, t, td, parcel=parcel, depth=depth, ground=sfc, **kwargs)
    return Dataset(_dataset(g, res, p, sfc[0]))


def surface_based_cape_cin(pressure, temperature, dewpoint, surface_pressure, surface_temperature, surface_dewpoint,
                           vert_dim=VERT, **kwargs):
    """CAPE / CIN of the parcel at the surface (ps, 2 m temperature, 2 m dewpoint) lifted through the isobaric levels above
    it.  pressure [hPa]: on the dims of `temperature`, or the isobars on `vert_dim` alone; temperature, dewpoint [K] on the
    levels (humidity='specific' / 'relative' / 'mixing_ratio': specific humidity [kg/kg], relative humidity as a fraction or
    the mixing ratio [kg/kg] on the levels, the surface stays a dewpoint; relative humidity in percent is refused); the
    surface fields on the
    horizontal dims.  Returns a Dataset of the per-column scalars (cape, cin, the LCL, LFC and EL, status, the parcel; indices
    count the rows of the column cut at the ground) and levels_below_ground; no profile.  kwargs: want, moist and the CAPE /
    CIN options of numpy_api.cape_cin_columns."""
    return _cape_cin('surface', None, pressure, temperature, dewpoint, (surface_pressure, surface_temperature, surface_dewpoint),
                     vert_dim, kwargs)


def most_unstable_cape_cin(pressure, temperature, dewpoint, surface_pressure, surface_temperature, surface_dewpoint,
                           vert_dim=VERT, depth=300, **kwargs):
    """As surface_based_cape_cin for the most unstable parcel of the lowest `depth` hPa above the surface (the surface
    included)."""
    return _cape_cin('most_unstable', depth, pressure, temperature, dewpoint,
                     (surface_pressure, surface_temperature, surface_dewpoint), vert_dim, kwargs)


def mixed_layer_cape_cin(pressure, temperature, dewpoint, surface_pressure, surface_temperature, surface_dewpoint,
                         vert_dim=VERT, depth=100, **kwargs):
    """As surface_based_cape_cin for the parcel mixed over the lowest `depth` hPa above the surface."""
    return _cape_cin('mixed_layer', depth, pressure, temperature, dewpoint,
                     (surface_pressure, surface_temperature, surface_dewpoint), vert_dim, kwargs)


def cape_cin_multi(pressure, temperature, dewpoint, surface_pressure, surface_temperature, surface_dewpoint, parcels,
                   vert_dim=VERT, **kwargs):
    """Several parcels of one grid in one call, the grid cut at the ground once: `parcels` as numpy_api.cape_cin_multi takes
    them, e.g. ['surface', ('most_unstable', 300), ('mixed_layer', 100)].  Returns one Dataset: the scalars of parcel i
    carry the suffix '_<i>', levels_below_ground none."""
    g, p, t, td, sfc = _inputs(pressure, temperature, dewpoint,
                               (surface_pressure, surface_temperature, surface_dewpoint), vert_dim, kwargs)
    outs = _device(_api.cape_cin_multi, p, t, td, parcels, ground=sfc, **kwargs)
    out = {}
    for i, res in enumerate(outs):
        out.update(_dataset(g, res, p, sfc[0], '_%d' % i))
    return Dataset(out)
