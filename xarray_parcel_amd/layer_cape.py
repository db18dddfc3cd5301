"""
CAPE / CIN over layers of the ascent on DataArrays: cape_cin_layers, and on top of it 0-3 km CAPE and hail-growth-zone CAPE,
for every column of a grid through libxparcel (numpy_api.cape_cin_layers).  The reference has no counterparts, so this
lives next to the mirror (parcel_functions.py) rather than in it, and is built from the mirror's plumbing, as kinematics.py.
"""
import numpy as np

from . import numpy_api as _api
from .parcel_functions import VERT, _Grid, _device, _moisture

_CAPE = 'J kg$^{-1}$'
_ATTRS = {
    'cape': {'long_name': 'CAPE inside the layer', 'units': _CAPE},
    'cin': {'long_name': 'CIN inside the layer', 'units': _CAPE},
    'bottom_pressure': {'long_name': 'Layer bottom pressure (NaN: the first node of the ascent)', 'units': 'hPa'},
    'top_pressure': {'long_name': 'Layer top pressure', 'units': 'hPa'},
    'total_cape': {'long_name': 'CAPE', 'units': _CAPE},
    'total_cin': {'long_name': 'CIN', 'units': _CAPE},
    'lfc_pressure': {'long_name': 'LFC pressure', 'units': 'hPa'},
    'el_pressure': {'long_name': 'EL pressure', 'units': 'hPa'},
    'lcl_pressure': {'long_name': 'LCL pressure', 'units': 'hPa'},
    'status': {'long_name': 'Status bits'},
    'cape_3km': {'long_name': 'CAPE between the surface and 3 km above it', 'units': _CAPE},
    'hail_growth_zone_cape': {'long_name': 'CAPE between the -10 and -30 degC levels', 'units': _CAPE},
}
_PER_LAYER = ('cape', 'cin', 'bottom_pressure', 'top_pressure')
_PER_COLUMN = ('total_cape', 'total_cin', 'lfc_pressure', 'el_pressure', 'lcl_pressure', 'status')


def cape_cin_layers(pressure, temperature, dewpoint, layers, height=None, vert_dim=VERT, parcel='surface', depth=None,
                    parcel_values=None, moist=None, **cape_cin_options):
    """CAPE and CIN [J/kg] of every column over 1 ... 4 layers of one ascent: `layers` as numpy_api.cape_cin_layers takes
    them (dicts of 'bottom' / 'top' [hPa], '..._height' [m above the lowest valid level], '..._temperature' [K]; per-column
    bounds as DataArrays on the horizontal dims).  Returns a Dataset: cape, cin and the resolved bottom_pressure /
    top_pressure under the leading dim 'layer', and total_cape, total_cin, lfc_pressure, el_pressure, lcl_pressure and
    status on the horizontal dims.  A layer with a NaN top or top >= bottom is NaN.  humidity='relative' (a fraction; percent is
    refused) or 'mixing_ratio' [kg/kg] among the options: what `dewpoint` holds."""
    g = _Grid(pressure, vert_dim)
    specs = [{k: g.per_col(v) for k, v in l.items()} for l in layers]
    pv = None if parcel_values is None else [g.per_col(x) for x in parcel_values]
    res = _device(_api.cape_cin_layers, g.values(pressure), g.values(temperature), _moisture(g, dewpoint, cape_cin_options),
                  specs, height=g.per_col(height), parcel=parcel, depth=depth, parcel_values=pv, moist=moist, **cape_cin_options)
    out = g.dataset(res, _PER_LAYER, _ATTRS.get, vert=True, vcoord=np.arange(len(specs)), dim='layer')
    for k in _PER_COLUMN:
        out[k] = g.horiz(res[k], k, _ATTRS[k])
    return out


def _one(fn, name, pressure, temperature, dewpoint, height, vert_dim, kwargs):
    g = _Grid(pressure, vert_dim)
    if kwargs.get('parcel_values') is not None:
        kwargs = dict(kwargs, parcel_values=[g.per_col(x) for x in kwargs['parcel_values']])
    res = _device(fn, g.values(pressure), g.values(temperature), _moisture(g, dewpoint, kwargs), g.values(height), **kwargs)
    return g.horiz(res, name, _ATTRS[name])


def cape_3km(pressure, temperature, dewpoint, height, vert_dim=VERT, **kwargs):
    """0-3 km CAPE [J/kg] of every column: the CAPE of the ascent between its first node and 3000 m above the lowest valid
    level.  kwargs: parcel, depth, parcel_values, moist and the CAPE / CIN options of cape_cin_layers."""
    return _one(_api.cape_3km, 'cape_3km', pressure, temperature, dewpoint, height, vert_dim, kwargs)


def hail_growth_zone_cape(pressure, temperature, dewpoint, height, vert_dim=VERT, **kwargs):
    """Hail-growth-zone CAPE [J/kg] of every column: the CAPE of the ascent between the environment's lowest -10 degC and
    -30 degC levels; NaN where the column has no -30 degC crossing or the two come in the wrong order, from the first node
    of the ascent where it has no -10 degC crossing (a surface already colder).  kwargs as cape_3km."""
    return _one(_api.hail_growth_zone_cape, 'hail_growth_zone_cape', pressure, temperature, dewpoint, height, vert_dim, kwargs)
