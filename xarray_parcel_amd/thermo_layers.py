"""
Temperature and humidity over caller-chosen layers on DataArrays: thermo_layers, and on top of it metpy.calc.precipitable_water,
the layer-mean relative humidity, lapse rate and thickness between two bounds, the hail-growth-zone thickness and the theta_e
difference, for every column of a grid through libxparcel (numpy_api.thermo_layers).  The reference has no counterparts, so
this lives next to the mirror (parcel_functions.py) rather than in it, and is built from the mirror's plumbing, as
kinematics.py and layer_cape.py.
"""
import numpy as np

from . import numpy_api as _api
from .parcel_functions import VERT, _Grid, _device

_ATTRS = {
    'precipitable_water': {'long_name': 'Precipitable water of the layer', 'units': 'mm'},
    'mean_mixing_ratio': {'long_name': 'Pressure-weighted mean mixing ratio of the layer', 'units': 'kg kg$^{-1}$'},
    'mean_relative_humidity': {'long_name': 'Pressure-weighted mean relative humidity of the layer', 'units': '1'},
    'thickness': {'long_name': 'Thickness of the layer', 'units': 'm'},
    'lapse_rate': {'long_name': 'Lapse rate between the bounds of the layer', 'units': 'K km$^{-1}$'},
    'theta_e_min': {'long_name': 'Smallest equivalent potential temperature of the layer', 'units': 'K'},
    'theta_e_min_pressure': {'long_name': 'Pressure of the smallest equivalent potential temperature of the layer', 'units': 'hPa'},
    'theta_e_max': {'long_name': 'Largest equivalent potential temperature of the layer', 'units': 'K'},
    'theta_e_max_pressure': {'long_name': 'Pressure of the largest equivalent potential temperature of the layer', 'units': 'hPa'},
    'status': {'long_name': 'Status bits'},
    'hail_growth_zone_thickness': {'long_name': 'Thickness of the layer between the -10 and -30 degC levels', 'units': 'm'},
    'hail_growth_zone_lapse_rate': {'long_name': 'Lapse rate between the -10 and -30 degC levels', 'units': 'K km$^{-1}$'},
    'theta_e_difference': {'long_name': 'Theta-e difference over the lowest 3 km', 'units': 'K'},
}


def _layer(g, spec):
    """A layer as numpy_api.thermo_layers takes it, per-column bounds (DataArrays on the horizontal dims) as their values."""
    if isinstance(spec, dict):
        return {k: g.per_col(v) for k, v in spec.items()}
    return tuple(spec[:1]) + tuple(g.per_col(v) for v in spec[1:])


def thermo_layers(pressure, temperature=None, dewpoint=None, height=None, layers=(), want=None, vert_dim=VERT):
    """Temperature and humidity over up to four layers of every column in one pass: `layers` as in numpy_api.thermo_layers --
    {'bottom': 700, 'top': 500}, {'depth': 100}, {'bottom_height': 0, 'top_height': 3000}, {'bottom': None, 'top': None} (the
    whole column), per-column 'bottom' / 'top' as DataArrays on the horizontal dims.  Returns a Dataset under the leading dim
    'thermo_layer' (the layer's index): precipitable water, the mean mixing ratio and relative humidity, thickness, lapse
    rate and the theta_e extremes with their pressures -- those that `want` names, by default every one the supplied inputs
    allow -- and the per-column status.  Layers that a column does not span are NaN."""
    g = _Grid(pressure, vert_dim)
    specs = [_layer(g, s) for s in layers]
    res = _device(_api.thermo_layers, g.values(pressure), g.per_col(temperature), g.per_col(dewpoint), g.per_col(height),
                  layers=specs, want=want)
    out = g.dataset(res, [k for k in res if k != 'status'], _ATTRS.get, vert=True, vcoord=np.arange(len(specs)),
                    dim='thermo_layer')
    out['status'] = g.horiz(res['status'], 'status', _ATTRS['status'])
    return out


def precipitable_water(pressure, dewpoint, bottom=None, top=None, vert_dim=VERT):
    """metpy.calc.precipitable_water [mm] of every column between `bottom` and `top` [hPa; scalars or DataArrays on the
    horizontal dims; None: the lowest / the highest valid level]."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.precipitable_water, g.values(pressure), g.values(dewpoint), bottom=g.per_col(bottom), top=g.per_col(top))
    return g.horiz(res, 'precipitable_water', _ATTRS['precipitable_water'])


def mean_relative_humidity(pressure, temperature, dewpoint, height=None, layer=('pressure', 700.0, 500.0), vert_dim=VERT):
    """The pressure-weighted mean relative humidity [0 ... 1] of one layer (default 700-500 hPa) of every column."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.mean_relative_humidity, g.values(pressure), g.values(temperature), g.values(dewpoint), g.per_col(height),
                  layer=_layer(g, layer))
    return g.horiz(res, 'mean_relative_humidity', _ATTRS['mean_relative_humidity'])


def layer_lapse_rate(pressure, temperature, height, layer=('pressure', 700.0, 500.0), vert_dim=VERT):
    """Lapse rate [K/km, positive where it cools upward] and thickness [m] between the bounds of one layer (default 700-500
    hPa) of every column, as a Dataset of lapse_rate and thickness."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.layer_lapse_rate, g.values(pressure), g.values(temperature), g.values(height), layer=_layer(g, layer))
    return g.dataset(dict(zip(('lapse_rate', 'thickness'), res)), attrs=_ATTRS.get)


def hail_growth_zone_thickness(pressure, temperature, height, vert_dim=VERT):
    """Thickness [m] and lapse rate [K/km] of the layer between the environment's lowest -10 degC and -30 degC levels of every
    column, as a Dataset of hail_growth_zone_thickness and hail_growth_zone_lapse_rate; NaN where the column has no -30 degC
    crossing or the two come in the wrong order."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.hail_growth_zone_thickness, g.values(pressure), g.values(temperature), g.values(height))
    return g.dataset(dict(zip(('hail_growth_zone_thickness', 'hail_growth_zone_lapse_rate'), res)), attrs=_ATTRS.get)


def theta_e_difference(pressure, temperature, dewpoint, height, vert_dim=VERT):
    """The theta_e-difference index [K] of every column: the largest minus the smallest equivalent potential temperature of
    the lowest 3 km, 0 where the largest lies above the smallest; NaN where the column does not reach 3 km."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.theta_e_difference, g.values(pressure), g.values(temperature), g.values(dewpoint), g.values(height))
    return g.horiz(res, 'theta_e_difference', _ATTRS['theta_e_difference'])
