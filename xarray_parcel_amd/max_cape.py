"""
CAPE / CIN of the maximum-CAPE parcel on DataArrays: a parcel is lifted from every level of the lowest `depth` hPa and the
one with the largest CAPE is kept (XP_PARCEL_MAX_CAPE, include/xparcel.h; numpy_api's parcel='max_cape') -- the
"most-unstable CAPE" of the archives that define it that way, where the reference's most unstable parcel is the level of
highest theta-e.  The reference has no counterpart, so this lives next to the mirror (parcel_functions.py) rather than in
it, and is built from the mirror's plumbing, as ground.py.
"""
from . import numpy_api as _api
from .parcel_functions import VERT, _Grid, _device, _moisture

_CAPE = 'J kg$^{-1}$'
_ATTRS = {
    'cape': {'long_name': 'Convective available potential energy of the maximum-CAPE parcel', 'units': _CAPE},
    'cin': {'long_name': 'Convective inhibition of the maximum-CAPE parcel', 'units': _CAPE},
    'lcl_pressure': {'long_name': 'Lifting condensation level pressure', 'units': 'hPa'},
    'lcl_temperature': {'long_name': 'Lifting condensation level temperature', 'units': 'K'},
    'lcl_virtual_temperature': {'long_name': 'Lifting condensation level virtual temperature', 'units': 'K'},
    'lfc_pressure': {'long_name': 'Level of free convection pressure', 'units': 'hPa'},
    'lfc_temperature': {'long_name': 'Level of free convection temperature', 'units': 'K'},
    'el_pressure': {'long_name': 'Equilibrium level pressure', 'units': 'hPa'},
    'el_temperature': {'long_name': 'Equilibrium level temperature', 'units': 'K'},
    'lfc_index': {'long_name': 'Interval of the LFC, counted from the parcel level'},
    'el_index': {'long_name': 'Interval of the EL, counted from the parcel level'},
    'status': {'long_name': 'Status bits'},
    'parcel_index': {'long_name': 'Level of the parcel: the departure level with the largest CAPE'},
    'parcel_pressure': {'long_name': 'Parcel pressure', 'units': 'hPa'},
    'parcel_temperature': {'long_name': 'Parcel temperature', 'units': 'K'},
    'parcel_dewpoint': {'long_name': 'Parcel dewpoint', 'units': 'K'},
}
_PARCEL = {'pressure': 'parcel_pressure', 'temperature': 'parcel_temperature', 'dewpoint': 'parcel_dewpoint', 'index': 'parcel_index'}


def max_cape_cape_cin(pressure, temperature, dewpoint, vert_dim=VERT, depth=300, **kwargs):
    """CAPE / CIN of the parcel with the largest CAPE among the levels of the lowest `depth` hPa.  pressure [hPa],
    temperature, dewpoint [K] on the same dims with `vert_dim` among them.  Returns a Dataset of the per-column scalars
    (cape, cin, the LCL, LFC and EL, status, the parcel; parcel_index is the level, lfc_index / el_index count from it); no
    profile.  kwargs: want, moist and the CAPE / CIN options of numpy_api.cape_cin_columns; among them humidity='relative'
    (`dewpoint` holds relative humidity as a fraction; percent is refused) or 'mixing_ratio' [kg/kg], not 'specific'."""
    g = _Grid(temperature, vert_dim)
    res = _device(_api.cape_cin_columns, g.values(pressure), g.values(temperature), _moisture(g, dewpoint, kwargs),
                  parcel='max_cape', depth=depth, **kwargs)
    return g.dataset(res, attrs=_ATTRS.get)


def max_cape_parcel(pressure, temperature, dewpoint, vert_dim=VERT, depth=300):
    """The parcel itself: a Dataset of parcel_pressure, parcel_temperature, parcel_dewpoint and parcel_index per column
    (default options, exact moist adiabat)."""
    g = _Grid(temperature, vert_dim)
    res = _device(_api.max_cape_parcel, g.values(pressure), g.values(temperature), g.values(dewpoint), depth=depth)
    return g.dataset({_PARCEL[k]: v for k, v in res.items()}, attrs=_ATTRS.get)
