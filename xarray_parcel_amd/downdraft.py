"""
Downdraft CAPE on DataArrays: metpy.calc.downdraft_cape for every column of a grid, through libxparcel
(numpy_api.downdraft_cape).  The reference has no counterpart, so this lives next to the mirror (parcel_functions.py)
rather than in it, and is built from the mirror's plumbing: a _Grid splits the inputs and wraps the results, _device
turns the library's missing-tables error into the reference's assert, and the moist mode defaults as in the mirror
(parcel_functions.set_moist_lapse; None = the lookup tables).
"""
from . import numpy_api as _api
from .parcel_functions import VERT, _Grid, _device, _moist_mode

_ATTRS = {
    'dcape': {'long_name': 'Downdraft convective available potential energy', 'units': 'J kg$^{-1}$'},
    'dcape_start_pressure': {'long_name': 'Pressure of the downdraft parcel start (minimum theta-e in the layer)',
                             'units': 'hPa'},
    'dcape_start_temperature': {'long_name': 'Wet bulb temperature of the downdraft parcel start', 'units': 'K'},
    'dcape_parcel_temperature': {'long_name': 'Downdraft parcel temperature', 'units': 'K'},
}
_KEYS = {'dcape': 'dcape', 'start_pressure': 'dcape_start_pressure', 'start_temperature': 'dcape_start_temperature'}


def downdraft_cape(pressure, temperature, dewpoint, vert_dim=VERT, bottom=700, depth=200, moist=None):
    """Downdraft CAPE of the saturated parcel that starts at the minimum of theta-e in the layer from `bottom` up `depth`
    hPa (MetPy: 700 and 200) and descends moist-adiabatically to the surface.  Returns (Dataset of dcape [J/kg],
    dcape_start_pressure and dcape_start_temperature on the horizontal dims, DataArray dcape_parcel_temperature on the
    input's dims: NaN above the start and on missing levels) -- MetPy's (dcape, down_pressure, down_parcel_trace) for a
    grid.  Columns that do not span the layer (MetPy raises) are NaN throughout."""
    moist = _moist_mode(moist)
    g = _Grid(pressure, vert_dim)
    res = _device(_api.downdraft_cape, g.values(pressure), g.values(temperature), g.values(dewpoint), bottom=bottom,
                  depth=depth, moist=moist, want_profile=True)
    ds = g.dataset({name: res[k] for k, name in _KEYS.items()}, attrs=_ATTRS.get)
    return ds, g.vert(res['parcel_temperature'], 'dcape_parcel_temperature', _ATTRS['dcape_parcel_temperature'])
