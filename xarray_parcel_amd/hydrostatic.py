"""
Hydrostatic heights and layer thickness on DataArrays: the height of every level from pressure, temperature and humidity,
metpy.calc.thickness_hydrostatic, geopotential_to_height and height_to_geopotential for every column of a grid through
libxparcel (numpy_api.hydrostatic; include/xparcel.h has the rules).  The reference has no counterparts, so this lives next
to the mirror (parcel_functions.py) rather than in it, and is built from the mirror's plumbing, as thermo_layers.py and
isentropic.py.
"""
import numpy as np

from . import numpy_api as _api
from ._xr import DataArray, Dataset
from .parcel_functions import VERT, _Grid, _device, _host

_ATTRS = {
    'height': {'long_name': 'Hydrostatic height', 'units': 'm'},
    'thickness': {'long_name': 'Hydrostatic thickness of the layer', 'units': 'm'},
    'status': {'long_name': 'Status bits'},
    'geopotential': {'long_name': 'Geopotential', 'units': 'm$^{2}$ s$^{-2}$'},
    'geopotential_height': {'long_name': 'Height from geopotential', 'units': 'm'},
}


def hydrostatic(pressure, temperature, dewpoint=None, specific_humidity=None, base_height=None, layers=(), want=None,
                vert_dim=VERT):
    """Hydrostatic heights and the thickness of up to four layers by pressure in one pass, as a Dataset: 'height' on the
    dims of `temperature` (vertical first), 'thickness' per column under the leading dim 'hydrostatic_layer' (the layer's
    index; absent without layers) and the per-column 'status' -- or those that `want` names.  Arguments as numpy_api.hydrostatic: dewpoint OR
    specific_humidity (neither: dry), base_height a scalar or a DataArray on the horizontal dims (None: 0, heights above the
    lowest valid level), a pressure that has only the vertical dim is isobaric data."""
    g = _Grid(temperature, vert_dim)
    res = _device(_api.hydrostatic, g.values(pressure), g.values(temperature), g.per_col(dewpoint), g.per_col(specific_humidity),
                  g.per_col(base_height), layers=layers, want=want)
    out = {}
    if 'height' in res:
        out['height'] = g.vert(res['height'], 'height', _ATTRS['height'])
    if res.get('thickness'):                             # (without layers: no variable)
        th = np.stack([_host(x) for x in res['thickness']])
        out['thickness'] = g.vert(th, 'thickness', _ATTRS['thickness'], vcoord=np.arange(len(th)), dim='hydrostatic_layer')
    if 'status' in res:
        out['status'] = g.horiz(res['status'], 'status', _ATTRS['status'])
    return Dataset(out)


def hydrostatic_height(pressure, temperature, dewpoint=None, specific_humidity=None, base_height=None, vert_dim=VERT):
    """The hydrostatic height [m] of every level on the dims of `temperature` (vertical first), with units and a long_name:
    base_height (None: 0) at each column's lowest valid level, NaN at invalid levels."""
    g = _Grid(temperature, vert_dim)
    res = _device(_api.hydrostatic_height, g.values(pressure), g.values(temperature), g.per_col(dewpoint),
                  g.per_col(specific_humidity), g.per_col(base_height))
    return g.vert(res, 'height', _ATTRS['height'])


def thickness_hydrostatic(pressure, temperature, dewpoint=None, specific_humidity=None, bottom=None, depth=None, vert_dim=VERT):
    """metpy.calc.thickness_hydrostatic [m] per column: from `bottom` [hPa; None: the lowest valid level] up `depth` [hPa; None:
    to the highest valid level].  The moisture is dewpoint or specific_humidity, not MetPy's mixing_ratio."""
    g = _Grid(temperature, vert_dim)
    res = _device(_api.thickness_hydrostatic, g.values(pressure), g.values(temperature), g.per_col(dewpoint),
                  g.per_col(specific_humidity), bottom=bottom, depth=depth)
    return g.horiz(res, 'thickness', _ATTRS['thickness'])


def _point(fn, x, name):
    res = _host(_device(fn, np.asarray(x.values) if isinstance(x, DataArray) else np.asarray(x, dtype=np.float64)))
    if isinstance(x, DataArray):
        return DataArray(res, dims=x.dims, coords=dict(x.coords), attrs=dict(_ATTRS[name]), name=name)
    return res


def geopotential_to_height(geopotential):
    """metpy.calc.geopotential_to_height per point: [m^2/s^2] -> [m], on the input's dims."""
    return _point(_api.geopotential_to_height, geopotential, 'geopotential_height')


def height_to_geopotential(height):
    """metpy.calc.height_to_geopotential per point: [m] -> [m^2/s^2], on the input's dims."""
    return _point(_api.height_to_geopotential, height, 'geopotential')
