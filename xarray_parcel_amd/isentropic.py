"""
Isentropic interpolation on DataArrays: metpy.calc.isentropic_interpolation for every column of a grid through libxparcel
(numpy_api.isentropic_interpolation; include/xparcel.h has the rules and the deliberate differences from MetPy).
The reference has no counterpart, so this lives next to the mirror (parcel_functions.py) rather than in it, and is built
from the mirror's plumbing, as sounding_indices.py and thermo_layers.py.
"""
import numpy as np

from . import numpy_api as _api
from ._xr import Dataset
from .parcel_functions import VERT, _Grid, _device

LEVEL_DIM = 'isentropic_level'
_ATTRS = {
    'pressure': {'long_name': 'Pressure on the isentropic surface', 'units': 'hPa'},
    'temperature': {'long_name': 'Temperature on the isentropic surface', 'units': 'K'},
    'status': {'long_name': 'Status bits'},
}


def isentropic_interpolation(levels, pressure, temperature, *args, temperature_out=False, max_iters=50, eps=1e-6,
                             bottom_up_search=True, vert_dim=VERT):
    """pressure [hPa], temperature [K] and the further variables `args` on the surfaces of potential temperature `levels` [K],
    as a Dataset on the new leading dim 'isentropic_level' (the sorted levels its coordinate, in K) and the horizontal dims:
    'pressure', 'temperature' (with temperature_out), each arg under its own name ('var0', 'var1', ... where it has none, its
    attrs kept) and the horizontal 'status'.  Arguments as numpy_api.isentropic_interpolation; a pressure that has only the
    vertical dim is isobaric data."""
    g = _Grid(temperature, vert_dim)
    lev = np.sort(np.asarray(levels, dtype=np.float64).reshape(-1))
    res = _device(_api.isentropic_interpolation, lev, g.values(pressure), g.values(temperature), *[g.values(a) for a in args],
                  temperature_out=temperature_out, max_iters=max_iters, eps=eps, bottom_up_search=bottom_up_search, status=True)
    names = ['pressure'] + (['temperature'] if temperature_out else [])
    names += [getattr(a, 'name', None) or 'var%d' % i for i, a in enumerate(args)]
    assert len(set(names)) == len(names), 'the further variables need names of their own'
    attrs = dict(_ATTRS, **{k: dict(getattr(a, 'attrs', {})) for k, a in zip(names[len(names) - len(args):], args)})
    out = {k: g.vert(x, k, attrs[k], vcoord=lev, dim=LEVEL_DIM) for k, x in zip(names, res)}
    out['status'] = g.horiz(res[-1], 'status', _ATTRS['status'])
    return Dataset(out, attrs={'isentropic_level_units': 'K'})
