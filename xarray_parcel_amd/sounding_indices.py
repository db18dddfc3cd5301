"""
The classic sounding indices and the convective condensation level on DataArrays: MetPy's k_index, total_totals_index,
cross_totals, vertical_totals, showalter_index, sweat_index and ccl for every column of a grid through libxparcel
(numpy_api.sounding_indices), with the values at 850, 700 and 500 hPa interpolated in ln p where no level lies on the isobar.
The reference has no counterparts, so this lives next to the mirror (parcel_functions.py) rather than in it, and is built
from the mirror's plumbing, as kinematics.py and thermo_layers.py.
"""
from . import numpy_api as _api
from ._xr import Dataset
from .parcel_functions import VERT, _Grid, _device

_ATTRS = {
    'k_index': {'long_name': 'K index', 'units': 'K'},
    'total_totals': {'long_name': 'Total totals index', 'units': 'K'},
    'cross_totals': {'long_name': 'Cross totals index', 'units': 'K'},
    'vertical_totals': {'long_name': 'Vertical totals index', 'units': 'K'},
    'showalter_index': {'long_name': 'Showalter index', 'units': 'K'},
    'sweat_index': {'long_name': 'Severe weather threat index', 'units': '1'},
    'ccl_pressure': {'long_name': 'Pressure of the convective condensation level', 'units': 'hPa'},
    'ccl_temperature': {'long_name': 'Temperature of the convective condensation level', 'units': 'K'},
    'convective_temperature': {'long_name': 'Convective temperature', 'units': 'K'},
    'status': {'long_name': 'Status bits'},
}


def sounding_indices(pressure, temperature, dewpoint, u=None, v=None, moist=None, which='top', mixed_layer_depth=None,
                     want=None, vert_dim=VERT):
    """Every index and the CCL of every column in one pass, as a Dataset on the horizontal dims: k_index, total_totals,
    cross_totals, vertical_totals, showalter_index [K], sweat_index (with u, v [m/s]), ccl_pressure [hPa], ccl_temperature,
    convective_temperature [K] -- those that `want` names, by default all the inputs allow -- and the per-column status.
    Arguments as numpy_api.sounding_indices."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.sounding_indices, g.values(pressure), g.values(temperature), g.values(dewpoint), g.per_col(u), g.per_col(v),
                  moist=moist, which=which, mixed_layer_depth=mixed_layer_depth, want=want)
    return g.dataset(res, attrs=_ATTRS.get)


def _one(key, pressure, temperature, dewpoint, vert_dim, u=None, v=None, **kwargs):
    return sounding_indices(pressure, temperature, dewpoint, u, v, want=(key,), vert_dim=vert_dim, **kwargs)[key]


def k_index(pressure, temperature, dewpoint, vert_dim=VERT):
    """metpy.calc.k_index [K] of every column."""
    return _one('k_index', pressure, temperature, dewpoint, vert_dim)


def total_totals_index(pressure, temperature, dewpoint, vert_dim=VERT):
    """metpy.calc.total_totals_index [K] of every column."""
    return _one('total_totals', pressure, temperature, dewpoint, vert_dim)


def cross_totals(pressure, temperature, dewpoint, vert_dim=VERT):
    """metpy.calc.cross_totals [K] of every column."""
    return _one('cross_totals', pressure, temperature, dewpoint, vert_dim)


def vertical_totals(pressure, temperature, dewpoint=None, vert_dim=VERT):
    """metpy.calc.vertical_totals [K] of every column (without a dewpoint the temperature decides which levels are valid)."""
    return _one('vertical_totals', pressure, temperature, temperature if dewpoint is None else dewpoint, vert_dim)


def showalter_index(pressure, temperature, dewpoint, moist=None, vert_dim=VERT):
    """metpy.calc.showalter_index [K] of every column."""
    return _one('showalter_index', pressure, temperature, dewpoint, vert_dim, moist=moist)


def sweat_index(pressure, temperature, dewpoint, u, v, vert_dim=VERT):
    """metpy.calc.sweat_index of every column, from u, v [m/s]."""
    return _one('sweat_index', pressure, temperature, dewpoint, vert_dim, u, v)


def ccl(pressure, temperature, dewpoint, mixed_layer_depth=None, which='top', vert_dim=VERT):
    """metpy.calc.ccl of every column, as a Dataset of ccl_pressure [hPa], ccl_temperature and convective_temperature [K]."""
    res = sounding_indices(pressure, temperature, dewpoint, which=which, mixed_layer_depth=mixed_layer_depth,
                           want=_api.L.SOUNDING_CCL_OUT, vert_dim=vert_dim)
    return Dataset({k: res[k] for k in _api.L.SOUNDING_CCL_OUT})
