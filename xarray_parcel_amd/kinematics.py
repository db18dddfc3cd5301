"""
Storm motion, helicity and the composites on DataArrays: metpy.calc.bunkers_storm_motion, storm_relative_helicity,
significant_tornado and supercell_composite for every column (or point) of a grid, what feeds the composites' effective
arguments -- the effective inflow layer and helicity / bulk wind difference between per-column bounds -- and the wind over
caller-chosen layers with what is built on it (mean_pressure_weighted, bulk_shear, critical_angle, corfidi_storm_motion, the
effective-layer significant tornado parameter) through libxparcel (numpy_api.bunkers_storm_motion, ...).  The reference has no counterparts, so this lives next to the mirror
(parcel_functions.py) rather than in it, and is built from the mirror's plumbing: a _Grid splits the inputs and wraps
the results, _device turns library errors into the mirror's.
"""
import numpy as np

from . import numpy_api as _api
from .parcel_functions import VERT, _Grid, _device, _moisture

_WIND = 'm s$^{-1}$'
_SRH = 'm$^{2}$ s$^{-2}$'
_ATTRS = {
    'bunkers_right_u': {'long_name': 'Bunkers right-mover storm motion, u component', 'units': _WIND},
    'bunkers_right_v': {'long_name': 'Bunkers right-mover storm motion, v component', 'units': _WIND},
    'bunkers_left_u': {'long_name': 'Bunkers left-mover storm motion, u component', 'units': _WIND},
    'bunkers_left_v': {'long_name': 'Bunkers left-mover storm motion, v component', 'units': _WIND},
    'mean_wind_u': {'long_name': 'Pressure-weighted 0-6 km mean wind, u component', 'units': _WIND},
    'mean_wind_v': {'long_name': 'Pressure-weighted 0-6 km mean wind, v component', 'units': _WIND},
    'positive_srh': {'long_name': 'Positive storm-relative helicity', 'units': _SRH},
    'negative_srh': {'long_name': 'Negative storm-relative helicity', 'units': _SRH},
    'total_srh': {'long_name': 'Storm-relative helicity', 'units': _SRH},
    'shear_u': {'long_name': 'Bulk wind difference over the layer, u component', 'units': _WIND},
    'shear_v': {'long_name': 'Bulk wind difference over the layer, v component', 'units': _WIND},
    'shear_magnitude': {'long_name': 'Bulk wind difference over the layer', 'units': _WIND},
    'base_pressure': {'long_name': 'Effective inflow layer base pressure', 'units': 'hPa'},
    'top_pressure': {'long_name': 'Effective inflow layer top pressure', 'units': 'hPa'},
    'base_height': {'long_name': 'Effective inflow layer base height above the lowest level', 'units': 'm'},
    'top_height': {'long_name': 'Effective inflow layer top height above the lowest level', 'units': 'm'},
    'base_index': {'long_name': 'Effective inflow layer base level index'},
    'top_index': {'long_name': 'Effective inflow layer top level index'},
    'status': {'long_name': 'Status bits'},
    'candidate_cape': {'long_name': 'CAPE of the parcel lifted from the level', 'units': 'J kg$^{-1}$'},
    'candidate_cin': {'long_name': 'CIN of the parcel lifted from the level', 'units': 'J kg$^{-1}$'},
    'significant_tornado': {'long_name': 'Significant tornado parameter', 'units': '1'},
    'supercell_composite': {'long_name': 'Supercell composite parameter', 'units': '1'},
    'layer_mean_wind_u': {'long_name': 'Pressure-weighted mean wind of the layer, u component', 'units': _WIND},
    'layer_mean_wind_v': {'long_name': 'Pressure-weighted mean wind of the layer, v component', 'units': _WIND},
    'bulk_shear_u': {'long_name': 'Bulk shear over the layer (bounds in ln p), u component', 'units': _WIND},
    'bulk_shear_v': {'long_name': 'Bulk shear over the layer (bounds in ln p), v component', 'units': _WIND},
    'layer_bottom_wind_u': {'long_name': 'Wind at the bottom of the layer, u component', 'units': _WIND},
    'layer_bottom_wind_v': {'long_name': 'Wind at the bottom of the layer, v component', 'units': _WIND},
    'max_wind_u': {'long_name': 'Strongest wind of the layer, u component', 'units': _WIND},
    'max_wind_v': {'long_name': 'Strongest wind of the layer, v component', 'units': _WIND},
    'max_wind_pressure': {'long_name': 'Pressure of the strongest wind of the layer', 'units': 'hPa'},
    'critical_angle': {'long_name': 'Critical angle', 'units': 'degrees'},
    'corfidi_upwind_u': {'long_name': 'Corfidi upwind-propagating MCS motion, u component', 'units': _WIND},
    'corfidi_upwind_v': {'long_name': 'Corfidi upwind-propagating MCS motion, v component', 'units': _WIND},
    'corfidi_downwind_u': {'long_name': 'Corfidi downwind-propagating MCS motion, u component', 'units': _WIND},
    'corfidi_downwind_v': {'long_name': 'Corfidi downwind-propagating MCS motion, v component', 'units': _WIND},
    'significant_tornado_effective': {'long_name': 'Significant tornado parameter (effective layer)', 'units': '1'},
}
_BUNKERS = {'right_u': 'bunkers_right_u', 'right_v': 'bunkers_right_v', 'left_u': 'bunkers_left_u',
            'left_v': 'bunkers_left_v', 'mean_u': 'mean_wind_u', 'mean_v': 'mean_wind_v'}
_SRH_NAMES = {'positive': 'positive_srh', 'negative': 'negative_srh', 'total': 'total_srh'}
_LAYER_NAMES = dict(_SRH_NAMES, shear_u='shear_u', shear_v='shear_v', shear_magnitude='shear_magnitude')
_WIND_LAYERS = {'mean_u': 'layer_mean_wind_u', 'mean_v': 'layer_mean_wind_v', 'shear_u': 'bulk_shear_u', 'shear_v': 'bulk_shear_v',
                'bottom_u': 'layer_bottom_wind_u', 'bottom_v': 'layer_bottom_wind_v', 'max_u': 'max_wind_u',
                'max_v': 'max_wind_v', 'max_pressure': 'max_wind_pressure'}
_CORFIDI = {k: 'corfidi_' + k for k in ('upwind_u', 'upwind_v', 'downwind_u', 'downwind_v')}
_EFFECTIVE = ('base_pressure', 'top_pressure', 'base_height', 'top_height', 'base_index', 'top_index', 'status')


def bunkers_storm_motion(pressure, u, v, height, vert_dim=VERT):
    """Bunkers right- and left-mover storm motion and the 0-6 km pressure-weighted mean wind of every column, from
    pressure [hPa], u, v [m/s] and height [m] on one vertical (pressure on the wind levels).  Returns a Dataset on the
    horizontal dims; columns that do not reach 6 km above their lowest level (MetPy raises) are NaN."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.bunkers_storm_motion, g.values(pressure), g.values(u), g.values(v), g.values(height))
    return g.dataset({name: res[k] for k, name in _BUNKERS.items()}, attrs=_ATTRS.get)


def storm_relative_helicity(height, u, v, depth, vert_dim=VERT, bottom=0.0, storm_u=0.0, storm_v=0.0, surface_u=None,
                            surface_v=None):
    """Positive, negative and total storm-relative helicity [m^2/s^2] of every column from `bottom` up `depth` metres
    above the lowest level (or, with surface_u / surface_v, above the surface, height being the height above it).
    storm_u / storm_v: scalars or DataArrays on the horizontal dims (e.g. bunkers_storm_motion's bunkers_right_u).  A
    sequence of up to four depths, computed in one pass, adds the leading dim 'srh_depth'.  Depths that the column does
    not span are NaN."""
    g = _Grid(height, vert_dim)
    res = _device(_api.storm_relative_helicity, g.values(height), g.values(u), g.values(v), depth, bottom=bottom,
                  storm_u=g.per_col(storm_u), storm_v=g.per_col(storm_v), surface_u=g.per_col(surface_u),
                  surface_v=g.per_col(surface_v))
    layered = {} if np.ndim(depth) == 0 else dict(vert=True, vcoord=np.asarray(depth, dtype=np.float64), dim='srh_depth')
    return g.dataset({name: res[k] for k, name in _SRH_NAMES.items()}, attrs=_ATTRS.get, **layered)


def effective_inflow_layer(pressure, temperature, dewpoint, height=None, vert_dim=VERT, cape_min=100.0, cin_min=-250.0,
                           search_depth=300.0, moist=None, want_candidates=False, **cape_cin_options):
    """The effective inflow layer (Thompson et al. 2007) of every column: the lowest contiguous run of levels whose lifted
    parcels have CAPE >= cape_min and CIN >= cin_min, searched over the lowest search_depth hPa.  Returns a Dataset on
    the horizontal dims: base / top pressure [hPa], height [m above the lowest valid level; NaN without `height`] and
    level index (-1: none), and the status bits; with want_candidates also candidate_cape / candidate_cin on the
    vertical (NaN where a level was not lifted).  Columns without a layer are NaN.  humidity='relative' (a fraction; percent
    is refused) or 'mixing_ratio' [kg/kg] among the options: what `dewpoint` holds."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.effective_inflow_layer, g.values(pressure), g.values(temperature),
                  _moisture(g, dewpoint, cape_cin_options),
                  g.per_col(height), cape_min=cape_min, cin_min=cin_min,
                  search_depth=search_depth, moist=moist, want_candidates=want_candidates, **cape_cin_options)
    out = g.dataset(res, _EFFECTIVE, _ATTRS.get)
    if want_candidates:
        for name in ('candidate_cape', 'candidate_cin'):
            out[name] = g.vert(res[name], name, _ATTRS[name])
    return out


def storm_relative_helicity_layers(height, u, v, bottom, top, vert_dim=VERT, storm_u=0.0, storm_v=0.0, surface_u=None,
                                   surface_v=None):
    """Storm-relative helicity [m^2/s^2] and the bulk wind difference [m/s] of every column between its OWN bounds:
    `bottom`, `top` [m] scalars or DataArrays on the horizontal dims, in storm_relative_helicity's height convention (what
    effective_inflow_layer returns as base_height / top_height).  A sequence of up to four tops that share the bottom,
    computed in one pass, adds the leading dim 'srh_layer'.  The wind difference is the wind at top minus the wind at
    bottom, each linear in height (not MetPy's ln p bulk_shear).  Layers that are not spanned, or whose bounds are NaN or
    inverted, are NaN."""
    g = _Grid(height, vert_dim)
    many = isinstance(top, (list, tuple))
    tops = [g.per_col(x) for x in top] if many else g.per_col(top)
    res = _device(_api.storm_relative_helicity_layers, g.values(height), g.values(u), g.values(v), g.per_col(bottom), tops,
                  storm_u=g.per_col(storm_u), storm_v=g.per_col(storm_v), surface_u=g.per_col(surface_u),
                  surface_v=g.per_col(surface_v))
    layered = dict(vert=True, vcoord=np.arange(len(top)), dim='srh_layer') if many else {}
    return g.dataset({name: res[k] for k, name in _LAYER_NAMES.items()}, attrs=_ATTRS.get, **layered)


def significant_tornado(sbcape, lcl_height, storm_helicity_1km, shear_6km):
    """Significant tornado parameter per point: sbcape [J/kg], LCL height [m], 0-1 km SRH [m^2/s^2], 0-6 km shear [m/s]."""
    g = _Grid(sbcape, None)
    out = _device(_api.significant_tornado, *(g.values(x) for x in (sbcape, lcl_height, storm_helicity_1km, shear_6km)))
    return g.horiz(out, 'significant_tornado', _ATTRS['significant_tornado'])


def supercell_composite(mucape, effective_storm_helicity, effective_shear):
    """Supercell composite parameter per point: mucape [J/kg], SRH [m^2/s^2], shear [m/s]."""
    g = _Grid(mucape, None)
    out = _device(_api.supercell_composite, *(g.values(x) for x in (mucape, effective_storm_helicity, effective_shear)))
    return g.horiz(out, 'supercell_composite', _ATTRS['supercell_composite'])


def wind_layers(pressure, u, v, height=None, layers=(), vert_dim=VERT):
    """The wind over up to four layers of every column in one pass: `layers` as in numpy_api.wind_layers -- {'bottom': 850,
    'top': 300} or {'depth': 100} in hPa, {'bottom_height': 0, 'top_height': 6000} in metres above the lowest valid level
    (needs `height`).  Returns a Dataset under the leading dim 'wind_layer' (the layer's index): the pressure-weighted mean
    wind, the ln p bulk shear, the wind at the bottom, the strongest wind and its pressure, and the per-column status.
    Layers that a column does not span are NaN."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.wind_layers, g.values(pressure), g.values(u), g.values(v), g.per_col(height), layers=layers)
    ds = g.dataset({name: res[k] for k, name in _WIND_LAYERS.items()}, attrs=_ATTRS.get, vert=True,
                   vcoord=np.arange(len(layers)), dim='wind_layer')
    ds['status'] = g.horiz(res['status'], 'status', _ATTRS['status'])
    return ds


def mean_pressure_weighted(pressure, u, v, height=None, bottom=None, depth=100.0, vert_dim=VERT):
    """metpy.calc.mean_pressure_weighted of the wind for every column, as a Dataset of layer_mean_wind_u / _v.  bottom,
    depth: metres (bottom above the lowest valid level) if `height` is given and `bottom` is not None, hPa otherwise
    (bottom=None: the lowest valid level) -- numpy_api.mean_pressure_weighted states the rule."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.mean_pressure_weighted, g.values(pressure), g.values(u), g.values(v), g.per_col(height), bottom=bottom,
                  depth=depth)
    return g.dataset(dict(zip(('layer_mean_wind_u', 'layer_mean_wind_v'), res)), attrs=_ATTRS.get)


def bulk_shear(pressure, u, v, height=None, bottom=None, depth=100.0, vert_dim=VERT):
    """metpy.calc.bulk_shear for every column, as a Dataset of bulk_shear_u / _v; bottom, depth as in mean_pressure_weighted."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.bulk_shear, g.values(pressure), g.values(u), g.values(v), g.per_col(height), bottom=bottom, depth=depth)
    return g.dataset(dict(zip(('bulk_shear_u', 'bulk_shear_v'), res)), attrs=_ATTRS.get)


def critical_angle(pressure, u, v, height, storm_u, storm_v, vert_dim=VERT):
    """metpy.calc.critical_angle [degrees] for every column: the angle between the 0-500 m bulk shear and the storm-relative
    inflow at the lowest valid level; storm_u / storm_v scalars or DataArrays on the horizontal dims."""
    g = _Grid(pressure, vert_dim)
    out = _device(_api.critical_angle, g.values(pressure), g.values(u), g.values(v), g.values(height), g.per_col(storm_u),
                  g.per_col(storm_v))
    return g.horiz(out, 'critical_angle', _ATTRS['critical_angle'])


def corfidi_storm_motion(pressure, u, v, llj_u=None, llj_v=None, vert_dim=VERT):
    """Corfidi upwind- and downwind-propagating MCS motion of every column, as a Dataset; the low-level jet (scalars or
    DataArrays on the horizontal dims, both or neither) defaults to the strongest wind at or below 850 hPa."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.corfidi_storm_motion, g.values(pressure), g.values(u), g.values(v), llj_u=g.per_col(llj_u),
                  llj_v=g.per_col(llj_v))
    return g.dataset({name: res[k] for k, name in _CORFIDI.items()}, attrs=_ATTRS.get)


def significant_tornado_effective(mlcape, mlcin, lcl_height, esrh, ebwd, base_height=None):
    """SPC's effective-layer significant tornado parameter per point; base_height: effective_inflow_layer's base_height
    (where it is > 0 the result is 0)."""
    g = _Grid(mlcape, None)
    args = [g.values(x) for x in (mlcape, mlcin, lcl_height, esrh, ebwd)]
    out = _device(_api.significant_tornado_effective, *args, base_height=g.per_col(base_height))
    return g.horiz(out, 'significant_tornado_effective', _ATTRS['significant_tornado_effective'])
