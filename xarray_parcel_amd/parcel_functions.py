"""
xarray-facing mirror of the hot path of traupach/xarray_parcel's modules/parcel_functions.py ("pf.py").

Same function names, argument names, defaults, return structure, attrs and assert messages as the
reference; the bodies hand the arrays to libxparcel (HIP, MI355X) through numpy_api.  Only the path named by
BASELINE.json is here: the drivers, the column algorithms they use, and the table loader.  DataArrays may be
xarray's (when installed) or the small stand-in of _xr.py.

Arrays are moved to (vert_dim, ...) order, flattened to columns and sent to the GPU; dask-backed inputs are
loaded by `.values` (the vertical must be one chunk in the reference too, pf.py:564).  Every function reads as
three steps: split its inputs with a _Grid, call the library through _device, wrap the results with the same _Grid.
"""
import numpy as np

from . import numpy_api as _api
from ._lib import XP_E_NO_TABLES, XParcelError
from ._xr import DataArray, Dataset

VERT = 'model_level_number'


# -- DataArray plumbing ---------------------------------------------------------------------------
def _values(x, dtype=np.float64):
    """The values of a DataArray (or x itself) as an array of `dtype`; dtype=None keeps theirs."""
    return np.asarray(getattr(x, 'values', x), dtype=dtype)


def _names(ds):
    return list(ds.data_vars) if hasattr(ds, 'data_vars') else list(ds.keys())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


class _Grid:
    """The grid of one call, taken from its leading DataArray (or the first variable of a Dataset that has `vert_dim`):
    the horizontal `dims` and their `coords`, and the vertical coordinate `vc` (None when there is no vertical, the
    index when it has no coordinate).  A leading input that is not a DataArray gives a grid without dims."""

    def __init__(self, x, vert_dim):
        self.vert_dim, self.dims, self.coords, self.vc = vert_dim, (), {}, None
        if isinstance(x, Dataset):
            x = next((x[k] for k in _names(x) if vert_dim in x[k].dims), None)
        if isinstance(x, DataArray):
            self.dims = tuple(d for d in x.dims if d != vert_dim)
            self.coords = {k: np.asarray(v) for k, v in x.coords.items() if k in self.dims}
            if vert_dim in x.dims:
                self.vc = (np.asarray(x.coords[vert_dim]) if vert_dim in x.coords else
                           np.arange(x.shape[x.dims.index(vert_dim)]))

    def values(self, x, dim=None):
        """x with `dim` (default: the vertical) first: a DataArray's values in their dtype, anything else as float64."""
        if not isinstance(x, DataArray):
            return np.asarray(x, dtype=np.float64)
        dim = self.vert_dim if dim is None else dim
        if dim in x.dims:
            x = x.transpose(dim, *(d for d in x.dims if d != dim))
        return np.asarray(x.values)

    def per_col(self, x):
        """An argument that may be absent, a scalar or a field: None and 0-d values as they are, anything else as values(x)."""
        return x if x is None or np.ndim(x) == 0 else self.values(x)

    def split(self, ds):
        """Dataset -> name -> values with the vertical first; variables without it are broadcast along it
        (xarray.broadcast)."""
        arrs = {k: self.values(ds[k]) for k in _names(ds)}
        shape = next((v.shape for v in arrs.values() if self.vc is not None and v.ndim == len(self.dims) + 1), None)
        return {k: (np.broadcast_to(v, shape) if shape is not None and v.shape != shape else v) for k, v in arrs.items()}

    def check_index(self, msg):
        if self.vc is not None and len(self.vc) > 1:
            assert np.all(np.abs(np.diff(self.vc)) == 1), msg

    def horiz(self, values, name=None, attrs=None):
        """A per-point result (NumPy array or torch tensor) on the horizontal dims."""
        return DataArray(_host(values), dims=self.dims, coords=self.coords, attrs=dict(attrs or {}), name=name)

    def vert(self, values, name=None, attrs=None, vcoord=None, dim=None):
        """A result with a vertical first: `dim` (default: the call's) labelled `vcoord` (default: `vc`)."""
        dim = self.vert_dim if dim is None else dim
        coords = {**self.coords, dim: self.vc if vcoord is None else vcoord}
        return DataArray(_host(values), dims=(dim,) + self.dims, coords=coords, attrs=dict(attrs or {}), name=name)

    def dataset(self, arrs, keys=None, attrs=None, vert=False, **kw):
        """Dataset of the results `arrs` (name -> array; only `keys` if given), each named by its key, with attrs(name)
        (default: none), per point or (vert=True) with a vertical (`kw` as for vert())."""
        wrap = self.vert if vert else self.horiz
        return Dataset({k: wrap(arrs[k], k, attrs(k) if attrs else None, **kw) for k in (keys or arrs)})


def _moisture(g, x, options):
    """g.values(x) for the moisture argument of a CAPE-family call with the keyword `options`.  humidity='relative' takes a
    fraction: a DataArray that says it holds percent is refused rather than read a hundred times too moist."""
    units = str(getattr(x, 'attrs', {}).get('units', '')).strip().lower()
    if options.get('humidity') == 'relative' and units in ('%', 'percent', 'percentage'):
        raise ValueError("humidity='relative' takes relative humidity as a fraction (1 = saturated), not in %r: "
                         "divide by 100 first" % x.attrs['units'])
    return g.values(x)


def _attrs_of(ds):
    """attrs(name) of the variables of an input Dataset."""
    return lambda k: getattr(ds[k], 'attrs', {}) if k in ds else {}


def _device(fn, *args, **kw):
    """fn(*args, **kw), a numpy_api call; the library's missing-tables error is the reference's assert (pf.py:60)."""
    try:
        return fn(*args, **kw)
    except XParcelError as e:
        if e.code == XP_E_NO_TABLES:
            raise AssertionError('Call load_moist_adiabat_lookups first.') from e
        raise


# -- attrs of the results --------------------------------------------------------------------------------------------
# By result name, or by 'function.name' where one name has different attrs in different functions; the bundles' mu_cape,
# mixed_100_lifted_index, ... take those of their suffix (_BUNDLE_SUFFIXES).  {fields} are filled from the call's arguments.
# The reference's quirks are verbatim (sic).
_SHIP_UNITS = 'J kg$^{-2}$ g K$^2$ km$^{-1}$ m s$^{-1}$'
_ATTRS = {
    'cape': {'long_name': 'Convective available potential energy', 'units': 'J kg$^{-1}$'},       # pf.py:1366-1368
    'cin': {'long_name': 'Convective inhibition', 'units': 'J kg$^{-1}$'},                          # pf.py:1383-1385
    'lcl_pressure': {'long_name': 'Lifting condensation level pressure', 'units': 'hPa'},            # pf.py:669-677
    'lcl_temperature': {'long_name': 'Lifting condensation level temperature', 'units': 'K'},
    'lcl_virtual_temperature': {'long_name': 'Lifting condensation level virtual temperature', 'units': 'K'},
    'el_pressure': {'long_name': 'Equilibrium level pressure', 'units': 'hPa'},                      # pf.py:1188-1196
    'el_temperature': {'long_name': 'Equilibrium level temperature', 'units': 'K'},
    'lfc_pressure': {'long_name': 'Level of free convection pressure', 'units': 'hPa'},
    'lfc_temperature': {'long_name': 'Level of free convection temperature', 'units': 'K'},
    'pressure': {'long_name': 'Pressure at LCL'},                                                    # pf.py:889-890 (sic)
    'temperature': {'long_name': 'Temperature at LCL', 'units': 'K'},
    'virtual_temperature': {'long_name': 'Virtual temperature', 'units': 'K'},
    'environment_temperature': {'long_name': 'Environment temperature', 'units': 'K'},               # pf.py:849-852
    'environment_dewpoint': {'long_name': 'Environment dewpoint', 'units': 'K'},
    'environment_virtual_temperature': {'long_name': 'Virtual temperature', 'units': 'K'},
    'most_unstable.pressure': {'long_name': 'Pressure'},
    'most_unstable.temperature': {'long_name': 'Temperature'},
    'most_unstable.dewpoint': {'long_name': 'Dewpoint'},
    'mixed_layer.pressure': {'long_name': 'Pressure'},
    'mixed_parcel.temperature': {'long_name': 'Mixed parcel temperature', 'units': 'K'},
    'mixed_parcel.dewpoint': {'long_name': 'Mixed-parcel dewpoint'},
    'dry_lapse': {'long_name': 'Dry lapse rate temperature', 'units': 'K'},
    'moist_lapse': {'long_name': 'Moist lapse rate temperature', 'units': 'K'},
    'parcel_profile.temperature': {'long_name': 'Lifted parcel temperature', 'units': 'K'},
    'add_lcl_to_profile.temperature': {'long_name': 'Temperature at LCL'},                          # pf.py:889-891 (sic)
    'add_lcl_to_profile.pressure': {'long_name': 'Pressure at LCL'},
    'add_lcl_to_profile.lcl_virtual_temperature': {'long name': 'Virtual temperature at LCL'},
    'wet_bulb_temperature': {'long_name': 'Wet bulb temperature', 'units': 'K'},
    'dewpoint': {'long_name': 'Dewpoint temperature', 'units': 'K'},
    'mixing_ratio': {'units': 'kg kg$^{-1}$'},
    'lifted_index': {'long_name': 'Lifted index', 'units': 'K'},
    'dci': {'long_name': 'Deep convective index', 'units': 'C'},
    'lapse_rate': {'long_name': 'Lapse rate', 'description': '{from_pressure}-{to_pressure} hPa lapse rate',
                   'units': 'K km$^{-1}$'},
    'lapse_rate_700_500': {'long_name': 'Lapse rate', 'description': '700-500 hPa lapse rate', 'units': 'K km$^{-1}$'},
    'isobar_temperature': {'description': 'Temperature at {isobar} hPa.', 'long_name': 'Isobar temperature', 'units': 'K'},
    'temp_500': {'description': 'Temperature at 500 hPa.', 'long_name': 'Isobar temperature', 'units': 'K'},
    'freezing_level': {'long_name': 'Freezing-level height', 'description': 'Height of zero degree dry-bulb temperature isotherm.',
                       'units': 'm'},
    'melting_level': {'long_name': 'Melting-level height', 'description': 'Height of zero degree wet-bulb temperature isotherm.',
                      'units': 'm'},
    'mu_mixing_ratio': {'long_name': 'Mixing ratio', 'description': 'Mixing ratio of most unstable parcel'},
    'wind_shear.shear_u': {'long_name': 'Surface to {shear_height} m wind shear, U component.', 'units': 'm s$^{-1}$'},
    'wind_shear.shear_v': {'long_name': 'Surface to {shear_height} m wind shear, V component.', 'units': 'm s$^{-1}$'},
    'wind_shear.shear_magnitude': {'long_name': 'Surface to {shear_height} m bulk wind shear.', 'units': 'm s$^{-1}$'},
    'wind_shear.positive_shear': {'long_name': 'True if {shear_height} wind > surface wind.'},
    'significant_hail_parameter': {'long_name': 'Significant hail parameter', 'units': _SHIP_UNITS},
    'ship': {'long_name': 'Significant hail parameter (SHIP)', 'units': _SHIP_UNITS},
    **{k: {'long_name': 'Proxy ' + label} for k, label in (
        ('proxy_Craven2004', 'Craven 2004'), ('proxy_Kunz2007', 'Kunz 2007'), ('proxy_Trapp2007', 'Trapp 2007'),
        ('proxy_Marsh2009', 'Marsh 2009'), ('proxy_Allen2011', 'Allen 2011'), ('proxy_Allen2014', 'Allen 2014'),
        ('proxy_Eccel2012', 'Eccel 2012'), ('proxy_Mohr2013', 'Mohr 2013'), ('proxy_SHIP_0.1', 'SHIP > 0.1'))},
}
_BUNDLE_SUFFIXES = ('cape', 'cin', 'lifted_index', 'dci')
_PROFILE_KEYS = ('pressure', 'temperature', 'virtual_temperature', 'environment_temperature',
                 'environment_virtual_temperature', 'environment_dewpoint')
_LFC_KEYS = ('lfc_pressure', 'lfc_temperature', 'el_pressure', 'el_temperature')
_LCL_KEYS = ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature')
_PARCEL_KEYS = ('pressure', 'temperature', 'dewpoint')


def _attrs(key, **fields):
    """A copy of the attrs of result `key` ({} if it has none), its {fields} filled."""
    out = dict(_ATTRS.get(key, {}))
    for f, v in fields.items():
        out = {k: a.replace('{%s}' % f, str(v)) for k, a in out.items()}
    return out


def _bundle_attrs(key):
    return _attrs(next((s for s in _BUNDLE_SUFFIXES if key.endswith('_' + s)), key))


# -- which moist adiabat a call uses --------------------------------------------------------------------
# The reference has ONE moist_lapse: the lookup-table one (pf.py:525-607), and every call of it starts with
# lookup_tables_loaded() (pf.py:554, 56-61).  So here: unless the caller names a mode (`moist=` keyword, an extension
# of this mirror) or has switched the module default with set_moist_lapse(), every function that lifts a parcel
# moist-adiabatically uses the tables handed over by load_moist_adiabat_lookups() and raises the reference's
# 'Call load_moist_adiabat_lookups first.' when there are none.  set_moist_lapse('exact') is the counterpart of what
# the reference's own known-answer tests do (`parcel.moist_lapse = tests.metpy_moist_lapse`,
# parcel_functions_demo.ipynb cell 33, unit_tests.py:114-140): MetPy's ODE instead of the tables.
_MOIST = {'override': None}


def set_moist_lapse(mode=None):
    """Module-wide moist-adiabat mode: None (the reference's behaviour: lookup tables), 'exact' (MetPy's ODE by RK4),
    'family' (the same ODE from the adiabat-family table) or 'table'."""
    assert mode is None or mode in _api.L.MOIST, "mode must be None, 'exact', 'family' or 'table'"
    _MOIST['override'] = mode


def _moist_mode(moist=None):
    if moist is not None:
        return moist
    if _MOIST['override'] is not None:
        return _MOIST['override']
    lookup_tables_loaded()                                                               # pf.py:554
    return 'table'


def _run(pressure, temperature, dewpoint, vert_dim, parcel, depth=None, parcel_values=None, trim=False, parcel_attrs=None,
         **kwargs):
    """The drivers: (cape / cin Dataset, profile Dataset, the parcel as a Dataset with attrs parcel_attrs(name))."""
    kwargs['moist'] = _moist_mode(kwargs.get('moist'))
    g = _Grid(pressure, vert_dim)
    p, t, td = g.values(pressure), g.values(temperature), _moisture(g, dewpoint, kwargs)
    g.check_index('Vert_dim index increments must all be 1.')                          # pf.py:957
    res = _device(_api.cape_cin_columns, p, t, td, parcel=parcel, depth=depth, parcel_values=parcel_values,
                  want_profile=True, **kwargs)
    vtc = kwargs.get('virtual_temperature_correction', True)
    cc = g.dataset(res, ('cape', 'cin'), _attrs)
    cc.attrs = {'correction': ('Virtual temperature correction used in CAPE/CIN calculations.' if vtc else
                               'Virtual temperature correction not used in CAPE/CIN calculations.')}  # pf.py:1453, 1472
    prof = {k: _host(res['profile'][k]) for k in _PROFILE_KEYS}
    nrow = prof['pressure'].shape[0]
    if trim:
        # the reference drops levels that are NaN in every column (pf.py:1552, 1637): trim the NaN padding
        while nrow > 1 and np.all(np.isnan(prof['pressure'][nrow - 1])):
            nrow -= 1
    vcoord = np.arange(nrow) + (g.vc[0] if g.vc is not None else 0)  # re-indexed vertical coordinate (pf.py:875)
    profile = g.dataset({k: v[:nrow] for k, v in prof.items()}, attrs=_attrs, vert=True, vcoord=vcoord)
    for k in _LCL_KEYS + _LFC_KEYS:
        profile[k] = g.horiz(res[k], k, _attrs(k))
    return cc, profile, g.dataset({k: res['parcel_' + k] for k in _PARCEL_KEYS}, attrs=parcel_attrs)


def _prefix(res, prefix):
    if prefix is not None:
        res = res.rename({'cape': prefix + '_cape', 'cin': prefix + '_cin'})              # pf.py:1510-1512
    return res


# -- drivers ------------------------------------------------------------------------------------------
def cape_cin(pressure, temperature, dewpoint, parcel_temperature, parcel_pressure, parcel_dewpoint,
             vert_dim=VERT, virtual_temperature_correction=True, lcl_interp='log', **kwargs):
    """pf.py:1394.  Returns (Dataset{cape, cin}, profile Dataset merged with LFC/EL)."""
    pv = tuple(_values(x) for x in (parcel_pressure, parcel_temperature, parcel_dewpoint))
    cc, profile, _ = _run(pressure, temperature, dewpoint, vert_dim, 'explicit', parcel_values=pv,
                          virtual_temperature_correction=virtual_temperature_correction, lcl_interp=lcl_interp,
                          **kwargs)
    return cc, profile


def surface_based_cape_cin(pressure, temperature, dewpoint, vert_dim=VERT, prefix=None, **kwargs):
    """pf.py:1477."""
    res, profile, _ = _run(pressure, temperature, dewpoint, vert_dim, 'surface', **kwargs)
    res.cape.attrs['description'] = 'CAPE for surface-based parcel.'                   # pf.py:1508-1509
    res.cin.attrs['description'] = 'CIN for surface-based parcel.'
    return _prefix(res, prefix), profile


def _named(pressure, temperature, dewpoint):
    assert getattr(pressure, 'name', None) == 'pressure', 'Pressure requires name pressure.'              # pf.py:1538
    assert getattr(temperature, 'name', None) == 'temperature', 'Temperature requires name temperature.'   # pf.py:1539
    assert getattr(dewpoint, 'name', None) == 'dewpoint', 'Dewpoint requires name dewpoint.'              # pf.py:1541


def most_unstable_cape_cin(pressure, temperature, dewpoint, vert_dim=VERT, depth=300, prefix=None, **kwargs):
    """pf.py:1557.  Returns (cape/cin, profile, most-unstable parcel)."""
    _named(pressure, temperature, dewpoint)
    res, profile, layer = _run(pressure, temperature, dewpoint, vert_dim, 'most_unstable', depth=depth, trim=True,
                               parcel_attrs=lambda k: _attrs('most_unstable.' + k), **kwargs)
    desc = f'most-unstable parcel in lowest {depth} hPa.'
    res.cape.attrs['description'] = f'CAPE for {desc}'
    res.cin.attrs['description'] = f'CIN for {desc}'
    return _prefix(res, prefix), profile, layer


def _mixed_attrs(k):
    return _attrs('mixed_layer.' + k) if k == 'pressure' else _attrs('mixed_parcel.' + k)


def mixed_layer_cape_cin(pressure, temperature, dewpoint, vert_dim=VERT, depth=100, prefix=None, **kwargs):
    """pf.py:1651.  Returns (cape/cin, profile, mixed parcel)."""
    _named(pressure, temperature, dewpoint)
    res, profile, mp = _run(pressure, temperature, dewpoint, vert_dim, 'mixed_layer', depth=depth, trim=True,
                            parcel_attrs=_mixed_attrs, **kwargs)
    desc = f'fully-mixed lowest {depth} hPa parcel'
    res.cape.attrs['description'] = f'CAPE for {desc}.'
    res.cin.attrs['description'] = f'CIN for {desc}'
    return _prefix(res, prefix), profile, mp


# -- column algorithms -----------------------------------------------------------------------------------
def lcl(parcel_pressure, parcel_temperature, parcel_dewpoint):
    """pf.py:609.  Dataset with lcl_pressure, lcl_temperature, lcl_virtual_temperature."""
    g = _Grid(parcel_pressure, None)
    p, t, td = np.broadcast_arrays(*map(g.values, (parcel_pressure, parcel_temperature, parcel_dewpoint)))
    r = _device(_api.lcl, p, t, td)
    return g.dataset({k: _host(r[k]).reshape(p.shape) for k in _LCL_KEYS}, attrs=_attrs)


def dry_lapse(pressure, parcel_temperature, parcel_pressure=None, vert_dim=VERT):
    """pf.py:291."""
    g = _Grid(pressure, vert_dim)
    pp = None if parcel_pressure is None else _values(parcel_pressure, None)
    return g.vert(_device(_api.dry_lapse, g.values(pressure), _values(parcel_temperature), pp), attrs=_attrs('dry_lapse'))


def moist_lapse(pressure, parcel_temperature, parcel_pressure=None, vert_dim=VERT, persist=True, moist=None):
    """pf.py:525: the reference's table lookup (needs load_moist_adiabat_lookups() first, pf.py:554); `moist='exact'`
    / `'family'` or set_moist_lapse() select the ODE instead (an extension of this mirror)."""
    moist = _moist_mode(moist)
    g = _Grid(pressure, vert_dim)
    pp = None if parcel_pressure is None else _values(parcel_pressure, None)
    return g.vert(_device(_api.moist_lapse, g.values(pressure), _values(parcel_temperature), pp, moist=moist),
                  attrs=_attrs('moist_lapse'))


def parcel_profile(pressure, parcel_pressure, parcel_temperature, parcel_dewpoint, vert_dim=VERT, moist=None):
    """pf.py:712."""
    moist = _moist_mode(moist)
    g = _Grid(pressure, vert_dim)
    p = g.values(pressure)
    r = _device(_api.parcel_profile, p, *map(_values, (parcel_pressure, parcel_temperature, parcel_dewpoint)), moist=moist)
    out = Dataset()
    out['pressure'] = g.vert(p, 'pressure')
    out['temperature'] = g.vert(r['temperature'], 'temperature', _attrs('parcel_profile.temperature'))
    out['virtual_temperature'] = g.vert(r['virtual_temperature'], 'virtual_temperature', _attrs('virtual_temperature'))
    for k in _LCL_KEYS:
        out[k] = g.horiz(r[k], k, _attrs(k))
    return out


def parcel_profile_with_lcl(pressure, temperature, dewpoint, parcel_pressure, parcel_temperature, parcel_dewpoint,
                            vert_dim=VERT, lcl_interp='log', moist=None):
    """pf.py:806."""
    pv = tuple(_values(x) for x in (parcel_pressure, parcel_temperature, parcel_dewpoint))
    _, profile, _ = _run(pressure, temperature, dewpoint, vert_dim, 'explicit', parcel_values=pv,
                         lcl_interp=lcl_interp, moist=moist)
    return Dataset({k: profile[k] for k in _PROFILE_KEYS + _LCL_KEYS})


def lfc_el(pressure, parcel_temperature, temperature, lcl_pressure, lcl_temperature, vert_dim=VERT):
    """pf.py:1066."""
    g = _Grid(pressure, vert_dim)
    g.check_index('Index increments must all be 1.')                                      # pf.py:1012
    r = _device(_api.lfc_el, *map(g.values, (pressure, parcel_temperature, temperature)),
                _values(lcl_pressure, None), _values(lcl_temperature, None))
    return g.dataset(r, _LFC_KEYS, _attrs)


def cape_cin_base(pressure, temperature, lfc_pressure, el_pressure, parcel_temperature, vert_dim=VERT,
                  pos_cape_neg_cin=True, post_zero_cin=False, **kwargs):
    """pf.py:1291."""
    g = _Grid(pressure, vert_dim)
    g.check_index('Index increments must all be 1.')                                      # pf.py:1221
    r = _device(_api.cape_cin_base, g.values(pressure), g.values(temperature), _values(lfc_pressure, None),
                _values(el_pressure, None), g.values(parcel_temperature), pos_cape_neg_cin=pos_cape_neg_cin,
                post_zero_cin=post_zero_cin)
    res = g.dataset(r, ('cape', 'cin'), _attrs)
    res.attrs = []                                                                          # pf.py:1391
    return res


def most_unstable_parcel(dat, depth=300, vert_dim=VERT):
    """pf.py:102: dat = Dataset with pressure, temperature, dewpoint."""
    g = _Grid(dat['pressure'], vert_dim)
    r = _device(_api.most_unstable_parcel, *(g.values(dat[k]) for k in _PARCEL_KEYS), depth=depth)
    return g.dataset(r, _PARCEL_KEYS, _attrs_of(dat))


def mixed_parcel(pressure, temperature, dewpoint, depth=100, vert_dim=VERT):
    """pf.py:229."""
    assert getattr(pressure, 'name', 'pressure') is not None, 'pressure requires name pressure.'   # pf.py:263
    g = _Grid(pressure, vert_dim)
    r = _device(_api.mixed_parcel, *map(g.values, (pressure, temperature, dewpoint)), depth=depth)
    return g.dataset(r, _PARCEL_KEYS, lambda k: _attrs('mixed_parcel.' + k))


def mixed_layer(dat, depth=100, vert_dim=VERT):
    """pf.py:137: dat = Dataset with pressure and the variables to mix."""
    g = _Grid(dat['pressure'], vert_dim)
    arrs = {k: g.values(dat[k]) for k in ['pressure'] + [k for k in dat.keys() if k != 'pressure']}
    return g.dataset(_device(_api.mixed_layer, arrs, depth=depth))


# -- SURVEY 8(f) items on the same kernels ------------------------------------------------------------------------
def wet_bulb_temperature(pressure, temperature, dewpoint, vert_dim=VERT, moist=None):
    """pf.py:389 (Normand's rule; its descent is a moist_lapse call, pf.py:436)."""
    moist = _moist_mode(moist)
    g = _Grid(pressure, vert_dim)
    p = g.values(pressure)
    out = _host(_device(_api.wet_bulb_temperature, p, g.values(temperature), g.values(dewpoint), moist=moist))
    if g.vc is None:
        return g.horiz(out.reshape(p.shape), 'wet_bulb_temperature', _attrs('wet_bulb_temperature'))
    return g.vert(out, 'wet_bulb_temperature', _attrs('wet_bulb_temperature'))


def _interp(x, coords, at, dim, log, keep_attrs=True):
    g = _Grid(coords, dim)
    cv, atv = g.values(coords), _values(at, None)

    def one(v):
        return g.horiz(_device(_api.interp_level, cv, g.values(v), atv, log=log), getattr(v, 'name', None),
                       getattr(v, 'attrs', {}) if keep_attrs else {})
    if isinstance(x, Dataset):                                      # every variable of the dataset (pf.py:82, 896, 901)
        return Dataset({k: one(x[k]) for k in _names(x)})
    return one(x)


def log_interp(x, coords, at, dim=VERT):
    """pf.py:1813: `x` a DataArray or a Dataset."""
    return _interp(x, coords, at, dim, log=True)


def linear_interp(x, coords, at, dim=VERT, keep_attrs=True, extrapolate=False):
    """pf.py:1758 (extrapolate=False only): `x` a DataArray or a Dataset."""
    assert not extrapolate, 'extrapolation is not part of the MI355X path'
    return _interp(x, coords, at, dim, log=False, keep_attrs=keep_attrs)


def _index(g, values, base, description, prefix):
    """lifted_index / deep_convective_index: a Dataset with the one variable `base` or prefix_base."""
    attrs = _attrs(base)
    if description is not None:
        attrs['description'] = description
    name = base if prefix is None else prefix + '_' + base
    return Dataset({name: g.horiz(values, name, attrs)})


def lifted_index(profile, vert_dim=VERT, description=None, prefix=None):
    """pf.py:1722."""
    g = _Grid(profile['pressure'], vert_dim)
    prof = {k: g.values(profile[k]) for k in ('pressure', 'temperature', 'environment_temperature')}
    return _index(g, _device(_api.lifted_index, prof), 'lifted_index', description, prefix)


def mixing_ratio(temperature, dewpoint, pressure):
    """pf.py:684."""
    if not isinstance(temperature, DataArray):
        return _host(_device(_api.mixing_ratio, temperature, dewpoint, pressure))
    out = _device(_api.mixing_ratio, *(_values(x, None) for x in (temperature, dewpoint, pressure)))
    return DataArray(_host(out), dims=temperature.dims, coords=temperature.coords, attrs=_attrs('mixing_ratio'))


def virtual_temperature(temperature, mixing_ratio, epsilon=0.608):
    """pf.py:782."""
    res = temperature * (1 + epsilon * mixing_ratio)
    if isinstance(res, DataArray):
        res.attrs['units'] = 'K'
        res.attrs['long_name'] = 'Virtual temperature'
    return res


def wet_bulb_temperature_fast(temperature, dewpoint):
    """pf.py:364: "1/3 rule" estimate (array arithmetic on the DataArrays, as in the reference)."""
    wb = temperature - (1 / 3) * (temperature - dewpoint)
    wb.name = 'wet_bulb_temperature'
    wb.attrs['long_name'] = 'Wet bulb temperature'
    wb.attrs['description'] = 'Estimated using 1/3 method.'
    wb.attrs['units'] = 'K'
    return wb


def deep_convective_index(pressure, temperature, dewpoint, lifted_index, vert_dim=VERT, description=None, prefix=None):
    """pf.py:1830 (Kunz 2009): T + Td at 850 hPa [deg C] minus the lifted index."""
    g = _Grid(pressure, vert_dim)
    dci = _device(_api.deep_convective_index, *map(g.values, (pressure, temperature, dewpoint, lifted_index)))
    return _index(g, dci, 'dci', description, prefix)


def lapse_rate(pressure, temperature, height, from_pressure=700, to_pressure=500, vert_dim=VERT):
    """pf.py:2102: observed lapse rate between two pressure levels [K/km]."""
    g = _Grid(pressure, vert_dim)
    out = _device(_api.lapse_rate, *map(g.values, (pressure, temperature, height)), from_pressure=from_pressure,
                  to_pressure=to_pressure)
    return g.horiz(out, attrs=_attrs('lapse_rate', from_pressure=from_pressure, to_pressure=to_pressure))


def freezing_level_height(temperature, height, vert_dim=VERT):
    """pf.py:2137: height of the lowest 273.15 K crossing of the temperature profile."""
    g = _Grid(temperature, vert_dim)
    g.check_index('Index increments must all be 1.')                                    # pf.py:1011
    out = _device(_api.freezing_level_height, g.values(temperature), g.values(height))
    return g.horiz(out, 'freezing_level', _attrs('freezing_level'))


def melting_level_height(pressure, temperature, dewpoint, height, fast=True, vert_dim=VERT, moist=None):
    """pf.py:2160: freezing level of the wet-bulb temperature; returns (melting level, wet bulb)."""
    if fast:
        wb = wet_bulb_temperature_fast(temperature=temperature, dewpoint=dewpoint)
    else:
        wb = wet_bulb_temperature(pressure=pressure, temperature=temperature, dewpoint=dewpoint, vert_dim=vert_dim,
                                  moist=moist)
    mlh = freezing_level_height(temperature=wb, height=height, vert_dim=vert_dim)
    mlh.attrs['long_name'] = 'Melting-level height'
    mlh.attrs['description'] = 'Height of zero degree wet-bulb temperature isotherm.'
    mlh.name = 'melting_level'
    return mlh, wb


def isobar_temperature(pressure, temperature, isobar, vert_dim=VERT):
    """pf.py:2193."""
    g = _Grid(pressure, vert_dim)
    out = _device(_api.isobar_temperature, g.values(pressure), g.values(temperature), isobar)
    return g.horiz(out, attrs=_attrs('isobar_temperature', isobar=isobar))


def dewpoint_from_specific_humidity(pressure, temperature, specific_humidity, vert_dim=VERT):
    """metpy.calc.dewpoint_from_specific_humidity (MetPy 1.4.1 chain) as the reference's harness and products call it
    (parcel_test.py:262-266, pf.py:1889-1894), result in K."""
    g = _Grid(pressure, vert_dim)
    p = g.values(pressure)
    out = _host(_device(_api.dewpoint_from_specific_humidity, p, g.values(temperature), g.values(specific_humidity)))
    if g.vc is None:
        return g.horiz(out.reshape(p.shape), 'dewpoint', _attrs('dewpoint'))
    return g.vert(out, 'dewpoint', _attrs('dewpoint'))


# -- product bundle (pf.py:1951-2100, 2216-2407) ------------------------------------------------------------------------
def wind_shear(surface_wind_u, surface_wind_v, wind_u, wind_v, height, shear_height=6000, vert_dim=VERT):
    """pf.py:2216: Dataset with shear_u, shear_v, shear_magnitude [m/s] and positive_shear."""
    g = _Grid(height, vert_dim)
    r = _device(_api.wind_shear, *map(g.values, (surface_wind_u, surface_wind_v, wind_u, wind_v, height)),
                shear_height=shear_height)
    return g.dataset(r, attrs=lambda k: _attrs('wind_shear.' + k, shear_height=shear_height))


def significant_hail_parameter(mucape, mixing_ratio, lapse, temp_500, shear, flh):
    """pf.py:2261 (SHIP)."""
    ship = _device(_api.significant_hail_parameter, *map(_values, (mucape, mixing_ratio, lapse, temp_500, shear, flh)))
    ref = mucape if isinstance(mucape, DataArray) else None
    return DataArray(ship, dims=ref.dims if ref is not None else None, coords=ref.coords if ref is not None else None,
                     attrs=_attrs('significant_hail_parameter'))


def valid_data(dat, vert_dim):
    """pf.py:2308."""
    vc = _values(dat[vert_dim], None)
    assert np.all(np.abs(np.diff(vc)) == 1), 'Index increments must all be 1.'
    p = _Grid(dat['pressure'], vert_dim).values(dat['pressure'])
    assert np.nanmax(np.diff(p, axis=0)) < 0, 'Pressures must decrease with increasing level number.'
    return True


def conv_properties(dat, vert_dim=VERT, ignore_nans=False, moist=None):
    """pf.py:1951: the convective-property bundle.  `dat` holds pressure, temperature, specific_humidity, height_asl on
    `vert_dim`, wind_u, wind_v, wind_height_above_surface on their own vertical, surface_wind_u, surface_wind_v."""
    return _bundle(dat, vert_dim, _api.conv_properties, ignore_nans=ignore_nans, moist=_moist_mode(moist))


def _bundle(dat, vert_dim, fn, **kw):
    g = _Grid(dat['pressure'], vert_dim)
    wdim = [d for d in dat['wind_u'].dims if d not in g.dims][0]
    arrs = {k: g.values(dat[k], wdim if k.startswith('wind_') else None) for k in
            ('pressure', 'temperature', 'specific_humidity', 'height_asl', 'wind_u', 'wind_v', 'wind_height_above_surface',
             'surface_wind_u', 'surface_wind_v')}
    return g.dataset(_device(fn, arrs, **kw), attrs=_bundle_attrs)


def min_conv_properties(dat, vert_dim=VERT, moist=None):
    """pf.py:1873: the minimal property set (mixed-layer CAPE/CIN + lifted index, lapse rate, T500, freezing / melting
    level, 0-6 km shear)."""
    return _bundle(dat, vert_dim, _api.min_conv_properties, moist=_moist_mode(moist))


def storm_proxies(dat):
    """pf.py:2323: proxies (booleans) and SHIP from the Dataset returned by conv_properties()."""
    ref = dat['mu_cape']
    r = _device(_api.storm_proxies, {k: _values(dat[k], None) for k in dat.keys()})
    return Dataset({k: DataArray(np.asarray(v), dims=ref.dims, coords=ref.coords, attrs=_attrs(k), name=k)
                    for k, v in r.items()})



# -- the reference's array primitives ------------------------------------------------------------------------------------
# (the CAPE / CIN kernels do not use them -- they stream a column once -- but callers of the reference can)
def round_to(x, to, dp=2):
    """pf.py:358."""
    return np.round(np.round(x / to) * to, dp)


def interp1d_numba(at, xp, fp, out=None):
    """pf.py:23: numpy.interp along the LAST axis of each argument (the reference's gufunc signature
    (m),(n),(n)->(m)), leading axes broadcast; `out` is the gufunc's optional output array."""
    at, xp, fp = map(_values, (at, xp, fp))
    lead = np.broadcast_shapes(at.shape[:-1], xp.shape[:-1], fp.shape[:-1])
    m, n = at.shape[-1], xp.shape[-1]
    a = np.moveaxis(np.broadcast_to(at, lead + (m,)), -1, 0).reshape(m, -1)
    shared = xp.ndim == 1
    x = xp if shared else np.moveaxis(np.broadcast_to(xp, lead + (n,)), -1, 0).reshape(n, -1)
    f = fp if fp.ndim == 1 else np.moveaxis(np.broadcast_to(fp, lead + (n,)), -1, 0).reshape(n, -1)
    res = np.moveaxis(_host(_device(_api.interp1d, a, x, f)).reshape((m,) + lead), 0, -1)
    if out is not None:
        out[...] = res
        return out
    return res


def bound_pressure(pressure, bound, vert_dim=VERT):
    """pf.py:208."""
    g = _Grid(pressure, vert_dim)
    return g.horiz(_device(_api.bound_pressure, g.values(pressure), _values(bound, None)), getattr(pressure, 'name', None),
                   getattr(pressure, 'attrs', {}))


def get_layer(dat, depth=100, vert_dim=VERT, interpolate=True):
    """pf.py:63."""
    g = _Grid(dat, vert_dim)
    r = _device(_api.get_layer, g.split(dat), depth=depth, interpolate=interpolate)
    vcoord = (np.arange(len(g.vc) + 1) + g.vc[0]) if interpolate else g.vc      # insert_level re-indexes (pf.py:971)
    return g.dataset(r, attrs=_attrs_of(dat), vert=True, vcoord=vcoord)


def insert_level(d, level, coords, vert_dim=VERT, fill_value=-999):
    """pf.py:933."""
    g = _Grid(d, vert_dim)
    arrs = g.split(d)
    g.check_index('Vert_dim index increments must all be 1.')                             # pf.py:957
    assert not np.any(arrs[coords] == fill_value), 'dataset d contains fill_value.'        # pf.py:965
    lev = {k: np.broadcast_to(_values(level[k], None), arrs[coords].shape[1:]) for k in _names(level)}
    r = _device(_api.insert_level, arrs, lev, coords=coords, fill_value=fill_value)
    return g.dataset(r, attrs=_attrs_of(d), vert=True, vcoord=np.arange(len(g.vc) + 1) + g.vc[0])


def find_intersections(x, a, b, dim, log_x=False):
    """pf.py:992."""
    g = _Grid(x, dim)
    g.check_index('Index increments must all be 1.')                                      # pf.py:1012
    xv = g.values(x)
    r = _device(_api.find_intersections, xv, np.broadcast_to(g.values(a), xv.shape), np.broadcast_to(g.values(b), xv.shape),
                log_x=log_x)
    return g.dataset(r, vert=True, vcoord=g.vc[1:], dim='offset_dim')                     # pf.py:1062


def trapz(dat, x, dim, mask=None, only_positive=False, only_negative=False):
    """pf.py:164: `dat` a Dataset, `x` the NAME of its x variable; every variable is integrated (x itself included, as
    in the reference)."""
    g = _Grid(dat, dim)
    arrs = g.split(dat)
    g.check_index('Index increments must all be 1.')                                      # pf.py:183
    assert not (only_positive and only_negative), 'Only negative OR positive regions can be included in trapz.'
    m = None
    if mask is not None:
        m = g.values(mask) if isinstance(mask, DataArray) else np.asarray(mask)
        m = np.broadcast_to(m, (m.shape[0],) + arrs[x].shape[1:])[:len(g.vc) - 1]          # labels 0 .. n-2 (pf.py:190-195)
    r = _device(_api.trapz, arrs, arrs[x], mask=m, only_positive=only_positive, only_negative=only_negative)
    return g.dataset(r)


def trap_around_zeros(x, y, dim, log_x=True, start=0):
    """pf.py:1200 (start = 0)."""
    g = _Grid(x, dim)
    g.check_index('Index increments must all be 1.')                                      # pf.py:1221
    areas, mask = _device(_api.trap_around_zeros, g.values(x), g.values(y), log_x=log_x, start=start)
    labels = np.concatenate([g.vc, g.vc[1:]])                                              # pf.py:1273: concat of the two families
    return g.dataset(areas, vert=True, vcoord=labels), g.vert(mask)


def shift_out_nans(x, name, dim):
    """pf.py:1699."""
    g = _Grid(x, dim)
    arrs = g.split(x)
    g.check_index('Index increments must all be 1.')                                      # pf.py:1712
    return g.dataset(_device(_api.shift_out_nans, arrs, name), attrs=_attrs_of(x), vert=True)


def _profiles(g, values, inputs, vcoord):
    """The rebased pressure, temperature and dewpoint of from_most_unstable_parcel / mix_layer, with their inputs' attrs."""
    return tuple(g.vert(v, k, getattr(src, 'attrs', {}), vcoord) for k, v, src in zip(_PARCEL_KEYS, values, inputs))


def from_most_unstable_parcel(pressure, temperature, dewpoint, vert_dim=VERT, depth=300):
    """pf.py:1517."""
    _named(pressure, temperature, dewpoint)
    g = _Grid(pressure, vert_dim)
    *prof, parcel, kept = _device(_api.from_most_unstable_parcel, *map(g.values, (pressure, temperature, dewpoint)),
                                  depth=depth)
    vcoord = g.vc[kept]                                                                    # dropna keeps the labels (pf.py:1552)
    return (*_profiles(g, prof, (pressure, temperature, dewpoint), vcoord), g.dataset(parcel, _PARCEL_KEYS))


def mix_layer(pressure, temperature, dewpoint, vert_dim=VERT, depth=100, load=True):
    """pf.py:1604."""
    _named(pressure, temperature, dewpoint)
    g = _Grid(pressure, vert_dim)
    *prof, parcel, kept = _device(_api.mix_layer, *map(g.values, (pressure, temperature, dewpoint)), depth=depth)
    surv = g.vc[kept]
    vcoord = np.concatenate([[(surv.min() if len(surv) else g.vc[0]) - 1], surv])         # pf.py:1641
    mp = g.dataset(parcel, _PARCEL_KEYS, lambda k: _attrs('mixed_parcel.' + k))
    return (*_profiles(g, prof, (pressure, temperature, dewpoint), vcoord), mp)


def add_lcl_to_profile(profile, vert_dim=VERT, environment=None, interpolator='log'):
    """pf.py:858."""
    assert interpolator in ['linear', 'log'], 'interpolator must be linear or log'         # pf.py:878
    g = _Grid(profile['pressure'], vert_dim)
    g.check_index('Vert_dim index increments must all be 1.')
    prof = {**{k: g.values(profile[k]) for k in ('pressure', 'temperature', 'virtual_temperature')},
            **{k: _values(profile[k], None) for k in _LCL_KEYS}}
    env = None if environment is None else _Grid(environment, vert_dim).split(environment)
    r = _device(_api.add_lcl_to_profile, prof, environment=env, interpolator=interpolator)
    vcoord = np.arange(len(g.vc) + 1) + g.vc[0]
    out = Dataset()
    for k, v in r.items():
        if k in _LCL_KEYS:
            out[k] = g.horiz(v, k, _attrs(k))
        else:
            src = environment[k[12:]] if k.startswith('environment_') else profile[k]
            out[k] = g.vert(v, k, getattr(src, 'attrs', {}), vcoord)
    for k in ('temperature', 'pressure', 'lcl_virtual_temperature'):                        # pf.py:889-891 (sic)
        out[k].attrs.update(_ATTRS['add_lcl_to_profile.' + k])
    return out


def moist_adiabat_lookup(pressure_levels=np.round(np.arange(1100, 2, step=-0.5), 1),
                         temperatures=np.round(np.arange(173, 316, step=0.02), 2), pres_step=0.5, temp_step=0.02):
    """pf.py:447: the two lookup tables as Datasets in the reference's layout -- adiabat_lookup.adiabat(pressure,
    temperature) = adiabat number (NaN = none) and adiabats.temperature(adiabat, pressure) -- generated on the GPU
    (adiabat_tables.moist_adiabat_lookup).  Only the reference's default grid is implemented: the device tables are
    addressed arithmetically on it."""
    from . import adiabat_tables as at
    pl, tt = at._grids()
    assert (np.array_equal(np.asarray(pressure_levels), pl) and np.array_equal(np.asarray(temperatures), tt) and
            pres_step == at.P_STEP and temp_step == at.T_STEP), 'only the default table grid is implemented'
    return _table_datasets(*at.moist_adiabat_lookup())


def _table_datasets(index, adiabats):
    from . import adiabat_tables as at
    pl, tt = at._grids()
    lookup = Dataset({'adiabat': DataArray(np.where(index == 0, np.nan, index.astype(np.float64)), dims=('pressure', 'temperature'),
                                           coords={'pressure': pl, 'temperature': tt}, attrs={'long_name': 'Adiabat index'},
                                           name='adiabat')})
    curves = Dataset({'temperature': DataArray(np.asarray(adiabats, dtype=np.float64)[:, ::-1], dims=('adiabat', 'pressure'),
                                               coords={'adiabat': np.arange(1, adiabats.shape[0] + 1), 'pressure': pl},
                                               attrs={'long_name': 'Temperature', 'units': 'K'}, name='temperature')})
    return lookup, curves


def moist_adiabat_tables(regenerate=False, cache=True, chunks=None, base_dir='.',
                         lookup_cache='/adiabat_lookups/moist_adiabat_lookup.nc',
                         adiabats_cache='/adiabat_lookups/adiabats_cache.nc', **kwargs):
    """pf.py:318: the cached tables, or freshly generated ones.  The cache is one .npz under
    base_dir/adiabat_lookups/ (NetCDF is not available here; `lookup_cache` / `adiabats_cache` / `chunks` are accepted
    and ignored); unlike the reference, a missing cache is regenerated instead of failing to open."""
    from . import adiabat_tables as at
    return _table_datasets(*at.moist_adiabat_tables(regenerate=regenerate, cache=cache, base_dir=base_dir))


# -- tables (pf.py:39-61) ------------------------------------------------------------------------------
def load_moist_adiabat_lookups(**kwargs):
    """pf.py:39: load (or generate and cache) the reference-format lookup tables; from here on every moist call of this
    module uses them, as in the reference."""
    from . import adiabat_tables
    adiabat_tables.load_moist_adiabat_lookups(**kwargs)


def lookup_tables_loaded():
    """pf.py:56."""
    from . import _lib
    assert _lib.load().xp_tables_loaded(), 'Call load_moist_adiabat_lookups first.'
