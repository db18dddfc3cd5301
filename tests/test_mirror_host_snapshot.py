"""CPU snapshot of the xarray mirror (xarray_parcel_amd/parcel_functions.py) around the array API.

The launch (`numpy_api._Call.run`) does nothing and every output the API allocates (`_Call.out`) is filled with a
pattern keyed on the number of outputs that call has allocated so far.  The mirror then runs to the end on a machine
without a GPU, and what it does around the API is recorded: every numpy_api call it makes (name, array arguments with
dtype, shape and values, scalar and keyword arguments) and what it returns (types, names, dims, coords, attrs, dtypes,
shapes, values).  The recording is tests/golden/mirror_host_snapshot.json; `python -m tests.test_mirror_host_snapshot`
rewrites it.  Not covered here: the table generators (moist_adiabat_lookup, moist_adiabat_tables,
load_moist_adiabat_lookups), which compute on the device and use none of the DataArray plumbing."""
import inspect
import json
import os

import numpy as np
import pytest

from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd import parcel_functions as pf
from xarray_parcel_amd._xr import DataArray, Dataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mirror_host_snapshot.json')
VD = 'model_level_number'
NOT_RECORDED = {'moist_adiabat_lookup', 'moist_adiabat_tables', 'load_moist_adiabat_lookups',   # device table generators
                'set_moist_lapse', 'lookup_tables_loaded'}                                     # test_table_asserts

# -- inputs: 5 levels, one column or a 2 x 3 grid ------------------------------------------------------------------------
P = np.array([1000., 925., 850., 700., 500.])
T = np.array([300., 295., 290., 282., 265.])
TD = np.array([295., 290., 283., 270., 250.])
Z = np.array([100., 800., 1500., 3000., 5500.])
Q = np.array([16., 13., 10., 6., 2.]) / 1000
OFF = np.arange(6.).reshape(2, 3) / 2
HC = {'lat': [10., 20.], 'lon': [1., 2., 3.]}


def col(v, name=None, coord=True, dtype=np.float64):
    """One column on VD (coordinate 1..5 unless coord=False)."""
    return DataArray(np.asarray(v, dtype=dtype), dims=(VD,), coords={VD: np.arange(1, 6)} if coord else None,
                     attrs={'units': 'x'}, name=name)


def grid(v, name=None, vdim=VD):
    """(lat, vdim, lon): the vertical between the horizontal dims, as in test_grid_dims_are_preserved."""
    return DataArray(v[None, :, None] + OFF[:, None, :], dims=('lat', vdim, 'lon'),
                     coords={**HC, vdim: np.arange(1, 6)}, attrs={'units': 'g'}, name=name)


def horiz(v, name=None):
    """A per-point field on (lat, lon)."""
    return DataArray(v + OFF, dims=('lat', 'lon'), coords=HC, attrs={'units': 'h'}, name=name)


def named(mk):
    return mk(P, 'pressure'), mk(T, 'temperature'), mk(TD, 'dewpoint')


def bundle():
    return Dataset({'pressure': grid(P), 'temperature': grid(T), 'specific_humidity': grid(Q), 'height_asl': grid(Z),
                    'wind_u': grid(np.arange(5.), vdim='wind_level'), 'wind_v': grid(-np.arange(5.), vdim='wind_level'),
                    'wind_height_above_surface': grid(Z - 100, vdim='wind_level'),
                    'surface_wind_u': horiz(1.0), 'surface_wind_v': horiz(-1.0)})


def profile():
    return Dataset({'pressure': grid(P, 'pressure'), 'temperature': grid(T - 1, 'temperature'),
                    'virtual_temperature': grid(T + 1, 'virtual_temperature'),
                    'environment_temperature': grid(T, 'environment_temperature'),
                    'lcl_pressure': horiz(900., 'lcl_pressure'), 'lcl_temperature': horiz(288., 'lcl_temperature'),
                    'lcl_virtual_temperature': horiz(289., 'lcl_virtual_temperature')})


def env():
    return Dataset({'pressure': grid(P, 'pressure'), 'temperature': grid(T, 'temperature'),
                    'dewpoint': grid(TD, 'dewpoint'), 'virtual_temperature': grid(T + 2, 'virtual_temperature')})


def ptd(surface=True):
    """pressure, temperature, dewpoint and (surface=True) a variable without the vertical."""
    ds = Dataset({'pressure': grid(P, 'pressure'), 'temperature': grid(T, 'temperature'), 'dewpoint': grid(TD, 'dewpoint')})
    if surface:
        ds['surface'] = horiz(5.0, 'surface')
    return ds


PV = (np.full((2, 3), 990.), np.full((2, 3), 299.), np.full((2, 3), 293.))
AT = np.linspace(520., 980., 4)

# name 'function' or 'function:variant' -> the call
CASES = {
    # drivers
    'surface_based_cape_cin:grid': lambda: pf.surface_based_cape_cin(grid(P), grid(T), grid(TD)),
    'surface_based_cape_cin:column_prefix': lambda: pf.surface_based_cape_cin(
        col(P), col(T), col(TD), prefix='sb', virtual_temperature_correction=False, lcl_interp='linear'),
    'surface_based_cape_cin:no_vert_coord': lambda: pf.surface_based_cape_cin(
        col(P, coord=False), col(T, coord=False), col(TD, coord=False)),
    'surface_based_cape_cin:f32_dataarray': lambda: pf.surface_based_cape_cin(
        col(P, dtype=np.float32), col(T, dtype=np.float32), col(TD, dtype=np.float32)),
    'surface_based_cape_cin:f32_ndarray': lambda: pf.surface_based_cape_cin(
        P.astype(np.float32), T.astype(np.float32), TD.astype(np.float32)),
    'cape_cin:grid': lambda: pf.cape_cin(grid(P), grid(T), grid(TD), PV[1], PV[0], PV[2], moist='family'),
    'most_unstable_cape_cin:column': lambda: pf.most_unstable_cape_cin(*named(col), depth=200, prefix='mu'),
    'most_unstable_cape_cin:grid': lambda: pf.most_unstable_cape_cin(*named(grid)),
    'mixed_layer_cape_cin:column': lambda: pf.mixed_layer_cape_cin(*named(col), prefix='ml'),
    'mixed_layer_cape_cin:grid': lambda: pf.mixed_layer_cape_cin(*named(grid), depth=50, lcl_interp='linear'),
    # column algorithms
    'lcl:grid': lambda: pf.lcl(horiz(990.), horiz(299.), PV[2]),
    'lcl:scalars': lambda: pf.lcl(1000., 300., 290.),
    'dry_lapse:grid': lambda: pf.dry_lapse(grid(P), PV[1], parcel_pressure=horiz(990.)),
    'dry_lapse:column': lambda: pf.dry_lapse(col(P), np.array([300.])),
    'moist_lapse:grid': lambda: pf.moist_lapse(grid(P), horiz(299.), parcel_pressure=PV[0]),
    'moist_lapse:column_table': lambda: pf.moist_lapse(col(P), np.array([300.]), moist='table'),
    'parcel_profile:column': lambda: pf.parcel_profile(col(P), 1000., 300., 295.),
    'parcel_profile:grid': lambda: pf.parcel_profile(grid(P), *PV, moist='family'),
    'parcel_profile_with_lcl:grid': lambda: pf.parcel_profile_with_lcl(grid(P), grid(T), grid(TD), *PV, lcl_interp='linear'),
    'lfc_el:grid': lambda: pf.lfc_el(grid(P), grid(T + 3), grid(T), horiz(900.), PV[1]),
    'cape_cin_base:grid': lambda: pf.cape_cin_base(grid(P), grid(T), horiz(850.), PV[0] - 500, grid(T + 3),
                                                   pos_cape_neg_cin=False, post_zero_cin=True),
    'most_unstable_parcel:grid': lambda: pf.most_unstable_parcel(ptd(False), depth=250),
    'mixed_parcel:grid': lambda: pf.mixed_parcel(*named(grid), depth=50),
    'mixed_layer:grid': lambda: pf.mixed_layer(ptd(False)),
    'wet_bulb_temperature:grid': lambda: pf.wet_bulb_temperature(grid(P), grid(T), grid(TD)),
    'wet_bulb_temperature:no_vertical': lambda: pf.wet_bulb_temperature(horiz(900.), horiz(290.), horiz(285.)),
    'log_interp:dataarray': lambda: pf.log_interp(grid(T, 'temperature'), grid(P), 500.),
    'log_interp:dataset': lambda: pf.log_interp(env(), grid(P), horiz(600.)),
    'linear_interp:no_attrs': lambda: pf.linear_interp(grid(T, 'temperature'), grid(P), 600., keep_attrs=False),
    'lifted_index:grid': lambda: pf.lifted_index(profile()),
    'lifted_index:prefix': lambda: pf.lifted_index(profile(), description='500 hPa', prefix='mu'),
    'mixing_ratio:dataarray': lambda: pf.mixing_ratio(grid(T), grid(TD), grid(P)),
    'mixing_ratio:ndarray': lambda: pf.mixing_ratio(T, TD, P),
    'virtual_temperature:dataarray': lambda: pf.virtual_temperature(grid(T), 0.01),
    'virtual_temperature:ndarray': lambda: pf.virtual_temperature(T, 0.01),
    'wet_bulb_temperature_fast:grid': lambda: pf.wet_bulb_temperature_fast(grid(T, 'temperature'), grid(TD)),
    'deep_convective_index:grid': lambda: pf.deep_convective_index(grid(P), grid(T), grid(TD), horiz(-2.)),
    'deep_convective_index:prefix': lambda: pf.deep_convective_index(grid(P), grid(T), grid(TD), PV[0] / 100,
                                                                     description='d', prefix='mu'),
    'lapse_rate:grid': lambda: pf.lapse_rate(grid(P), grid(T), grid(Z), from_pressure=850, to_pressure=500),
    'lapse_rate:f32_dataarray': lambda: pf.lapse_rate(col(P, dtype=np.float32), col(T, dtype=np.float32),
                                                      col(Z, dtype=np.float32)),
    'lapse_rate:f32_ndarray': lambda: pf.lapse_rate(P.astype(np.float32), T.astype(np.float32), Z.astype(np.float32)),
    'freezing_level_height:grid': lambda: pf.freezing_level_height(grid(T), grid(Z)),
    'melting_level_height:fast': lambda: pf.melting_level_height(grid(P), grid(T), grid(TD), grid(Z)),
    'melting_level_height:slow': lambda: pf.melting_level_height(grid(P), grid(T), grid(TD), grid(Z), fast=False),
    'isobar_temperature:grid': lambda: pf.isobar_temperature(grid(P), grid(T), 700),
    'dewpoint_from_specific_humidity:grid': lambda: pf.dewpoint_from_specific_humidity(grid(P), grid(T), grid(Q)),
    'dewpoint_from_specific_humidity:no_vertical': lambda: pf.dewpoint_from_specific_humidity(
        horiz(900.), horiz(290.), horiz(0.01)),
    # product bundle
    'wind_shear:grid': lambda: pf.wind_shear(horiz(1.), PV[0] / 1000, grid(np.arange(5.), vdim='wind_level'),
                                             grid(-np.arange(5.), vdim='wind_level'), grid(Z, vdim='wind_level'),
                                             shear_height=3000, vert_dim='wind_level'),
    'significant_hail_parameter:dataarray': lambda: pf.significant_hail_parameter(
        horiz(2000.), horiz(12.), horiz(7.), horiz(-15.), horiz(25.), horiz(3500.)),
    'significant_hail_parameter:ndarray': lambda: pf.significant_hail_parameter(*(np.full(3, v) for v in (
        2000., 12., 7., -15., 25., 3500.))),
    'valid_data:dataset': lambda: pf.valid_data(Dataset({'pressure': grid(P), VD: DataArray(np.arange(1, 6), dims=(VD,))}),
                                                VD),
    'conv_properties:grid': lambda: pf.conv_properties(bundle()),
    'conv_properties:ignore_nans': lambda: pf.conv_properties(bundle(), ignore_nans=True, moist='family'),
    'min_conv_properties:grid': lambda: pf.min_conv_properties(bundle()),
    'storm_proxies:grid': lambda: pf.storm_proxies(pf.conv_properties(bundle())),
    # array primitives
    'round_to:array': lambda: pf.round_to(np.array([1.2345, 273.149]), 0.02),
    'interp1d_numba:grid': lambda: pf.interp1d_numba(np.broadcast_to(AT, (2, 3, 4)), P[::-1] + OFF[..., None],
                                                     T[::-1] + OFF[..., None]),
    'interp1d_numba:shared_xp': lambda: pf.interp1d_numba(AT, P[::-1], np.stack([T[::-1], TD[::-1]])),
    'interp1d_numba:out': lambda: pf.interp1d_numba(np.broadcast_to(AT, (3, 4)), P[::-1], T[::-1], out=np.zeros((3, 4))),
    'bound_pressure:grid': lambda: pf.bound_pressure(grid(P, 'pressure'), horiz(700.)),
    'bound_pressure:scalar': lambda: pf.bound_pressure(col(P), 650.),
    'get_layer:grid': lambda: pf.get_layer(ptd(), depth=100),
    'get_layer:no_interpolate': lambda: pf.get_layer(ptd(), depth=300, interpolate=False),
    'insert_level:grid': lambda: pf.insert_level(
        ptd(), Dataset({'pressure': horiz(800.), 'temperature': horiz(285.), 'dewpoint': horiz(280.)}), 'pressure'),
    'find_intersections:grid': lambda: pf.find_intersections(grid(P), grid(T), grid(TD), VD, log_x=True),
    'trapz:grid': lambda: pf.trapz(ptd(), 'pressure', VD),
    'trapz:mask': lambda: pf.trapz(ptd(), 'pressure', VD, mask=grid(np.array([1., 0, 1, 0, 1])), only_positive=True),
    'trapz:ndarray_mask': lambda: pf.trapz(ptd(), 'pressure', VD, mask=np.array([1, 0, 1, 0, 1]).reshape(5, 1, 1),
                                           only_negative=True),
    'trap_around_zeros:grid': lambda: pf.trap_around_zeros(grid(P), grid(T - TD - 5), VD, log_x=False),
    'shift_out_nans:grid': lambda: pf.shift_out_nans(ptd(), 'pressure', VD),
    'from_most_unstable_parcel:grid': lambda: pf.from_most_unstable_parcel(*named(grid), depth=200),
    'mix_layer:grid': lambda: pf.mix_layer(*named(grid)),
    'add_lcl_to_profile:environment': lambda: pf.add_lcl_to_profile(profile(), environment=env(), interpolator='linear'),
    'add_lcl_to_profile:plain': lambda: pf.add_lcl_to_profile(profile()),
}


# -- the stand-ins for the launch and the outputs ------------------------------------------------------------------------
def _fake_out(self, shape, dtype=None):
    """Output number k of this call: 10 k + i/2 for element i (ints: (k + i) mod 3), its last row NaN when it has at least
    three rows -- the NaN padding the drivers trim."""
    dtype = np.dtype(dtype or self.dtype)
    self._n_out = getattr(self, '_n_out', 0) + 1
    i = np.arange(int(np.prod(shape)))
    if dtype.kind in 'iu':
        return ((self._n_out + i) % 3).astype(dtype).reshape(shape)
    a = (10 * self._n_out + 0.5 * i).astype(dtype).reshape(shape)
    if len(shape) and shape[0] >= 3:
        a[-1] = np.nan
    return a


def _enc(x):
    """JSON form of an argument or result."""
    if isinstance(x, Dataset):
        names = list(x.data_vars) if hasattr(x, 'data_vars') else list(x.keys())
        return {'type': 'Dataset', 'vars': [[k, _enc(x[k])] for k in names],
                'attrs': x.attrs if isinstance(x.attrs, list) else _enc(dict(x.attrs))}
    if isinstance(x, DataArray):
        return {'type': 'DataArray', 'name': x.name, 'dims': list(x.dims), 'attrs': _enc(dict(x.attrs)),
                'coords': {k: _enc(np.asarray(v)) for k, v in x.coords.items()}, 'data': _enc(np.asarray(x.values))}
    if isinstance(x, (np.ndarray, np.generic)):
        return [str(x.dtype), list(np.shape(x)), np.asarray(x).tolist()]            # dtype, shape, values
    if isinstance(x, dict):
        return {str(k): _enc(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_enc(v) for v in x]
    assert x is None or isinstance(x, (bool, int, float, str)), type(x)
    return x


def _result(x):
    return {'type': type(x).__name__, 'value': _enc(x)}


def _offline(monkeypatch):
    """The API without its launches; returns the list the mirror's numpy_api calls are recorded into."""
    calls, depth = [], [0]
    monkeypatch.setattr(api._Call, 'run', lambda self, name, *args: None)
    monkeypatch.setattr(api._Call, 'out', _fake_out)
    monkeypatch.setattr(api.torch.cuda, 'is_available', lambda: False)      # the bundles stay on the host

    def recorded(name, fn):
        def call(*args, **kwargs):
            if depth[0] == 0:
                calls.append({'fn': name, 'args': _enc(list(args)), 'kwargs': _enc(kwargs)})
            depth[0] += 1
            try:
                return fn(*args, **kwargs)
            finally:
                depth[0] -= 1
        return call
    for name, fn in inspect.getmembers(api, inspect.isfunction):
        if not name.startswith('_') and fn.__module__ == api.__name__:
            monkeypatch.setattr(api, name, recorded(name, fn))
    return calls


@pytest.fixture
def offline(monkeypatch):
    return _offline(monkeypatch)


def _record(case, calls):
    del calls[:]
    out = _result(CASES[case]())
    return {'calls': list(calls), 'result': out}


def _canon(x):
    return json.dumps(x, sort_keys=True)


def test_every_public_function_is_recorded():
    public = {n for n, f in inspect.getmembers(pf, inspect.isfunction) if not n.startswith('_') and f.__module__ == pf.__name__}
    covered = {c.split(':')[0] for c in CASES}
    assert covered <= public and public - covered == NOT_RECORDED, (covered - public, public - covered - NOT_RECORDED)


@pytest.mark.parametrize('case', list(CASES))
def test_mirror_matches_snapshot(case, offline):
    with open(GOLDEN) as f:
        gold = json.load(f)[case]
    got = json.loads(_canon(_record(case, offline)))
    assert len(got['calls']) == len(gold['calls']), [c['fn'] for c in got['calls']]
    for i, (g, w) in enumerate(zip(got['calls'], gold['calls'])):
        assert _canon(g) == _canon(w), f'numpy_api call {i} ({w["fn"]})'
    assert _canon(got['result']) == _canon(gold['result'])


# -- assert paths: the reference's messages ------------------------------------------------------------------------------
def test_reference_asserts(offline):
    p, t, td = named(grid)
    for args, msg in (((col(P), t, td), 'Pressure requires name pressure.'),
                      ((p, col(T), td), 'Temperature requires name temperature.'),
                      ((p, t, col(TD)), 'Dewpoint requires name dewpoint.')):
        for fn in (pf.most_unstable_cape_cin, pf.mixed_layer_cape_cin, pf.from_most_unstable_parcel, pf.mix_layer):
            with pytest.raises(AssertionError, match=msg):
                fn(*args)
    with pytest.raises(AssertionError, match='pressure requires name pressure.'):
        pf.mixed_parcel(grid(P, None), t, td)
    step2 = lambda v: DataArray(v, dims=(VD,), coords={VD: np.arange(5) * 2}, name='pressure')
    with pytest.raises(AssertionError, match='Vert_dim index increments must all be 1.'):
        pf.surface_based_cape_cin(step2(P), step2(T), step2(TD))
    with pytest.raises(AssertionError, match='Vert_dim index increments must all be 1.'):
        pf.insert_level(Dataset({'pressure': step2(P)}), Dataset({'pressure': DataArray(800.)}), 'pressure')
    with pytest.raises(AssertionError, match='Vert_dim index increments must all be 1.'):
        pf.add_lcl_to_profile(Dataset({'pressure': step2(P), 'temperature': step2(T), 'virtual_temperature': step2(T),
                                       'lcl_pressure': DataArray(900.), 'lcl_temperature': DataArray(288.),
                                       'lcl_virtual_temperature': DataArray(289.)}))
    for call in (lambda: pf.lfc_el(step2(P), step2(T), step2(T), 900., 288.),
                 lambda: pf.cape_cin_base(step2(P), step2(T), 850., 300., step2(T)),
                 lambda: pf.freezing_level_height(step2(T), step2(Z)),
                 lambda: pf.find_intersections(step2(P), step2(T), step2(TD), VD),
                 lambda: pf.trapz(Dataset({'pressure': step2(P)}), 'pressure', VD),
                 lambda: pf.trap_around_zeros(step2(P), step2(T), VD),
                 lambda: pf.shift_out_nans(Dataset({'pressure': step2(P)}), 'pressure', VD)):
        with pytest.raises(AssertionError, match='Index increments must all be 1.'):
            call()
    with pytest.raises(AssertionError, match='Index increments must all be 1.'):
        pf.valid_data(Dataset({'pressure': grid(P), VD: DataArray(np.arange(5) * 2, dims=(VD,))}), VD)
    with pytest.raises(AssertionError, match='Pressures must decrease with increasing level number.'):
        pf.valid_data(Dataset({'pressure': grid(P[::-1]), VD: DataArray(np.arange(1, 6), dims=(VD,))}), VD)
    with pytest.raises(AssertionError, match='dataset d contains fill_value.'):
        pf.insert_level(Dataset({'pressure': col(np.where(P == 700, -999, P))}), Dataset({'pressure': DataArray(800.)}),
                        'pressure')
    with pytest.raises(AssertionError, match='extrapolation is not part of the MI355X path'):
        pf.linear_interp(grid(T), grid(P), 500., extrapolate=True)
    with pytest.raises(AssertionError, match='interpolator must be linear or log'):
        pf.add_lcl_to_profile(profile(), interpolator='cubic')
    with pytest.raises(AssertionError, match='Only negative OR positive regions can be included in trapz.'):
        pf.trapz(ptd(), 'pressure', VD, only_positive=True, only_negative=True)
    with pytest.raises(AssertionError, match='only the default table grid is implemented'):
        pf.moist_adiabat_lookup(pressure_levels=np.array([1000., 999.5]))


# every mirror function that lifts a parcel moist-adiabatically
MOIST_CALLS = {
    'surface_based_cape_cin': lambda **kw: pf.surface_based_cape_cin(grid(P), grid(T), grid(TD), **kw),
    'most_unstable_cape_cin': lambda **kw: pf.most_unstable_cape_cin(*named(grid), **kw),
    'mixed_layer_cape_cin': lambda **kw: pf.mixed_layer_cape_cin(*named(grid), **kw),
    'cape_cin': lambda **kw: pf.cape_cin(grid(P), grid(T), grid(TD), PV[1], PV[0], PV[2], **kw),
    'moist_lapse': lambda **kw: pf.moist_lapse(col(P), np.array([300.]), **kw),
    'parcel_profile': lambda **kw: pf.parcel_profile(col(P), 1000., 300., 295., **kw),
    'parcel_profile_with_lcl': lambda **kw: pf.parcel_profile_with_lcl(grid(P), grid(T), grid(TD), *PV, **kw),
    'wet_bulb_temperature': lambda **kw: pf.wet_bulb_temperature(grid(P), grid(T), grid(TD), **kw),
    'melting_level_height': lambda **kw: pf.melting_level_height(grid(P), grid(T), grid(TD), grid(Z), fast=False, **kw),
    'conv_properties': lambda **kw: pf.conv_properties(bundle(), **kw),
    'min_conv_properties': lambda **kw: pf.min_conv_properties(bundle(), **kw),
}


@pytest.mark.parametrize('fn', list(MOIST_CALLS))
def test_table_asserts(fn, offline, monkeypatch):
    """Without tables the reference's 'Call load_moist_adiabat_lookups first.': from lookup_tables_loaded() under the
    default mode, and from the library's XP_E_NO_TABLES under an explicit moist='table'.  Other library errors pass
    through as they are."""
    class _NoTables:
        def xp_tables_loaded(self):
            return 0
    monkeypatch.setattr(L, 'load', lambda: _NoTables())
    pf.set_moist_lapse(None)
    with pytest.raises(AssertionError, match='Call load_moist_adiabat_lookups first.'):
        MOIST_CALLS[fn]()
    pf.set_moist_lapse('exact')
    for code, err in ((L.XP_E_NO_TABLES, AssertionError), (L.XP_E_ARG, L.XParcelError)):
        def fail(self, name, *args, code=code):
            raise L.XParcelError(code, 'stand-in')
        monkeypatch.setattr(api._Call, 'run', fail)
        with pytest.raises(err) as e:
            MOIST_CALLS[fn](moist='table')
        assert err is L.XParcelError or str(e.value) == 'Call load_moist_adiabat_lookups first.'


if __name__ == '__main__':
    mp = pytest.MonkeyPatch()
    pf.set_moist_lapse('exact')                     # the suite's mode (tests/conftest.py)
    calls = _offline(mp)
    snap = {case: _record(case, calls) for case in CASES}
    mp.undo()
    with open(GOLDEN, 'w') as f:
        f.write(json.dumps(snap, sort_keys=True, separators=(',', ':')) + '\n')
    print(f'{GOLDEN}: {len(snap)} cases, {os.path.getsize(GOLDEN)} bytes')
