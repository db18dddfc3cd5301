"""Hydrostatic heights and layer thickness on the device (xp_hydrostatic_height, xp_geopotential_to_height,
xp_height_to_geopotential) against the NumPy restatement tests/hydrostatic_restatement.py, and their own argument checks.  The
inputs and what they hold are counted on the CPU (tests/test_hydrostatic_cpu.py::test_input_census).
Comparison rule: status words and NaN patterns equal the restatement's in EVERY column -- the gate's decisions involve no
transcendental, so there is no tie class to leave out.
Bound (TOL) on |device - restatement| of heights and thicknesses in f64: an interval's error from one last-bit difference in
ln p is about 29.3 m/K x 250 K x 2e-15 = 1.5e-11 m; 64 such intervals plus 64 roundings of a 2e4 m sum stay below 1e-9 m; the
cap 1e-7 m is 100 x that, so anything near 1e-6 m is a bug, not rounding.  TOL is at least 100 x the largest difference measured
on an MI355X over all grids and variants and never above the cap; the per-point products are held to 1e-12 relative.
Measured on an MI355X over the six grids x three moisture kinds x with and without base_height x four layers and none, the
isobaric variant and the hand-built columns: heights 1.6e-11 m, thicknesses 1.1e-11 m, hence TOL = 1e-8 m (600 x); f32 inputs
9.8e-4 m (one float32 spacing at 2e4 m is 2e-3 m); the per-point products equal NumPy's bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import hydrostatic_cases as K
from tests import hydrostatic_restatement as R
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa

pytestmark = pytest.mark.gpu
CAP = 1e-7                      # [m], what the rounding argument allows at most
TOL = 1e-8                      # [m], heights and thicknesses, f64
assert TOL <= CAP
KINDS = (R.DRY, R.DEWPOINT, R.SPECIFIC)


@functools.lru_cache(maxsize=None)
def inputs(name, dtype=np.float64):
    return K.inputs(*K.GRIDS[name], dtype=dtype)


@functools.lru_cache(maxsize=None)
def restated(name, kind, with_base, dtype=np.float64):
    """The restatement of one grid with K.LAYERS (computed once, shared, left unchanged); the heights are those of the call
    without layers too."""
    p, t, td, q, base = (a.astype(np.float64) for a in inputs(name, dtype))
    return R.grid(p, t, {R.DRY: None, R.DEWPOINT: td, R.SPECIFIC: q}[kind], kind, base if with_base else None, K.LAYERS)


def run(kind, p, t, td, q, base=None, layers=(), **kw):
    return xa.hydrostatic(p, t, dewpoint=td if kind == R.DEWPOINT else None, specific_humidity=q if kind == R.SPECIFIC else None,
                          base_height=base, layers=layers, **kw)


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


def compare(got, ref, layers=True, f32=False, label=''):
    """Status and NaN patterns equal in every column, every height and thickness within TOL; prints the largest difference."""
    # (without layers XP_ST_NO_LAYER is left to the columns without a valid level)
    want_status = ref['status'] if layers else np.where(ref['nvalid'] == 0, R.ST_NO_LAYER, ref['status'] & R.ST_BAD_PRESSURE)
    assert np.array_equal(_np(got['status']), want_status), (label, np.nonzero(_np(got['status']) != want_status)[0][:5])
    rows = [('height', _np(got['height']), ref['height'])]
    if layers:
        rows.append(('thickness', np.stack([_np(x) for x in got['thickness']]), ref['thickness']))
    for k, g, r in rows:
        g = g.astype(np.float64).reshape(r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, k, np.argwhere(np.isnan(g) != np.isnan(r))[:5])
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        bound = np.full(err.shape, TOL)
        if f32:
            bound = bound + np.spacing(np.abs(r[ok]).astype(np.float32)).astype(np.float64)
        worst = float(err.max()) if ok.any() else 0.0
        print('%-40s %-10s n = %6d  max = %.3e m' % (label, k, ok.sum(), worst))
        assert np.all(err <= bound), (label, k, worst, np.argwhere(ok)[np.argmax(err - bound)])


@pytest.mark.parametrize('name', sorted(K.GRIDS))
def test_grid_parity(name):
    """Every grid x {dry, dewpoint, specific humidity} x {base_height or not} x {all four layers, none}."""
    p, t, td, q, base = inputs(name)
    for kind in KINDS:
        for with_base in (False, True):
            ref = restated(name, kind, with_base)
            for layers in (K.API_LAYERS, ()):
                got = run(kind, p, t, td, q, base if with_base else None, layers)
                assert len(got['thickness']) == len(layers)
                compare(got, ref, bool(layers), label='%s %s base=%d layers=%d' % (name, kind, with_base, len(layers)))
    if name == '40x640':
        assert (np.isfinite(ref['thickness']).sum(axis=1) >= 160).all() and np.isnan(ref['thickness'][0]).sum() > 300


def test_outputs_do_not_depend_on_each_other():
    p, t, td, q, base = inputs('24x300')
    for kind in KINDS:
        full = run(kind, p, t, td, q, base, K.API_LAYERS)
        alone = run(kind, p, t, td, q, base)
        assert np.array_equal(full['height'], alone['height'], equal_nan=True), kind                # bit-identical
        only = run(kind, p, t, td, q, None, K.API_LAYERS, want=('thickness',))
        assert sorted(only) == ['thickness']
        for a, b in zip(only['thickness'], full['thickness']):
            assert np.array_equal(a, b, equal_nan=True), kind                                       # no height output, no base_height
        for lo, hi in ((1, 2), (0, 2), (1, 4)):                                                     # one, two, three layers: other kernels
            part = run(kind, p, t, td, q, base, K.API_LAYERS[lo:hi], want=('thickness', 'height'))
            assert np.array_equal(part['height'], full['height'], equal_nan=True), (kind, lo, hi)
            for a, b in zip(part['thickness'], full['thickness'][lo:hi]):
                assert np.array_equal(a, b, equal_nan=True), (kind, lo, hi)
    assert np.array_equal(xa.thickness_hydrostatic(p, t, td), run(R.DEWPOINT, p, t, td, q, None, K.API_LAYERS)['thickness'][3], equal_nan=True)
    z, st = xa.hydrostatic_height(p, t, td, base_height=base, status=True)
    full = run(R.DEWPOINT, p, t, td, q, base)
    assert np.array_equal(z, full['height'], equal_nan=True) and np.array_equal(st, full['status'])


def test_fp32_inputs_round_like_the_restatement():
    p, t, td, q, base = inputs('12x640', np.float32)
    for kind in KINDS:
        got = run(kind, p, t, td, q, base, K.API_LAYERS)
        assert got['height'].dtype == np.float32 and got['thickness'][0].dtype == np.float32 and got['status'].dtype == np.int32
        compare(got, restated('12x640', kind, True, np.float32), f32=True, label='f32 ' + kind)


def test_input_kinds_and_strided_views():
    import torch
    p, t, td, q, base = inputs('24x300')
    ref = run(R.DEWPOINT, p, t, td, q, base, K.API_LAYERS)
    cpu = run(R.DEWPOINT, *(torch.from_numpy(a) for a in (p, t, td, q, base)), K.API_LAYERS)
    dev = run(R.DEWPOINT, *(torch.from_numpy(a).cuda() for a in (p, t, td, q, base)), K.API_LAYERS)
    flat = lambda r: [r['height'], *r['thickness'], r['status']]
    for a, b, c in zip(flat(ref), flat(cpu), flat(dev)):
        assert isinstance(b, np.ndarray) and c.is_cuda                                              # the result stays on the device
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c.cpu().numpy(), equal_nan=True)
    # host arrays with a base height on the device: a device call
    mixed = run(R.SPECIFIC, p, t, td, q, torch.from_numpy(base).cuda())
    assert mixed['height'].is_cuda and np.array_equal(mixed['height'].cpu().numpy(), run(R.SPECIFIC, p, t, td, q, base)['height'], equal_nan=True)
    # a 1-D pressure (isobaric data) is expanded to the grid
    p1 = p[:, 0].copy()
    pg = np.ascontiguousarray(np.broadcast_to(p1[:, None], p.shape))
    want = run(R.DEWPOINT, pg, t, td, q, None, K.API_LAYERS)
    compare(want, R.grid(pg, t, td, R.DEWPOINT, None, K.LAYERS), label='isobaric')
    for one in (run(R.DEWPOINT, p1, t, td, q, None, K.API_LAYERS), run(R.DEWPOINT, torch.from_numpy(p1), torch.from_numpy(t).cuda(), td, q, None, K.API_LAYERS)):
        for a, b in zip(flat(want), flat(one)):
            assert np.array_equal(a, _np(b), equal_nan=True)
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev, ncol = p.shape
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (p, t, td)]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    z = torch.empty((nlev, ncol), dtype=torch.float64, device='cuda')
    th = [torch.empty(ncol, dtype=torch.float64, device='cuda') for _ in range(4)]
    status = torch.empty(ncol, dtype=torch.int32, device='cuda')
    dbase = torch.from_numpy(base).cuda()
    o = L.HydrostaticOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, height=z.data_ptr(), status=status.data_ptr())
    for i in range(4):
        o.thickness[i] = th[i].data_ptr()
    layers = (L.WindLayer * 4)(*[L.WindLayer(k, 0, b, tt) for k, b, tt in K.LAYERS])
    L.check(lib.xp_hydrostatic_height(views[0], views[1], views[2], dbase.data_ptr(), 4, layers, L.HydrostaticOpts(L.HUM_DEWPOINT, 0), o, None))
    torch.cuda.synchronize()
    for a, b in zip(flat(ref), [z] + th + [status]):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)


def test_hand_built_columns():
    p, t, td = K.hand_columns()
    q = K.specific_humidity(p, td)
    for kind in KINDS:
        m = {R.DRY: None, R.DEWPOINT: td, R.SPECIFIC: q}[kind]
        ref = R.grid(p, t, m, kind, None, K.HAND_LAYERS)
        got = run(kind, p, t, td, q, None, K.HAND_API_LAYERS)
        compare(got, ref, label='hand ' + kind)
        z, th, st = got['height'], np.stack(got['thickness']), got['status']
        assert list(st) == [0, 0, L.XP_ST_NO_LAYER, L.XP_ST_NO_LAYER, 0, L.ST_BAD_PRESSURE, 0, 0]
        assert np.isnan(z[:, 2]).all() and z[4, 3] == 0.0 and np.isnan(np.delete(z[:, 3], 4)).all()       # all NaN; one valid level
        assert np.isnan(z[3, 4]) and np.isfinite(np.delete(z[:, 4], 3)).all()                            # a NaN temperature in the middle
        assert np.isfinite(z[:4, 5]).all() and np.isnan(z[4:, 5]).all() and np.isnan(th[:, 5]).all()     # a repeated pressure
        assert abs(th[0, 6] - (z[5, 6] - z[2, 6])) <= TOL and abs(th[0, 7] - (z[5, 7] - z[2, 7])) <= TOL  # bounds on / close to levels
        assert np.all(np.abs(th[2, [0, 1, 4, 6, 7]] - z[7, [0, 1, 4, 6, 7]]) <= TOL)                     # the whole column
    dry = run(R.DRY, p, t, td, q)['height']
    assert np.all(np.abs(dry[:, 0] - R.RD * 250.0 / R.G * np.log(1000.0 / p[:, 0])) <= TOL)              # isothermal
    x = np.log(p[:, 1])
    a, b = 288.0 - 40.0 * x[0], 40.0
    assert np.all(np.abs(dry[:, 1] - R.RD / R.G * (a * (x[0] - x) + 0.5 * b * (x[0] ** 2 - x ** 2))) <= TOL)   # T linear in ln p


def test_per_point_products():
    import torch
    z = np.r_[0.0, np.geomspace(1.0, 8e4, 997), -300.0, np.nan]
    phi = R.height_to_geopotential(z)
    for fn, ref, x in ((xa.height_to_geopotential, phi, z), (xa.geopotential_to_height, R.geopotential_to_height(phi), phi)):
        got = fn(x.reshape(10, 100))
        assert got.shape == (10, 100) and np.array_equal(np.isnan(got.ravel()), np.isnan(ref))
        rel = np.abs(got.ravel() - ref)[:-1] / np.maximum(np.abs(ref[:-1]), 1e-300)
        print(fn.__name__, 'max relative difference %.3e' % rel[1:].max())
        assert got.ravel()[0] == 0.0 and np.all(rel[1:] <= 1e-12)
        dev = fn(torch.from_numpy(x).cuda())
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got.ravel(), equal_nan=True)
        f32 = fn(x.astype(np.float32))
        assert f32.dtype == np.float32 and np.allclose(f32[:-1], ref[:-1], rtol=3e-7, atol=0.0)
    back = xa.geopotential_to_height(xa.height_to_geopotential(z))
    assert np.all(np.abs(back - z)[:-1] <= 1e-11 * np.maximum(np.abs(z[:-1]), 1.0))


def test_heights_feed_wind_layers_on_the_device():
    """The chain the call exists for: device heights straight into a layer by height."""
    import torch
    p, t, td, q, base = inputs('40x640')
    rng = np.random.default_rng(5)
    u, v = rng.uniform(-30.0, 30.0, p.shape), rng.uniform(-30.0, 30.0, p.shape)
    dev = [torch.from_numpy(a).cuda() for a in (p, t, td, u, v)]
    z = xa.hydrostatic_height(dev[0], dev[1], dev[2])
    assert z.is_cuda
    layer = [('height', 0.0, 3000.0)]
    on_dev = xa.wind_layers(dev[0], dev[3], dev[4], z, layer)
    on_host = xa.wind_layers(p, u, v, z.cpu().numpy(), layer)
    st = on_dev['status'].cpu().numpy()
    assert not np.any(st & L.ST_BAD_HEIGHT) and not np.any(st & L.ST_BAD_PRESSURE) and (st == 0).sum() >= 600
    for k in L.WIND_LAYERS_OUT:
        assert on_dev[k].is_cuda and np.array_equal(on_dev[k].cpu().numpy(), on_host[k], equal_nan=True), k
    assert np.array_equal(st, on_host['status']) and np.isfinite(on_host['mean_u']).sum() >= 600


def test_raw_abi_errors():
    lib = L.init(0)
    p, t, td, q, base = (np.ascontiguousarray(a) for a in K.inputs(12, 8, seed=2))
    view = lambda a, nlev=12, dtype=L.XP_F64, mem=L.XP_MEM_HOST: L.View(a.ctypes.data, dtype, mem, nlev, 8, 8, 1)
    vp, vt, vm = view(p), view(t), view(td)
    z, th, extra = np.zeros((12, 8)), np.zeros(8), np.zeros(8)
    nan, inf = float('nan'), float('inf')

    def call(p=vp, t=vt, m=vm, nlayer=None, layers=((L.LAYER_PRESSURE, 900.0, 500.0),), opts=(L.HUM_DEWPOINT, 0), out=True,
             dtype=L.XP_F64, mem=L.XP_MEM_HOST, extra_at=None):
        o = L.HydrostaticOut(dtype=dtype, mem=mem, height=z.ctypes.data)
        n = (0 if layers is None else len(layers)) if nlayer is None else nlayer
        if layers:
            o.thickness[0] = th.ctypes.data
        if extra_at is not None:
            o.thickness[extra_at] = extra.ctypes.data
        la = (L.WindLayer * len(layers))(*[L.WindLayer(k, 0, b, tt) for k, b, tt in layers]) if layers else None
        return lib.xp_hydrostatic_height(p, t, m, base.ctypes.data, n, la, None if opts is None else L.HydrostaticOpts(*opts), o if out else None, None)
    assert call() == L.XP_OK and np.isfinite(z).any() and np.isfinite(th).any()
    assert call(opts=None) == L.XP_OK and call(m=None) == L.XP_OK and call(layers=None) == L.XP_OK
    assert call(layers=((L.LAYER_PRESSURE, nan, nan), (L.LAYER_PRESSURE_DEPTH, nan, 100.0))) == L.XP_OK
    for kw, word in (({'p': None}, 'pressure'), ({'t': None}, 'temperature'), ({'t': view(t, 6)}, 'temperature'),
                     ({'m': view(td, 6)}, 'moisture'), ({'m': view(td, dtype=L.XP_F32)}, 'moisture'),
                     ({'m': view(td, mem=L.XP_MEM_DEVICE)}, 'moisture'), ({'opts': (2, 0)}, 'humidity'), ({'opts': (-1, 0)}, 'humidity'),
                     ({'nlayer': -1}, 'nlayer'), ({'nlayer': 5}, 'nlayer'), ({'layers': None, 'nlayer': 1}, 'layers'),
                     ({'layers': ((L.LAYER_HEIGHT, 0.0, 3000.0),)}, 'height'), ({'layers': ((7, 900.0, 500.0),)}, 'kind'),
                     ({'layers': ((L.LAYER_PRESSURE_DEPTH, nan, 0.0),)}, 'depth'), ({'layers': ((L.LAYER_PRESSURE_DEPTH, nan, -5.0),)}, 'depth'),
                     ({'layers': ((L.LAYER_PRESSURE_DEPTH, nan, nan),)}, 'top'), ({'layers': ((L.LAYER_PRESSURE_DEPTH, nan, inf),)}, 'top'),
                     ({'layers': ((L.LAYER_PRESSURE, 900.0, inf),)}, 'top'), ({'layers': ((L.LAYER_PRESSURE, -inf, 500.0),)}, 'bottom'),
                     ({'extra_at': 1}, 'thickness[1]'), ({'layers': None, 'extra_at': 0}, 'thickness[0]'),
                     ({'out': False}, 'out'), ({'dtype': L.XP_F32}, 'out'), ({'mem': L.XP_MEM_DEVICE}, 'out')):
        assert call(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())
    for entry in (lib.xp_geopotential_to_height, lib.xp_height_to_geopotential):
        assert entry(8, L.XP_F64, L.XP_MEM_HOST, None, th.ctypes.data, None) == L.XP_E_ARG
        assert entry(8, L.XP_F64, L.XP_MEM_HOST, th.ctypes.data, None, None) == L.XP_E_ARG
        assert entry(-1, L.XP_F64, L.XP_MEM_HOST, th.ctypes.data, extra.ctypes.data, None) == L.XP_E_ARG


def test_dataarray_module_end_to_end():
    from xarray_parcel_amd import hydrostatic as mirror
    from xarray_parcel_amd._xr import DataArray
    p, t, td, q, base = inputs('12x640')
    full = run(R.SPECIFIC, p, t, td, q, base, K.API_LAYERS)
    da = [DataArray(a.reshape(12, 20, 32), dims=('model_level_number', 'y', 'x'), name=n) for a, n in zip((p, t, q), ('p', 't', 'q'))]
    ds = mirror.hydrostatic(da[0], da[1], specific_humidity=da[2], base_height=DataArray(base.reshape(20, 32), dims=('y', 'x')), layers=K.API_LAYERS)
    assert ds['height'].dims == ('model_level_number', 'y', 'x') and ds['height'].attrs['units'] == 'm'
    assert np.array_equal(np.asarray(ds['height'].values).reshape(12, -1), full['height'], equal_nan=True)
    assert ds['thickness'].dims == ('hydrostatic_layer', 'y', 'x')
    assert np.array_equal(np.asarray(ds['thickness'].values).reshape(4, -1), np.stack(full['thickness']), equal_nan=True)
    assert np.array_equal(np.asarray(ds['status'].values).reshape(-1), full['status']) and ds['status'].dims == ('y', 'x')
    z = mirror.hydrostatic_height(da[0], da[1], specific_humidity=da[2])
    assert np.array_equal(np.asarray(z.values).reshape(12, -1), run(R.SPECIFIC, p, t, td, q)['height'], equal_nan=True)
