"""xp_wind_layers, xp_critical_angle, xp_corfidi_storm_motion and xp_significant_tornado_effective on the GPU: against the
NumPy restatement (tests/wind_layers_restatement.py), bit for bit across the forms of one request, across input kinds and
through the convenience functions, and the argument checks of the raw C ABI.

Tolerances.  The wind outputs and max_pressure: tests/test_gpu_kinematics.py::compare's rule, 1e-9 x scale plus one f32
spacing for f32 outputs, scale = max(1, largest |u|, |v| among the column's valid levels) for the winds and max(1, |ref|)
for max_pressure.  max_pressure is compared only where the restatement's strongest point stands out by more than 1e-9
(relative) from the second strongest: below that the choice between two points hangs on the last bits of hypot, and both are
the layer's strongest wind; at most 1 % of the layers may be left out (tests/test_wind_layers_cpu.py checks the seed).
Critical angle: the kernel and the restatement form a x b and a . b with the same IEEE operations, so the difference is that of
two atan2 implementations and the multiplication by 180 / pi, a few ulp of 180 (4e-14): 1e-12 degrees, plus one f32 spacing
for f32.  The Corfidi vectors and the effective-layer STP are sums, products and quotients in a fixed order: bit-equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import kinematics_restatement as K
from tests import wind_layers_restatement as R
from tests.test_gpu_kinematics import _f64, compare
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu
NAN = float('nan')
SEED = 7
LAYERS = [(R.HEIGHT, 0.0, 500.0), (R.HEIGHT, 0.0, 6000.0), (R.PRESSURE, 850.0, 300.0), (R.PRESSURE, NAN, 850.0)]
API_LAYERS = [{'top_height': 500.0}, {'bottom_height': 0.0, 'top_height': 6000.0}, {'bottom': 850.0, 'top': 300.0},
              {'bottom': None, 'top': 850.0}]
OFFSETS = (0.0, 1e-6, -1e-6, 2e-5, -2e-5)               # on the bound; inside np.isclose; outside (1e-5 itself is its edge)
WK = R.WIND_KEYS


def inputs(nlev, ncol, seed, dtype=np.float64, p0=None):
    """Pressure, u, v, height (nlev, ncol) as tests/test_gpu_kinematics.py::inputs: veering winds plus noise, pressure
    hydrostatic-like on the heights, p0 in 985 ... 1030 hPa (or `p0` everywhere); ~5 % missing values; an eighth of the columns
    truncated at 3 ... 7 km; a sixteenth with p0 in 800 ... 845 hPa (no surface -> 850 hPa layer).  In half of the columns one
    level is moved onto a bound of LAYERS or next to it by OFFSETS (relative, in pressure): the height for z0 + 500 m and
    z0 + 6000 m (a height offset of 8200 m x the relative one), the pressure itself for 850 and 300 hPa."""
    rng = np.random.default_rng(seed)
    z0 = rng.integers(0, 1500, ncol).astype(np.float64)        # (z0 + 500 is exact)
    z = z0 + np.vstack([np.zeros(ncol), np.cumsum(rng.uniform(80.0, 600.0, (nlev - 1, ncol)), axis=0)])
    cols = rng.permutation(ncol)
    targets = [('z', 500.0), ('z', 6000.0), ('p', 850.0), ('p', 300.0)]
    combos = [(t, o) for t in targets for o in OFFSETS]
    groups = np.array_split(cols[:ncol // 2], len(combos))
    for g, ((kind, t), off) in zip(groups, combos):
        if kind != 'z':
            continue
        for c in g:
            want = z0[c] + t + off * 8200.0
            k = int(np.argmin(np.abs(z[:, c] - want)))
            if k and k + 1 < nlev and z[k - 1, c] < want < z[k + 1, c]:
                z[k, c] = want
    h = z - z0
    psfc = rng.uniform(985.0, 1030.0, ncol) if p0 is None else np.full(ncol, float(p0))
    high = cols[ncol // 2 + ncol // 8: ncol // 2 + ncol // 8 + ncol // 16]
    if p0 is None:
        psfc[high] = rng.uniform(800.0, 845.0, high.size)
    p = psfc * np.exp(-h / rng.uniform(7600.0, 8800.0, ncol))
    for g, ((kind, t), off) in zip(groups, combos):
        if kind != 'p':
            continue
        for c in g:
            want = t * (1.0 + off)
            k = int(np.argmin(np.abs(p[:, c] - want)))
            if k and k + 1 < nlev and p[k - 1, c] > want > p[k + 1, c]:
                p[k, c] = want
    u = 5.0 + h * 2.5e-3 + rng.normal(0, 3, (nlev, ncol))
    v = -2.0 + h * 1.0e-3 + rng.normal(0, 3, (nlev, ncol))
    arrs = [p, u, v, z]
    miss = rng.random((nlev, ncol)) < 0.05
    which = rng.integers(0, 4, (nlev, ncol))
    for i, a in enumerate(arrs):
        a[miss & (which == i)] = np.nan
    for c in cols[ncol // 2: ncol // 2 + ncol // 8]:
        cut = z0[c] + rng.uniform(3000.0, 7000.0)
        for a in arrs:
            a[z[:, c] > cut, c] = np.nan
    return [a.astype(dtype) for a in arrs]


@functools.lru_cache(maxsize=None)
def case(dtype):
    """The inputs of the comparison at 48 x 6000 and the restatement on them, computed once per dtype and left unchanged."""
    arrs = inputs(48, 6000, SEED, dtype)
    ref = R.wind_layers_grid(*(a.astype(np.float64) for a in arrs), LAYERS)
    for a in list(arrs) + list(ref.values()):
        a.setflags(write=False)
    return arrs, ref


def wind_scale(p, u, v, z):
    ok = ~(np.isnan(p) | np.isnan(u) | np.isnan(v) | np.isnan(z))
    big = np.max(np.where(ok, np.maximum(np.abs(u), np.abs(v)), 0.0), axis=0).astype(np.float64)
    return np.maximum(1.0, big)[None, :] * np.ones((len(LAYERS), 1))


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def same_bits(a, b, keys, tag):
    for k in keys:
        assert np.array_equal(_np(a[k]), _np(b[k]), equal_nan=True), (tag, k)


# -- 1. against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_wind_layers_vs_restatement(dtype):
    (p, u, v, z), ref = case(dtype)
    got = xa.wind_layers(p, u, v, z, layers=API_LAYERS)
    assert got['mean_u'].dtype == dtype and got['mean_u'].shape == (4, 6000) and got['status'].shape == (6000,)
    f32 = dtype == np.float32
    tag = 'wind_layers %s' % np.dtype(dtype).name
    s = wind_scale(p, u, v, z)
    compare(got, ref, WK[:8], lambda k: s, f32, tag)
    # max_pressure, where the strongest point stands out
    has = ~np.isnan(ref['max_pressure'])
    clear = has & (ref['gap'] > 1e-9)
    left_out = 1.0 - clear.sum() / has.sum()
    print('%s: max_pressure compared on %d of %d layers (%.3f %% left out)' % (tag, clear.sum(), has.sum(), 100 * left_out))
    assert left_out <= 0.01
    g = _f64(got['max_pressure'])
    assert np.array_equal(np.isnan(g), ~has)
    tol = 1e-9 * np.maximum(1.0, np.abs(ref['max_pressure'][clear]))
    if f32:
        tol = tol + np.spacing(np.abs(ref['max_pressure'][clear]).astype(np.float32)).astype(np.float64)
    err = np.abs(g[clear] - ref['max_pressure'][clear])
    assert np.all(err <= tol), (tag, float(err.max()), np.argwhere(clear)[np.argmax(err - tol)])
    # the inputs exercise what they are meant to
    st = ref['status']
    nan_l = np.isnan(ref['mean_u'])
    assert (st == 0).sum() >= 3000 and (st == R.ST_NO_LAYER).sum() >= 700
    assert nan_l[3].sum() >= 300 and (nan_l[2] & ~nan_l[3]).sum() >= 300 and (nan_l[1] & ~nan_l[0]).sum() >= 50
    assert (ref['max_pressure'][2] == 300.0).sum() >= 100 and (ref['max_pressure'][3] < 1000.0).sum() >= 1000


def test_ordering_violations():
    p, u, v, z = inputs(30, 256, seed=9)
    z[4, :64] = z[3, :64]                               # equal heights
    p[6, 64:128] = p[5, 64:128] + 1.0                   # pressure rising
    for a in (p, u, v, z):
        a[:, 200:] = a[:, 200:][::-1]                   # upside down
    ref = R.wind_layers_grid(p, u, v, z, LAYERS)
    got = xa.wind_layers(p, u, v, z, layers=API_LAYERS)
    compare(got, ref, WK[:8], lambda k: wind_scale(p, u, v, z), False, 'wind_layers ordering')
    assert np.count_nonzero(ref['status'] & R.ST_BAD_HEIGHT) >= 90 and np.count_nonzero(ref['status'] & R.ST_BAD_PRESSURE) >= 90
    ref = R.wind_layers_grid(p, u, v, None, LAYERS[2:])                  # without height its order is not looked at
    got = xa.wind_layers(p, u, v, layers=API_LAYERS[2:])
    assert np.array_equal(got['status'], ref['status']) and not np.any(ref['status'] & R.ST_BAD_HEIGHT)
    assert np.array_equal(np.isnan(got['mean_u']), np.isnan(ref['mean_u']))


# -- 2. one request, several forms: bit for bit ---------------------------------------------------------------------------
def test_four_layers_equal_each_alone_and_any_subset_of_outputs():
    (p, u, v, z), _ = case(np.float64)
    many = xa.wind_layers(p, u, v, z, layers=API_LAYERS)
    for i, lay in enumerate(API_LAYERS):
        one = xa.wind_layers(p, u, v, z, layers=[lay])
        for k in WK:
            assert np.array_equal(many[k][i], one[k][0], equal_nan=True), (i, k)
        assert np.array_equal(one['status'] != 0, np.isnan(one['mean_u'][0]))
        assert np.all((many['status'] & R.ST_NO_LAYER) >= (one['status'] & R.ST_NO_LAYER))
    # without the strongest wind another instantiation runs: the same bits in what is left
    part = xa.wind_layers(p, u, v, z, layers=API_LAYERS[:3], want=('mean_u', 'shear_v', 'bottom_u'))
    for k in ('mean_u', 'shear_v', 'bottom_u'):
        assert np.array_equal(part[k], many[k][:3], equal_nan=True), k


def test_pressure_depth_equals_pressure_on_columns_of_one_p0():
    p, u, v, z = inputs(48, 1500, seed=11, p0=1000.0)
    base = ~np.isnan(p[0]) & ~np.isnan(u[0]) & ~np.isnan(v[0])           # the lowest valid level is level 0: p0 = 1000
    assert base.sum() >= 1200
    for d in (100.0, 150.0, 700.0):
        a = xa.wind_layers(p, u, v, layers=[('pressure_depth', None, d), ('pressure_depth', 900.0, d)])
        b = xa.wind_layers(p, u, v, layers=[('pressure', 1000.0, 1000.0 - d), ('pressure', 900.0, 900.0 - d)])
        for k in WK + ('status',):
            assert np.array_equal(a[k][..., base], b[k][..., base], equal_nan=True), (d, k)
        assert np.isfinite(a['mean_u'][0, base]).sum() >= 900
    mu, mv = xa.mean_pressure_weighted(p, u, v)                          # MetPy's default: the lowest 100 hPa
    su, sv = xa.bulk_shear(p, u, v, depth=150.0)
    a = xa.wind_layers(p, u, v, layers=[{'depth': 100.0}, {'depth': 150.0}])
    assert np.array_equal(mu, a['mean_u'][0], equal_nan=True) and np.array_equal(mv, a['mean_v'][0], equal_nan=True)
    assert np.array_equal(su, a['shear_u'][1], equal_nan=True) and np.array_equal(sv, a['shear_v'][1], equal_nan=True)


def test_bottom_wind_of_a_surface_based_layer_is_the_lowest_valid_level():
    (p, u, v, z), ref = case(np.float64)
    got = xa.wind_layers(p, u, v, z, layers=API_LAYERS)
    ok = ~(np.isnan(p) | np.isnan(u) | np.isnan(v) | np.isnan(z))
    first = np.argmax(ok, axis=0)
    cols = np.arange(p.shape[1])
    for i in (0, 1, 3):                                                   # the layers that begin at the lowest valid level
        has = ~np.isnan(got['bottom_u'][i])
        assert has.sum() >= 3000
        assert np.array_equal(got['bottom_u'][i][has], u[first, cols][has]) and np.array_equal(got['bottom_v'][i][has], v[first, cols][has])


@pytest.mark.parametrize('ncol', [1, 257])
def test_small_grids(ncol):
    (p, u, v, z), ref = case(np.float64)
    cols = np.arange(40, 40 + ncol)
    got = xa.wind_layers(*(np.ascontiguousarray(a[:, cols]) for a in (p, u, v, z)), layers=API_LAYERS)
    full = xa.wind_layers(p, u, v, z, layers=API_LAYERS)
    for k in WK + ('status',):
        assert np.array_equal(got[k], full[k][..., cols], equal_nan=True), k
    if ncol == 1:
        one = xa.wind_layers(*(a[:, 40] for a in (p, u, v, z)), layers=API_LAYERS)   # a single column, (nlev,)
        assert one['mean_u'].shape == (4,) and one['status'].shape == () and np.array_equal(one['mean_u'], got['mean_u'][:, 0], equal_nan=True)


# -- 3. input kinds -----------------------------------------------------------------------------------------------------------
def _abi_out(n, ncol, device):
    import torch
    make = (lambda dt: torch.empty(n, ncol, dtype=dt, device='cuda')) if device else None
    res = {k: (make(torch.float64) if device else np.empty((n, ncol))) for k in WK}
    res['status'] = torch.empty(ncol, dtype=torch.int32, device='cuda') if device else np.empty(ncol, np.int32)
    ptr = (lambda a: a.data_ptr()) if device else (lambda a: a.ctypes.data)
    out = L.WindLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE if device else L.XP_MEM_HOST, status=ptr(res['status']))
    for k in WK:
        for i in range(n):
            getattr(out, k)[i] = ptr(res[k][i])
    return out, res


def _abi_layers(layers=LAYERS):
    return (L.WindLayer * len(layers))(*[L.WindLayer(k, 0, b, t) for k, b, t in layers])


def test_input_kinds_and_strided_views():
    import torch
    (p, u, v, z), _ = case(np.float64)
    p, u, v, z = (np.ascontiguousarray(a[:, :1500]) for a in (p, u, v, z))
    ref = xa.wind_layers(p, u, v, z, layers=API_LAYERS)
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).cuda()):
        got = xa.wind_layers(*(conv(a) for a in (p, u, v, z)), layers=API_LAYERS)
        same_bits(got, ref, WK + ('status',), 'torch')
    assert got['mean_u'].is_cuda and got['status'].dtype == torch.int32
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev, ncol = p.shape
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (p, u, v, z)]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    out, res = _abi_out(4, ncol, True)
    L.check(lib.xp_wind_layers(*views, 4, _abi_layers(), out, None))
    torch.cuda.synchronize()
    same_bits(res, ref, WK + ('status',), 'strided')


# -- 4. the per-point kernels ------------------------------------------------------------------------------------------------
def test_per_point_kernels_vs_restatement():
    rng = np.random.default_rng(21)
    n = 10000
    x = rng.normal(0, 10, (6, n))
    x[:, :8] = [[3, 0, 3, 3, 0, 0, NAN, 1], [0, -2, 4, 4, 0, 1, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1], [-2, -2, -2, -2, -2, -2, -2, -2],
                [1, 5, 7, -0.5, 2, 1, 2, 1], [3, -2, 6, -4, 1, -2, 0, -2]]   # 90, 90, 0, 180 degrees; zero vectors; a NaN
    x[:, 8:400] = x[:, 8:400] * np.array([1, 1, 0, 0, 1, 1])[:, None]
    x[4:, 8:200] = x[:2, 8:200] * rng.uniform(-3, 3, 192)                   # parallel and antiparallel to the shear
    cape, cin = rng.uniform(0, 5000, n), -rng.uniform(0, 300, n)
    lcl, srh, shr = rng.uniform(300, 2600, n), rng.normal(150, 150, n), rng.uniform(0, 40, n)
    base = np.where(rng.random(n) < 0.3, rng.uniform(1, 900, n), 0.0)
    lcl[:6] = [1000.0, 2000.0, 999.999, 2000.001, NAN, 1500.0]
    shr[6:16] = [12.5, 30.0, 12.499999, 30.000001, NAN, 0.0, 12.500001, 29.999999, 20.0, 40.0]
    cin[16:24] = [-50.0, -200.0, -49.999, -200.001, 0.0, NAN, -50.001, -199.999]
    cape[24], srh[25], base[26:30] = NAN, NAN, [NAN, 0.0, -5.0, 1e-300]
    base[[4, 10, 21, 24, 25]] = [0.0, 0.0, 250.0, 0.0, 0.0]
    for dtype in (np.float64, np.float32):
        f32 = dtype == np.float32
        a = [r.astype(dtype) for r in x]
        ang = xa._per_point('xp_critical_angle', a, (), 1)[0]
        want = R.critical_angle(*a)
        assert ang.dtype == dtype and np.array_equal(np.isnan(ang), np.isnan(want))
        ok = ~np.isnan(want)
        tol = 1e-12 + (np.spacing(want[ok].astype(np.float32)).astype(np.float64) if f32 else 0.0)
        err = np.abs(ang[ok].astype(np.float64) - want[ok])
        print('critical angle %s: worst difference %.3g degrees' % (np.dtype(dtype).name, err.max()))
        assert np.all(err <= tol)
        if not f32:
            assert np.all(np.abs(ang[:4] - [90.0, 90.0, 0.0, 180.0]) <= 1e-12) and np.isnan(ang[4:7]).all()
            assert np.all((ang[8:200] == 0.0) | (ang[8:200] == 180.0) | (np.minimum(ang[8:200], 180 - ang[8:200]) < 1e-5))
            cosf = R.critical_angle_arccos(*a)
            mid = ok & (want > 1.0) & (want < 179.0)
            assert mid.sum() >= 9000 and np.max(np.abs(ang[mid] - cosf[mid])) <= 1e-9
        cor = xa._per_point('xp_corfidi_storm_motion', a[:4], (), 4)
        for g, w in zip(cor, R.corfidi_storm_motion(*a[:4])):
            assert g.dtype == dtype and np.array_equal(g, w.astype(dtype), equal_nan=True)
        s = [r.astype(dtype) for r in (cape, cin, lcl, srh, shr, base)]
        for b in (None, s[5]):
            stp = xa.significant_tornado_effective(*s[:5], base_height=b)
            want = R.significant_tornado_effective(*s[:5], base_height=b).astype(dtype)
            assert stp.dtype == dtype and np.array_equal(stp, want, equal_nan=True), (dtype, b is None)
    assert np.isnan(stp[[24, 25]]).all() and stp[21] == 0.0 and np.isnan(stp[4]) and np.isnan(stp[10]) and (stp == 0.0).sum() >= 2500
    # n = 1 (one lane of one workgroup) through all six products, against the restatements of this file and its neighbours
    one = [np.array([t]) for t in (2500.0, -60.0, 1200.0, 180.0, 22.0, 0.0)]
    w = [np.array([t]) for t in (3.0, -1.0, 6.0, 2.0, 9.0, -4.0)]
    assert np.array_equal(xa.significant_tornado_effective(*one[:5], base_height=one[5]), R.significant_tornado_effective(*one[:5], base_height=one[5]))
    assert np.array_equal(xa.significant_tornado(one[0], one[2], one[3], one[4]), K.significant_tornado(one[0], one[2], one[3], one[4]))
    assert np.array_equal(xa.supercell_composite(one[0], one[3], one[4]), K.supercell_composite(one[0], one[3], one[4]))
    assert abs(xa._per_point('xp_critical_angle', w, (), 1)[0][0] - R.critical_angle(*w)[0]) <= 1e-12
    for g, want in zip(xa._per_point('xp_corfidi_storm_motion', w[:4], (), 4), R.corfidi_storm_motion(*w[:4])):
        assert g.shape == (1,) and np.array_equal(g, want)
    ship = xa.significant_hail_parameter(*[np.array([t]) for t in (2000.0, 0.012, -7.0, 258.15, 20.0, 3000.0)])
    assert ship.shape == (1,) and np.isfinite(ship[0]) and ship[0] > 0.0
    # n = 0: XP_OK, and nothing is written -- the buffers handed over hold eight elements each
    lib = L.init(0)
    x, y = np.ones(8), np.full(8, -77.0)
    xd, yd = x.ctypes.data, y.ctypes.data
    for D in (L.XP_F64, L.XP_F32):
        H = L.XP_MEM_HOST
        assert lib.xp_significant_hail_parameter(0, D, H, xd, xd, xd, xd, xd, xd, yd, None) == L.XP_OK
        assert lib.xp_significant_tornado(0, D, H, xd, xd, xd, xd, yd, None) == L.XP_OK
        assert lib.xp_supercell_composite(0, D, H, xd, xd, xd, yd, None) == L.XP_OK
        assert lib.xp_critical_angle(0, D, H, xd, xd, xd, xd, xd, xd, yd, None) == L.XP_OK
        assert lib.xp_corfidi_storm_motion(0, D, H, xd, xd, xd, xd, yd, yd, yd, yd, None) == L.XP_OK
        assert lib.xp_significant_tornado_effective(0, D, H, xd, xd, xd, xd, xd, xd, yd, None) == L.XP_OK
        assert np.all(y == -77.0) and np.all(x == 1.0)


# -- 5. the chains, on the device ----------------------------------------------------------------------------------------------
def test_convenience_chain_on_the_device():
    import torch
    (p, u, v, z), ref = case(np.float64)
    n = 3000
    hp, hu, hv, hz = (np.ascontiguousarray(a[:, :n]) for a in (p, u, v, z))
    dp, du, dv, dz = (torch.from_numpy(a).cuda() for a in (hp, hu, hv, hz))
    bm = xa.bunkers_storm_motion(dp, du, dv, dz)
    ang = xa.critical_angle(dp, du, dv, dz, bm['right_u'], bm['right_v'])
    cor = xa.corfidi_storm_motion(dp, du, dv)
    assert ang.is_cuda and ang.shape == (n,) and cor['downwind_u'].is_cuda
    r_bm = K.bunkers_grid(hp, hu, hv, hz)
    sub = {k: ref[k][:, :n] for k in WK}
    want = R.critical_angle(sub['shear_u'][0], sub['shear_v'][0], sub['bottom_u'][0], sub['bottom_v'][0], r_bm['right_u'], r_bm['right_v'])
    got = _np(ang)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    # the angle of two vectors known to 1e-9 x scale each: 1e-9 x scale / |vector| radians apiece
    s = wind_scale(hp, hu, hv, hz)[0]
    a_len = np.hypot(sub['shear_u'][0], sub['shear_v'][0])
    b_len = np.hypot(r_bm['right_u'] - sub['bottom_u'][0], r_bm['right_v'] - sub['bottom_v'][0])
    tol = 1e-12 + np.degrees(2e-9 * s[ok] * (1.0 / a_len[ok] + 1.0 / b_len[ok]))
    err = np.abs(got[ok] - want[ok])
    print('critical angle chain: %d columns, worst difference %.3g degrees' % (ok.sum(), err.max()))
    assert ok.sum() >= 1500 and np.all(err <= tol)
    # Corfidi with the jet found below 850 hPa: the vectors of the restatement where its jet is unambiguous (a reference of
    # its own: the call passes no height, so a level whose height is missing still counts)
    r_wl = R.wind_layers_grid(hp, hu, hv, None, LAYERS[2:])
    w = R.corfidi_storm_motion(r_wl['mean_u'][0], r_wl['mean_v'][0], r_wl['max_u'][1], r_wl['max_v'][1])
    clear = r_wl['gap'][1] > 1e-9
    assert np.array_equal(_np(cor['status']), r_wl['status'])
    for g, r in zip((cor[k] for k in ('upwind_u', 'upwind_v', 'downwind_u', 'downwind_v')), w):
        g = _np(g)
        assert np.array_equal(np.isnan(g), np.isnan(r))
        ok = ~np.isnan(r) & clear
        assert ok.sum() >= 1500 and np.all(np.abs(g[ok] - r[ok]) <= 4e-9 * s[ok])      # mean, jet: 1e-9 x scale each, mean twice
    # a jet passed in: one layer, and the per-point kernel on it
    cor2 = xa.corfidi_storm_motion(dp, du, dv, llj_u=torch.full((n,), 3.0, device='cuda', dtype=torch.float64), llj_v=-2.0)
    mean = xa.wind_layers(dp, du, dv, layers=[{'bottom': 850.0, 'top': 300.0}], want=('mean_u', 'mean_v'))
    w = R.corfidi_storm_motion(_np(mean['mean_u'][0]), _np(mean['mean_v'][0]), 3.0, -2.0)
    for g, r in zip((cor2[k] for k in ('upwind_u', 'upwind_v', 'downwind_u', 'downwind_v')), w):
        assert np.array_equal(_np(g), r, equal_nan=True)


def test_recipe_up_to_the_effective_layer_stp():
    """The README chain with the effective-layer STP at its end, on the device: mixed-layer CAPE / CIN / LCL ->
    interp_level(height) at the LCL -> effective_inflow_layer -> bunkers_storm_motion -> storm_relative_helicity_layers
    (ESRH over the inflow layer, EBWD up to half the equilibrium-level height) -> significant_tornado_effective with the
    layer's base_height.  Every link but the last has its own test; the last is held to the restatement on the very arrays
    the device handed it, bit for bit."""
    import torch
    from tests.test_gpu_effective_layer import heights
    n, nlev = 1000, 40
    p, t, td = synth.columns(nlev=nlev, ncol=n, seed=41, dtype=np.float64)
    z = heights(p)
    rng = np.random.default_rng(42)
    h = z - z[0]
    u = 5.0 + h * 2.5e-3 + rng.normal(0, 3, (nlev, n))
    v = -2.0 + h * 1.0e-3 + rng.normal(0, 3, (nlev, n))
    p, t, td, z, u, v = (torch.from_numpy(a).cuda() for a in (p, t, td, z, u, v))
    ml = xa.cape_cin_columns(p, t, td, parcel='mixed_layer', depth=100, moist='exact')
    mu = xa.cape_cin_columns(p, t, td, parcel='most_unstable', moist='exact')
    lcl_h = xa.interp_level(p, z, ml['lcl_pressure'], log=True) - z[0]
    z_el = xa.interp_level(p, z, mu['el_pressure'], log=True) - z[0]
    eff = xa.effective_inflow_layer(p, t, td, height=z)
    bm = xa.bunkers_storm_motion(p, u, v, z)
    half = eff['base_height'] + 0.5 * (z_el - eff['base_height'])
    lay = xa.storm_relative_helicity_layers(z, u, v, eff['base_height'], [eff['top_height'], half],
                                            storm_u=bm['right_u'], storm_v=bm['right_v'])
    args = (ml['cape'], ml['cin'], lcl_h, lay['total'][0], lay['shear_magnitude'][1])
    stp = xa.significant_tornado_effective(*args, base_height=eff['base_height'])
    assert stp.is_cuda and stp.shape == (n,)
    want = R.significant_tornado_effective(*(_np(a) for a in args), base_height=_np(eff['base_height']))
    got = _np(stp)
    assert np.array_equal(got, want, equal_nan=True)
    elevated = _np(eff['base_height']) > 0
    print('effective STP: %d finite, %d non-zero, %d elevated inflow layers' % (np.isfinite(got).sum(), (got != 0).sum(), elevated.sum()))
    assert np.isfinite(got).sum() >= 300 and np.count_nonzero(got[np.isfinite(got)]) >= 10 and np.all(got[elevated] == 0.0)


# -- 6. the raw ABI's argument checks --------------------------------------------------------------------------------------------
def test_raw_abi_errors():
    lib = L.init(0)
    p, u, v, z = (np.ascontiguousarray(a) for a in inputs(30, 8, seed=2))
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 30, 8, 8, 1) for a in (p, u, v, z)]
    short = L.View(z.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 30, 4, 4, 1)
    f32 = L.View(z.ctypes.data, L.XP_F32, L.XP_MEM_HOST, 30, 8, 8, 1)
    out, res = _abi_out(4, 8, False)

    def call(layers=LAYERS, n=None, vs=views, o=out, arr=True):
        for a in res.values():
            a[...] = -77
        rc = lib.xp_wind_layers(*vs, len(layers) if n is None else n, _abi_layers(layers) if arr else None, o, None)
        if rc != L.XP_OK:
            assert all(np.all(a == -77) for a in res.values()), 'outputs touched'
        return rc
    assert call() == L.XP_OK and np.isfinite(res['mean_u']).any() and not np.any(res['status'] == -77)
    assert call(LAYERS[2:], vs=views[:3] + [None]) == L.XP_OK and np.all(res['mean_u'][2:] == -77)
    inf = float('inf')
    bad = [(dict(layers=LAYERS[:1], vs=views[:3] + [None]), 'needs height'), (dict(n=0), 'nlayer'),
           (dict(layers=LAYERS + LAYERS[:1], n=5), 'nlayer'), (dict(arr=False), 'null'),
           (dict(layers=[(R.PRESSURE_DEPTH, NAN, 0.0)]), 'depth'), (dict(layers=[(R.PRESSURE_DEPTH, 900.0, -10.0)]), 'depth'),
           (dict(layers=[(R.HEIGHT, 500.0, 500.0)]), 'depth'), (dict(layers=[(R.HEIGHT, 600.0, 500.0)]), 'depth'),
           (dict(layers=[(R.HEIGHT, -1.0, 500.0)]), 'bottom'), (dict(layers=[(R.PRESSURE, 850.0, NAN)]), 'top'),
           (dict(layers=[(R.PRESSURE, 850.0, inf)]), 'top'), (dict(layers=[(R.HEIGHT, 0.0, inf)]), 'top'),
           (dict(layers=[(R.PRESSURE, inf, 300.0)]), 'bottom'), (dict(layers=[(R.PRESSURE, -inf, 300.0)]), 'bottom'),
           (dict(layers=LAYERS[:3] + [(3, 0.0, 1.0)]), 'kind'), (dict(layers=[(-1, 0.0, 1.0)]), 'kind'),
           (dict(vs=views[:3] + [short]), 'differ'), (dict(vs=[views[0], short, views[2], views[3]]), 'differ'),
           (dict(vs=views[:3] + [f32]), 'differ'), (dict(o=None), 'out'),
           (dict(o=L.WindLayersOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST, status=res['status'].ctypes.data)), 'out'),
           (dict(o=L.WindLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, status=res['status'].ctypes.data)), 'out')]
    for kw, word in bad:
        assert call(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())
    x, y = np.ones(8), np.full(8, -77.0)
    xd, yd = x.ctypes.data, y.ctypes.data
    H, D = L.XP_MEM_HOST, L.XP_F64
    assert lib.xp_critical_angle(8, D, H, xd, xd, xd, xd, xd, None, yd, None) == L.XP_E_ARG
    assert lib.xp_critical_angle(8, D, H, xd, xd, xd, xd, xd, xd, None, None) == L.XP_E_ARG
    assert lib.xp_critical_angle(8, 7, H, xd, xd, xd, xd, xd, xd, yd, None) == L.XP_E_ARG
    assert lib.xp_corfidi_storm_motion(8, D, H, xd, xd, None, xd, yd, yd, yd, yd, None) == L.XP_E_ARG
    assert lib.xp_corfidi_storm_motion(-1, D, H, xd, xd, xd, xd, yd, yd, yd, yd, None) == L.XP_E_ARG
    assert lib.xp_significant_tornado_effective(8, D, H, xd, xd, xd, xd, None, None, yd, None) == L.XP_E_ARG
    assert lib.xp_significant_tornado_effective(8, 2, H, xd, xd, xd, xd, xd, None, yd, None) == L.XP_E_ARG
    assert np.all(y == -77.0)
    assert lib.xp_corfidi_storm_motion(8, D, H, xd, xd, xd, xd, None, None, yd, None, None) == L.XP_OK and np.all(y == 1.0)
    assert lib.xp_significant_tornado_effective(8, D, H, xd, xd, xd, xd, xd, None, yd, None) == L.XP_OK and np.all(y == 0.0)
