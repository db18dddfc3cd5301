"""Storm motion, helicity and the composites on the device (xp_bunkers_storm_motion, xp_storm_relative_helicity,
xp_significant_tornado, xp_supercell_composite) against the NumPy restatement tests/kinematics_restatement.py, across
input kinds, and their argument checks."""
from ctypes import c_double as C_double

import numpy as np
import pytest

from tests import kinematics_restatement as R
from tests.test_kinematics_cpu import circular_hodograph
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa

pytestmark = pytest.mark.gpu
BK = R.BUNKERS_KEYS
DEPTHS = [500.0, 1000.0, 3000.0, 6000.0]
WORST = {}


def inputs(nlev, ncol, seed, dtype=np.float64):
    """Pressure, u, v, height (nlev, ncol): winds as in test_gpu_indices._bundle_inputs (veering with height plus noise),
    pressure hydrostatic-like on the heights; ~5 % missing values; an eighth of the columns truncated at 3 ... 7 km; levels
    moved onto and next to the Bunkers bounds (z0 + 500, 5500, 6000 m) and the SRH tops (1, 3 km above the surface)."""
    rng = np.random.default_rng(seed)
    z0 = rng.integers(0, 1500, ncol).astype(np.float64)        # (z0 + 500 and (z0 + 1000) - z0 are exact)
    z = z0 + np.vstack([np.zeros(ncol), np.cumsum(rng.uniform(80.0, 600.0, (nlev - 1, ncol)), axis=0)])
    cols = rng.permutation(ncol)
    groups = np.array_split(cols[:ncol // 2], 10)
    targets = [500.0, 5500.0, 6000.0, 1000.0, 3000.0]
    for g, (t, off) in zip(groups, [(t, o) for t in targets for o in (0.0, None)]):
        for c in g:
            o = off if off is not None else rng.choice([0.02, -0.02, 1e-6, -1e-6, 2.0, -2.0])
            want = z0[c] + t + o
            k = int(np.argmin(np.abs(z[:, c] - want)))
            lo = z[k - 1, c] if k else -np.inf
            hi = z[k + 1, c] if k + 1 < nlev else np.inf
            if k and lo < want < hi:
                z[k, c] = want
    h = z - z0
    p = rng.uniform(985.0, 1030.0, ncol) * np.exp(-h / rng.uniform(7600.0, 8800.0, ncol))
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


def _f64(a):
    return np.asarray(a.cpu() if hasattr(a, 'cpu') else a, dtype=np.float64)


def compare(got, ref, keys, scale, f32, tag):
    assert np.array_equal(np.asarray(got['status']), ref['status']), (tag, np.nonzero(np.asarray(got['status']) != ref['status']))
    worst = 0.0
    for k in keys:
        g, r = _f64(got[k]), ref[k]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, k, np.argwhere(np.isnan(g) != np.isnan(r))[:5])
        ok = ~np.isnan(r)
        s = scale(k)[ok] if callable(scale) else np.maximum(1.0, np.abs(r[ok]))
        tol = 1e-9 * s
        if f32:
            tol = tol + np.spacing(np.abs(r[ok]).astype(np.float32)).astype(np.float64)
        err = np.abs(g[ok] - r[ok])
        assert np.all(err <= tol), (tag, k, float(err.max()), np.argwhere(ok)[np.argmax(err - tol)])
        if ok.any():
            worst = max(worst, float(np.max(err / s)))
    WORST[tag] = max(WORST.get(tag, 0.0), worst)
    print('%s: worst relative difference %.3g' % (tag, worst))


def _srh_scale(ref):
    s = np.maximum(1.0, np.abs(ref['positive']) + np.abs(ref['negative']))
    return lambda k: s


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_bunkers_vs_restatement(dtype):
    p, u, v, z = inputs(40, 3000, seed=3, dtype=dtype)
    got = xa.bunkers_storm_motion(p, u, v, z)
    assert np.asarray(got['mean_u']).dtype == dtype
    ref = R.bunkers_grid(*(a.astype(np.float64) for a in (p, u, v, z)))
    compare(got, ref, BK, None, dtype == np.float32, 'bunkers %s' % np.dtype(dtype).name)
    st = ref['status']
    assert (st == 0).sum() >= 2000 and (st == R.ST_NO_LAYER).sum() >= 200


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_srh_vs_restatement(dtype):
    p, u, v, z = inputs(40, 3000, seed=4, dtype=dtype)
    rng = np.random.default_rng(5)
    cu, cv = rng.normal(8, 4, 3000).astype(dtype), rng.normal(2, 4, 3000).astype(dtype)
    for bottom, kw in ((0.0, {}), (250.0, {}), (0.0, {'surface_u': rng.normal(2, 2, 3000).astype(dtype),
                                                      'surface_v': rng.normal(0, 2, 3000).astype(dtype)})):
        if kw:
            z = z - np.nanmin(z, axis=0) + 10.0         # heights above the surface for the surface-wind form
        got = xa.storm_relative_helicity(z, u, v, DEPTHS, bottom=bottom, storm_u=cu, storm_v=cv, **kw)
        ref = R.srh_grid(*(a.astype(np.float64) for a in (z, u, v)), DEPTHS, bottom, cu.astype(np.float64),
                         cv.astype(np.float64), **{k: x.astype(np.float64) for k, x in kw.items()})
        compare(got, ref, R.SRH_KEYS, _srh_scale(ref), dtype == np.float32, 'srh %s' % np.dtype(dtype).name)
        assert (ref['status'] == 0).sum() >= 1000 and (ref['status'] == R.ST_NO_LAYER).sum() >= 100


def test_ordering_violations_on_the_device():
    p, u, v, z = inputs(30, 256, seed=9)
    z[4, :64] = z[3, :64]                               # equal heights
    p[6, 64:128] = p[5, 64:128] + 1.0                   # pressure rising
    for a in (p, u, v, z):
        a[:, 200:] = a[:, 200:][::-1]                   # upside down
    got = xa.bunkers_storm_motion(p, u, v, z)
    ref = R.bunkers_grid(p, u, v, z)
    compare(got, ref, BK, None, False, 'bunkers ordering')
    assert np.count_nonzero(ref['status'] & R.ST_BAD_HEIGHT) >= 90 and np.count_nonzero(ref['status'] & R.ST_BAD_PRESSURE) >= 90
    got = xa.storm_relative_helicity(z, u, v, DEPTHS[:2])
    ref = R.srh_grid(z, u, v, DEPTHS[:2])
    compare(got, ref, R.SRH_KEYS, _srh_scale(ref), False, 'srh ordering')


@pytest.mark.parametrize('clockwise', [True, False])
def test_analytic_columns(clockwise):
    n, rad, turn = 12, 10.0, np.pi / 2
    h, u, v = circular_hodograph(n, rad, turn, clockwise=clockwise)
    got = xa.storm_relative_helicity(h, u, v, n * 250.0, storm_u=3.0, storm_v=-2.0)
    want = n * rad ** 2 * np.sin(turn / n) * (1 if clockwise else -1)
    assert int(got['status']) == 0 and abs(float(got['total']) - want) < 1e-9 * abs(want)
    assert float(got['negative' if clockwise else 'positive']) == 0.0
    hs = np.array([0., 150., 400., 800., 1300., 2100., 3000., 4200.])
    got = xa.storm_relative_helicity(hs, 4e-3 * hs, 0 * hs, 3000.0, storm_u=4.0, storm_v=3.0)
    assert abs(float(got['total']) - (-3.0 * 12.0)) < 1e-12
    z = 120.0 + np.linspace(0.0, 12000.0, 30)
    p = 1010.0 * np.exp(-(z - 120.0) / 8200.0)
    r = xa.bunkers_storm_motion(p, 2.0 + 3e-3 * z, np.full_like(z, 1.5), z)
    assert abs(float(r['right_v']) - (float(r['mean_v']) - 7.5)) < 1e-12
    assert abs(float(r['left_v']) - (float(r['mean_v']) + 7.5)) < 1e-12
    r = xa.bunkers_storm_motion(p, np.full_like(z, 7.25), np.full_like(z, -3.5), z)
    assert abs(float(r['mean_u']) - 7.25) < 1e-12 and np.isnan(float(r['right_u'])) and int(r['status']) == 0


def test_input_kinds_and_strided_views():
    import torch
    p, u, v, z = inputs(24, 600, seed=6)
    ref_b = xa.bunkers_storm_motion(p, u, v, z)
    ref_s = xa.storm_relative_helicity(z, u, v, [1000.0, 3000.0], storm_u=ref_b['right_u'], storm_v=ref_b['right_v'])
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).cuda()):
        b = xa.bunkers_storm_motion(*(conv(a) for a in (p, u, v, z)))
        s = xa.storm_relative_helicity(*(conv(a) for a in (z, u, v)), [1000.0, 3000.0], storm_u=b['right_u'],
                                       storm_v=b['right_v'])
        for k in BK + ('status',):
            assert np.array_equal(np.asarray(b[k].cpu() if hasattr(b[k], 'cpu') else b[k]), ref_b[k], equal_nan=True), k
        for k in R.SRH_KEYS + ('status',):
            assert np.array_equal(np.asarray(s[k].cpu() if hasattr(s[k], 'cpu') else s[k]), ref_s[k], equal_nan=True), k
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev, ncol = p.shape
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (p, u, v, z)]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    ob = {k: torch.empty(ncol, dtype=torch.int32 if k == 'status' else torch.float64, device='cuda') for k in L.STORM_MOTION_OUT}
    o = L.StormMotionOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, **{k: t.data_ptr() for k, t in ob.items()})
    L.check(lib.xp_bunkers_storm_motion(*views, o, None))
    os_ = {k: torch.empty(2, ncol, dtype=torch.float64, device='cuda') for k in L.SRH_OUT}
    st = torch.empty(ncol, dtype=torch.int32, device='cuda')
    so = L.SrhOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, status=st.data_ptr())
    for k in L.SRH_OUT:
        for i in range(2):
            getattr(so, k)[i] = os_[k][i].data_ptr()
    cu, cv = (torch.from_numpy(np.ascontiguousarray(ref_b[k])).cuda() for k in ('right_u', 'right_v'))
    L.check(lib.xp_storm_relative_helicity(views[3], views[1], views[2], None, None, cu.data_ptr(), cv.data_ptr(), 0.0, 2,
                                           (C_double * 2)(1000.0, 3000.0), so, None))
    torch.cuda.synchronize()
    for k in BK + ('status',):
        assert np.array_equal(ob[k].cpu().numpy(), ref_b[k], equal_nan=True), k
    for k in R.SRH_KEYS:
        assert np.array_equal(os_[k].cpu().numpy(), ref_s[k], equal_nan=True), k
    assert np.array_equal(st.cpu().numpy(), ref_s['status'])


def test_several_depths_equal_separate_calls():
    p, u, v, z = inputs(40, 2000, seed=12)
    for kw in ({}, {'bottom': 300.0, 'storm_u': 7.0, 'storm_v': 1.5}):
        many = xa.storm_relative_helicity(z, u, v, DEPTHS, **kw)
        for i, d in enumerate(DEPTHS):
            one = xa.storm_relative_helicity(z, u, v, d, **kw)
            for k in R.SRH_KEYS:
                assert np.array_equal(many[k][i], one[k], equal_nan=True), (kw, d, k)
            lone = one['status'] & R.ST_NO_LAYER
            assert np.all((many['status'] & R.ST_NO_LAYER) >= lone)


def test_composites_vs_restatement():
    rng = np.random.default_rng(2)
    n = 4096
    cape = rng.uniform(0, 5000, n)
    lcl = rng.uniform(300, 2600, n)
    srh = rng.normal(150, 150, n)
    shear = rng.uniform(0, 40, n)
    lcl[:6] = [1000.0, 2000.0, 999.999, 2000.001, np.nan, 1500.0]
    shear[6:16] = [10.0, 12.5, 20.0, 30.0, 9.999999, 12.499999, 20.000001, 30.000001, np.nan, 0.0]
    cape[16], srh[17] = np.nan, np.nan
    for dtype in (np.float64, np.float32):
        a = [x.astype(dtype) for x in (cape, lcl, srh, shear)]
        stp = xa.significant_tornado(*a)
        scp = xa.supercell_composite(a[0], a[2], a[3])
        assert stp.dtype == dtype and scp.dtype == dtype
        want_stp = R.significant_tornado(*a).astype(dtype)
        want_scp = R.supercell_composite(a[0], a[2], a[3]).astype(dtype)
        assert np.array_equal(stp, want_stp, equal_nan=True) and np.array_equal(scp, want_scp, equal_nan=True), dtype
    assert np.isnan(stp[[4, 14, 16, 17]]).all() and stp[15] == 0.0 and np.isnan(scp[[14, 16, 17]]).all()


def test_raw_abi_errors():
    lib = L.init(0)
    p, u, v, z = (np.ascontiguousarray(a) for a in inputs(30, 8, seed=2))
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 30, 8, 8, 1) for a in (p, u, v, z)]
    short = L.View(z.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 30, 4, 4, 1)
    ru = np.empty(8)
    pos = np.empty(8)
    sfc = np.zeros(8)
    good_b = dict(dtype=L.XP_F64, mem=L.XP_MEM_HOST, right_u=ru.ctypes.data)

    def bunkers(out=True, vs=views, **o):
        return lib.xp_bunkers_storm_motion(*vs, L.StormMotionOut(**{**good_b, **o}) if out else None, None)
    assert bunkers() == L.XP_OK and np.isfinite(ru).any()
    for kw in ({'out': False}, {'dtype': L.XP_F32}, {'mem': L.XP_MEM_DEVICE}, {'vs': views[:3] + [short]}):
        assert bunkers(**kw) == L.XP_E_ARG, kw

    def srh(out=True, bottom=0.0, nd=1, depth=(1000.0,), su=None, sv=None, zv=views[3], **o):
        so = L.SrhOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
        so.positive[0] = pos.ctypes.data
        for k, x in o.items():
            setattr(so, k, x)
        d = (C_double * max(1, len(depth)))(*depth)
        return lib.xp_storm_relative_helicity(zv, views[1], views[2], su, sv, None, None, bottom, nd, d,
                                              so if out else None, None)
    assert srh() == L.XP_OK and np.isfinite(pos).any()
    assert srh(nd=4, depth=(500.0, 1000.0, 3000.0, 6000.0)) == L.XP_OK
    assert srh(su=sfc.ctypes.data, sv=sfc.ctypes.data) == L.XP_OK
    for kw, word in (({'out': False}, 'out'), ({'dtype': L.XP_F32}, 'out'), ({'mem': L.XP_MEM_DEVICE}, 'out'),
                     ({'zv': short}, 'differ'), ({'nd': 0}, 'ndepth'), ({'nd': 5, 'depth': (1e3,) * 5}, 'ndepth'),
                     ({'depth': (0.0,)}, 'depth'), ({'depth': (-5.0,)}, 'depth'), ({'depth': (float('nan'),)}, 'depth'),
                     ({'depth': (float('inf'),)}, 'depth'), ({'nd': 2, 'depth': (1e3, float('nan'))}, 'depth'),
                     ({'bottom': -1.0}, 'bottom'), ({'bottom': float('nan')}, 'bottom'), ({'bottom': float('inf')}, 'bottom'),
                     ({'su': sfc.ctypes.data}, 'surface'), ({'sv': sfc.ctypes.data}, 'surface')):
        assert srh(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())
    x = np.ones(8)
    assert lib.xp_significant_tornado(8, L.XP_F64, L.XP_MEM_HOST, x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                      None, x.ctypes.data, None) == L.XP_E_ARG
    assert lib.xp_supercell_composite(8, 7, L.XP_MEM_HOST, x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                      x.ctypes.data, None) == L.XP_E_ARG
    assert lib.xp_supercell_composite(-1, L.XP_F64, L.XP_MEM_HOST, x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                      x.ctypes.data, None) == L.XP_E_ARG


def grid_torch(nlev, ncol, seed):
    """A large f32 grid built on the device: heights from random layer depths, pressure on them, veering winds."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    dz = 80.0 + 520.0 * torch.rand(nlev - 1, ncol, device='cuda', generator=g)
    z0 = 1500.0 * torch.rand(1, ncol, device='cuda', generator=g)
    h = torch.cat([torch.zeros(1, ncol, device='cuda'), torch.cumsum(dz, 0)])
    p = (985.0 + 45.0 * torch.rand(1, ncol, device='cuda', generator=g)) * torch.exp(-h / 8200.0)
    u = 5.0 + h * 2.5e-3 + 3.0 * torch.randn(nlev, ncol, device='cuda', generator=g)
    v = -2.0 + h * 1.0e-3 + 3.0 * torch.randn(nlev, ncol, device='cuda', generator=g)
    return p.float(), u.float(), v.float(), (h + z0).float()


def test_large_grid_40_levels_by_4mi_columns():
    import torch
    ncol = 1 << 22
    p, u, v, z = grid_torch(40, ncol, seed=1)
    b = xa.bunkers_storm_motion(p, u, v, z)
    s = xa.storm_relative_helicity(z, u, v, [1000.0, 3000.0], storm_u=b['right_u'], storm_v=b['right_v'])
    torch.cuda.synchronize()
    assert b['mean_u'].dtype == torch.float32 and s['total'].shape == (2, ncol)
    assert int((b['status'] == 0).sum()) >= 0.99 * ncol and bool(torch.isfinite(s['total']).any())
    cols = np.sort(np.random.default_rng(0).choice(ncol, 2000, replace=False))
    idx = torch.from_numpy(cols).cuda()
    hp, hu, hv, hz = (x[:, idx].cpu().numpy().astype(np.float64) for x in (p, u, v, z))
    gb = {k: b[k][idx].cpu().numpy() for k in BK + ('status',)}
    ref_b = R.bunkers_grid(hp, hu, hv, hz)
    compare(gb, ref_b, BK, None, True, 'bunkers large f32')
    cu, cv = gb['right_u'].astype(np.float64), gb['right_v'].astype(np.float64)
    gs = {k: s[k][:, idx].cpu().numpy() for k in R.SRH_KEYS}
    gs['status'] = s['status'][idx].cpu().numpy()
    ref_s = R.srh_grid(hz, hu, hv, [1000.0, 3000.0], 0.0, cu, cv)
    compare(gs, ref_s, R.SRH_KEYS, _srh_scale(ref_s), True, 'srh large f32')
