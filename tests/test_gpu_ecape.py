"""Entraining CAPE on the device: xp_ncape against the NumPy restatement tests/ecape_restatement.py on bounds drawn here,
xp_ecape against the restated formula, the chain numpy_api.ecape against its six separate calls, the input kinds, the raw
ABI's argument checks, and one full-size grid."""
import functools

import numpy as np
import pytest

from tests import ecape_restatement as R
from tests.test_gpu_dcape import inputs
from tests.test_gpu_layer_cape import heights
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu
NAN = float('nan')
FLOATS = ('ncape', 'lfc_height', 'el_height')
CLASSES = ('between', 'one_interval', 'on_levels', 'lfc_below_p0', 'el_above_top', 'el_nan', 'lfc_nan', 'inverted')


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def draw_bounds(p, t, td, z, seed):
    """L and E per column, drawn from the column's own valid levels: column c gets CLASSES[c % 8].  Columns with fewer than
    four valid levels get 900 / 300 hPa whatever their class."""
    rng = np.random.default_rng(seed)
    ncol = p.shape[1]
    lfc, el = np.full(ncol, 900.0), np.full(ncol, 300.0)
    p64 = p.astype(np.float64)
    ok = ~(np.isnan(p) | np.isnan(t) | np.isnan(td) | np.isnan(z))
    for c in range(ncol):
        pv = p64[ok[:, c], c]
        kind = CLASSES[c % 8]
        if pv.size >= 4:
            i = int(rng.integers(0, pv.size - 2))
            j = int(rng.integers(i + 1, pv.size - 1))
            a, b = rng.uniform(0.1, 0.9, 2)
            lfc[c], el[c] = a * pv[i] + (1 - a) * pv[i + 1], b * pv[j] + (1 - b) * pv[j + 1]
            if kind == 'one_interval':
                lfc[c], el[c] = 0.8 * pv[i] + 0.2 * pv[i + 1], 0.3 * pv[i] + 0.7 * pv[i + 1]
            elif kind == 'on_levels':
                lfc[c], el[c] = pv[i], pv[j]
            elif kind == 'lfc_below_p0':
                lfc[c] = pv[0] + 25.0
            elif kind == 'el_above_top':
                el[c] = pv[-1] - 10.0
        if kind == 'el_nan':
            el[c] = NAN
        elif kind == 'lfc_nan':
            lfc[c] = NAN
        elif kind == 'inverted':
            el[c] = lfc[c] if c % 16 == 7 else lfc[c] + 40.0
    return lfc.astype(p.dtype), el.astype(p.dtype)


@functools.lru_cache(maxsize=None)
def case(nlev, dtype):
    """The inputs of the comparison at nlev x 333, their bounds and the restatement on them, computed once and left unchanged."""
    p, t, td = inputs(nlev, 333, seed=nlev, dtype=dtype)
    z = heights(p.astype(np.float64)).astype(dtype)
    lfc, el = draw_bounds(p, t, td, z, seed=nlev + 1)
    ref = R.grid(*(a.astype(np.float64) for a in (p, t, td, z, lfc, el)))
    for a in (p, t, td, z, lfc, el) + tuple(ref.values()):
        a.setflags(write=False)
    return (p, t, td, z, lfc, el), ref


def compare(got, ref, f32, tag):
    """Status and NaN pattern equal in every column; ncape to 1e-6 J/kg + 1e-9 relative, the heights to 1e-8 m; float32 outputs
    one float32 spacing more."""
    assert np.array_equal(_np(got['status']), ref['status']), (tag, np.argwhere(_np(got['status']) != ref['status'])[:5])
    for k in FLOATS:
        g, r = _np(got[k]).astype(np.float64), ref[k]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, k, np.argwhere(np.isnan(g) != np.isnan(r))[:5])
        ok = ~np.isnan(r)
        tol = (1e-6 + 1e-9 * np.abs(r[ok])) if k == 'ncape' else np.full(ok.sum(), 1e-8)
        if f32:
            tol = tol + np.spacing(np.abs(r[ok]).astype(np.float32)).astype(np.float64)
        err = np.abs(g[ok] - r[ok])
        print('%s %s: %d values, worst difference %.3g' % (tag, k, ok.sum(), err.max() if ok.any() else 0.0))
        assert np.all(err <= tol), (tag, k, float(err.max()), np.argwhere(ok)[np.argmax(err - tol)])


# -- 1. NCAPE against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('nlev', [12, 40])
def test_ncape_vs_restatement(nlev, dtype):
    args, ref = case(nlev, dtype)
    got = xa.ncape(*args)
    assert got['ncape'].dtype == dtype and got['ncape'].shape == (333,) and got['status'].dtype == np.int32
    compare(got, ref, dtype == np.float32, 'ncape %d %s' % (nlev, np.dtype(dtype).name))
    st = ref['status']
    assert np.isfinite(ref['ncape']).sum() >= 200 and (st == R.ST_NO_LAYER).sum() >= 30
    # the classes are what they claim to be
    c = np.arange(333)
    assert np.all(ref['ncape'][(c % 8 == 6)] == 0.0) and np.all(st[c % 8 == 7] == R.ST_NO_LAYER)
    assert np.count_nonzero(ref['lfc_height'][c % 8 == 3] == 0.0) >= 30
    assert np.count_nonzero(np.isfinite(ref['ncape']) & (ref['ncape'] != 0.0)) >= 200


def hand_built(dtype=np.float64):
    """One wavefront (columns 0 ... 63) in which 63 lanes end at 800 hPa and lane 17 runs to the top, then: one valid level,
    all NaN, a repeated height, a rising pressure."""
    nlev = 40
    p, t, td = (np.array(a) for a in synth.columns(nlev=nlev, ncol=68, seed=3, dtype=np.float64))
    z = heights(p)
    lfc, el = np.full(68, 900.0), np.full(68, 800.0)
    el[17] = NAN
    lfc[64:], el[64:] = 900.0, 300.0
    t[np.arange(nlev) != 5, 64] = NAN
    td[:, 65] = NAN
    z[7, 66] = z[6, 66]
    p[9, 67] = p[8, 67] + 2.0
    return tuple(a.astype(dtype) for a in (p, t, td, z, lfc, el))


def test_hand_built_columns():
    args = hand_built()
    ref = R.grid(*args)
    got = xa.ncape(*args)
    compare(got, ref, False, 'hand-built')
    st = ref['status']
    assert list(st[64:]) == [R.ST_NO_LAYER, R.ST_NO_LAYER, R.ST_BAD_HEIGHT, R.ST_BAD_PRESSURE] and np.all(st[:64] == 0)
    assert np.isnan(_np(got['ncape'])[64:]).all()
    top = heights(args[0][-1, 17]) - heights(args[0][0, 17])
    assert abs(ref['el_height'][17] - top) < 1e-6 and np.all(np.delete(ref['el_height'][:64], 17) < 2500.0)
    # above the levels read, the order is not looked at: with E between levels 4 and 5, level 9 of column 67 is not reached
    args2 = tuple(a.copy() for a in args)
    args2[4][67], args2[5][67] = args[0][1, 67], 0.5 * (args[0][4, 67] + args[0][5, 67])
    got2 = xa.ncape(*args2)
    want2 = R.column(*(a[:, 67] for a in args2[:4]), args2[4][67], args2[5][67])
    assert int(got2['status'][67]) == 0 == want2['status'] and abs(float(got2['ncape'][67]) - want2['ncape']) <= 1e-6


# -- 2. xp_ecape against the restated formula --------------------------------------------------------------------------------
def formula_inputs(n=4096):
    rng = np.random.default_rng(17)
    cape, ncape = rng.uniform(0.0, 6000.0, n), rng.uniform(-500.0, 3000.0, n)
    h, su, sv = rng.uniform(2000.0, 17000.0, n), rng.normal(0, 12, n), rng.normal(0, 12, n)
    cape[:8] = [0.0, -0.0, -50.0, NAN, 1e-300, 1e-3, 3000.0, 3000.0]
    ncape[8:16] = [0.0, -0.0, -200.0, NAN, 1e5, 5e4, 500.0, -1e4]
    h[16:24] = [0.0, -100.0, NAN, 1e-3, 1e30, 1.0, 50.0, 12000.0]
    su[24:32], sv[24:32] = [0.0, 0.0, 1e-3, 1e-4, NAN, 3.0, 0.0, -0.0], [0.0, 1e-3, 0.0, 0.0, 1.0, NAN, -0.0, 0.0]
    # the r < 0 guard: r = 1 + 2 psi + 2 a + (psi - a)^2 + 8 e cape with a = 2 e ncape is positive whenever cape > 0 (both
    # signs of ncape), so no input reaches it; these come closest -- hardly any CAPE against a large dilution, shallow and deep
    cape[32:48], ncape[32:48] = 10.0 ** rng.uniform(-6, 0, 16), rng.uniform(2000.0, 1e5, 16)
    h[32:40], su[32:48], sv[32:48] = rng.uniform(1.0, 500.0, 8), rng.uniform(20.0, 60.0, 16), 0.0
    ncape[48:64], su[48:64], sv[48:64] = -rng.uniform(100.0, 2000.0, 16), rng.uniform(0.0, 0.5, 16), 0.0      # B < 0
    return cape, ncape, h, su, sv


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_ecape_formula_vs_restatement(dtype):
    x = [a.astype(dtype) for a in formula_inputs()]
    f32 = dtype == np.float32
    got = xa.ecape_from_ncape(*x)
    x64 = [a.astype(np.float64) for a in x]
    want = R.ecape_value(*x64)
    any_nan = np.isnan(np.stack(x64)).any(axis=0) | ~(x64[2] > 0.0)
    with np.errstate(invalid='ignore'):
        scale = np.maximum(1.0, np.maximum(np.nan_to_num(x64[0]), 0.5 * np.hypot(x64[3], x64[4]) ** 2))
    for k, w in zip(L.ECAPE_OUT, want):
        g = got[k]
        assert g.dtype == dtype and g.shape == (4096,)
        g = g.astype(np.float64)
        assert np.array_equal(np.isnan(g), any_nan) and np.array_equal(np.isnan(w), any_nan), k
        ok = ~any_nan
        tol = 1e-12 * scale[ok] + (np.spacing(np.abs(w[ok]).astype(np.float32)).astype(np.float64) if f32 else 0.0)
        err = np.abs(g[ok] - w[ok])
        print('%s %s: worst difference %.3g (of %.3g allowed there)' % (k, np.dtype(dtype).name, err.max(), tol[np.argmax(err)]))
        assert np.all(err <= tol), (k, float(err.max()), np.argwhere(ok)[np.argmax(err - tol)])
    en, ea = got['ecape'].astype(np.float64), got['ecape_a'].astype(np.float64)
    assert np.all(en[:3] == 0.0) and np.all(ea[:3] == 0.0) and np.all(got['psi'][:3] > 0) and np.isnan(en[3]) and any_nan.sum() >= 7
    assert np.all(en[~any_nan] >= 0.0) and np.all(ea[~any_nan] >= en[~any_nan]) and (en[~any_nan] > 0.0).sum() >= 3500
    if not f32:
        assert abs(en[20] - x64[0][20]) <= 1e-6                              # psi ~ 0: ECAPE is CAPE


# -- 3. the chain ----------------------------------------------------------------------------------------------------------
def sounding(n=600, nlev=40, seed=41):
    p, t, td = synth.columns(nlev=nlev, ncol=n, seed=seed, dtype=np.float64)
    z = heights(p)
    rng = np.random.default_rng(seed + 1)
    h = z - z[0]
    u = 5.0 + h * 2.5e-3 + rng.normal(0, 3, (nlev, n))
    v = -2.0 + h * 1.0e-3 + rng.normal(0, 3, (nlev, n))
    return p, t, td, z, u, v


@pytest.mark.parametrize('parcel', ['most_unstable', 'mixed_layer'])
def test_chain_equals_its_six_calls(parcel):
    import torch
    host = sounding()
    p, t, td, z, u, v = (torch.from_numpy(a).cuda() for a in host)
    got = xa.ecape(p, t, td, z, u, v, parcel=parcel, moist='exact')
    cc = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='exact', want=('cape', 'cin', 'lfc_pressure', 'el_pressure', 'status'))
    nc = xa.ncape(p, t, td, z, cc['lfc_pressure'], cc['el_pressure'])
    bm = xa.bunkers_storm_motion(p, u, v, z)
    wl = xa.wind_layers(p, u, v, z, [{'bottom_height': 0.0, 'top_height': 1000.0}], want=('mean_u', 'mean_v'))
    sr_u, sr_v = wl['mean_u'][0] - bm['right_u'], wl['mean_v'][0] - bm['right_v']
    ec = xa.ecape_from_ncape(cc['cape'], nc['ncape'], nc['el_height'], sr_u, sr_v)
    want = dict(ec, ncape=nc['ncape'], cape=cc['cape'], cin=cc['cin'], lfc_height=nc['lfc_height'], el_height=nc['el_height'],
                sr_u=sr_u, sr_v=sr_v, status=cc['status'] | nc['status'] | bm['status'] | wl['status'])
    assert set(got) == set(want) and len(want) == 11
    for k in want:
        assert got[k].is_cuda and got[k].shape == (600,), k
        assert np.array_equal(_np(got[k]), _np(want[k]), equal_nan=True), k
    en, cape = _np(got['ecape']), _np(got['cape'])
    ok = np.isfinite(en)
    print('%s: %d finite ECAPE, %d positive, median ECAPE / CAPE %.3f' % (parcel, ok.sum(), (en[ok] > 0).sum(),
                                                                         np.median(en[ok & (cape > 100)] / cape[ok & (cape > 100)])))
    # (the C oracle finds an LFC in 455 of these columns for the most unstable parcel and in 412 for the mixed layer; a column
    # without one has no EL height, hence no ECAPE)
    assert ok.sum() >= 350 and (en[ok] > 0).sum() >= 100 and np.all(en[ok] >= 0.0)
    # the same from host arrays, and with the other storm motions and one of the caller's
    hgot = xa.ecape(*host, parcel=parcel, moist='exact')
    for k in want:
        assert isinstance(hgot[k], np.ndarray) and np.array_equal(hgot[k], _np(want[k]), equal_nan=True), k
    if parcel == 'most_unstable':
        left = xa.ecape(p, t, td, z, u, v, parcel=parcel, moist='exact', storm='left')
        assert np.array_equal(_np(left['sr_u']), _np(wl['mean_u'][0] - bm['left_u']), equal_nan=True)
        mine = xa.ecape(p, t, td, z, u, v, parcel=parcel, moist='exact', storm_u=bm['right_u'], storm_v=_np(bm['right_v']))
        for k in ('ecape', 'ecape_a', 'psi', 'sr_u', 'sr_v'):
            assert np.array_equal(_np(mine[k]), _np(want[k]), equal_nan=True), k
    # without entrainment (psi ~ 0 through a huge EL height) ECAPE is CAPE
    free = xa.ecape_from_ncape(cc['cape'], nc['ncape'], torch.full_like(cc['cape'], 1e30), sr_u, sr_v)
    fe = _np(free['ecape'])
    both = np.isfinite(fe)
    assert both.sum() >= 400 and np.array_equal(both, np.isfinite(cape)) and np.max(np.abs(fe[both] - cape[both])) <= 1e-6


# -- 4. input kinds and the raw ABI -------------------------------------------------------------------------------------------
def test_input_kinds_and_strided_views():
    import torch
    args, _ = case(40, np.float64)
    ref = xa.ncape(*args)
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).cuda()):
        got = xa.ncape(*(conv(np.array(a)) for a in args))
        for k in L.NCAPE_OUT:
            assert np.array_equal(_np(got[k]), ref[k], equal_nan=True), k
    assert got['ncape'].is_cuda and got['status'].dtype == torch.int32
    x = [a.astype(np.float64) for a in formula_inputs()]
    fref = xa.ecape_from_ncape(*x)
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).cuda()):
        fgot = xa.ecape_from_ncape(*(conv(a) for a in x))
        for k in L.ECAPE_OUT:
            assert np.array_equal(_np(fgot[k]), fref[k], equal_nan=True), k
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev; then NULL outputs
    nlev, ncol = args[0].shape
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in args[:4]]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    lfc, el = (torch.from_numpy(np.array(a)).cuda() for a in args[4:])
    outs = {k: torch.empty(ncol, dtype=torch.int32 if k == 'status' else torch.float64, device='cuda') for k in L.NCAPE_OUT}
    o = L.NcapeOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, **{k: v.data_ptr() for k, v in outs.items()})
    L.check(lib.xp_ncape(*views, lfc.data_ptr(), el.data_ptr(), o, None))
    torch.cuda.synchronize()
    for k in L.NCAPE_OUT:
        assert np.array_equal(_np(outs[k]), ref[k], equal_nan=True), k
    only = torch.full((ncol,), -77.0, dtype=torch.float64, device='cuda')
    L.check(lib.xp_ncape(*views, lfc.data_ptr(), el.data_ptr(), L.NcapeOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, el_height=only.data_ptr()), None))
    L.check(lib.xp_ncape(*views, lfc.data_ptr(), el.data_ptr(), L.NcapeOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE), None))
    torch.cuda.synchronize()
    assert np.array_equal(_np(only), ref['el_height'], equal_nan=True)


def test_raw_abi_errors():
    lib = L.init(0)
    args, _ = case(12, np.float64)
    p, t, td, z, lfc, el = (np.ascontiguousarray(a[..., :8]) for a in args)
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 12, 8, 8, 1) for a in (p, t, td, z)]
    short = L.View(z.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 12, 4, 4, 1)
    f32 = L.View(z.ctypes.data, L.XP_F32, L.XP_MEM_HOST, 12, 8, 8, 1)
    nodata = L.View(None, L.XP_F64, L.XP_MEM_HOST, 12, 8, 8, 1)
    res = {k: np.empty(8, np.int32 if k == 'status' else np.float64) for k in L.NCAPE_OUT}
    good = L.NcapeOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, **{k: a.ctypes.data for k, a in res.items()})

    def call(vs=views, l=lfc.ctypes.data, e=el.ctypes.data, o=good):
        for a in res.values():
            a[...] = -77
        rc = lib.xp_ncape(*vs, l, e, o, None)
        if rc != L.XP_OK:
            assert all(np.all(a == -77) for a in res.values()), 'outputs touched'
        return rc
    assert call() == L.XP_OK and not np.any(res['status'] == -77)
    ref = R.grid(p, t, td, z, lfc, el)
    assert np.array_equal(res['status'], ref['status']) and np.array_equal(np.isnan(res['ncape']), np.isnan(ref['ncape']))
    bad = [(dict(vs=views[:3] + [short]), 'differ'), (dict(vs=[views[0], short] + views[2:]), 'differ'),
           (dict(vs=views[:3] + [f32]), 'differ'), (dict(vs=views[:3] + [None]), 'height'), (dict(vs=[None] + views[1:]), 'pressure'),
           (dict(vs=[views[0], None] + views[2:]), 'temperature'), (dict(vs=views[:2] + [nodata, views[3]]), 'dewpoint'),
           (dict(l=None), 'lfc_pressure'), (dict(e=None), 'el_pressure'), (dict(o=None), 'out'),
           (dict(o=L.NcapeOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST, ncape=res['ncape'].ctypes.data)), 'out'),
           (dict(o=L.NcapeOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, ncape=res['ncape'].ctypes.data)), 'out')]
    for kw, word in bad:
        assert call(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())
    x, y = np.full(8, 1000.0), np.full(8, -77.0)
    xd, yd = x.ctypes.data, y.ctypes.data
    H, D = L.XP_MEM_HOST, L.XP_F64
    for i, word in enumerate(L.ECAPE_IN):
        ins = [xd] * 5
        ins[i] = None
        assert lib.xp_ecape(8, D, H, *ins, yd, yd, yd, None) == L.XP_E_ARG, word
        assert word in lib.xp_last_error().decode().split(':')[1], (word, lib.xp_last_error())
    assert lib.xp_ecape(-1, D, H, xd, xd, xd, xd, xd, yd, yd, yd, None) == L.XP_E_ARG
    assert lib.xp_ecape(8, 7, H, xd, xd, xd, xd, xd, yd, yd, yd, None) == L.XP_E_ARG and np.all(y == -77.0)
    assert lib.xp_ecape(0, D, H, xd, xd, xd, xd, xd, yd, yd, yd, None) == L.XP_OK and np.all(y == -77.0)
    assert lib.xp_ecape(8, D, H, xd, xd, xd, xd, xd, None, None, None, None) == L.XP_OK                # every output may be NULL
    assert lib.xp_ecape(8, D, H, xd, xd, xd, xd, xd, None, None, yd, None) == L.XP_OK and np.all(y == R.C_PSI / 1000.0)


# -- 5. one full-size grid ---------------------------------------------------------------------------------------------------
def test_full_grid_64_levels_by_1mi_columns():
    import torch
    ncol = 1 << 20
    p, t, td = synth.columns_torch(64, ncol, 'cuda', dtype=torch.float64)
    z = 44330.8 * (1.0 - (p / 1013.25) ** 0.190263)
    cc = xa.cape_cin_columns(p, t, td, parcel='surface', moist='exact', want=('lfc_pressure', 'el_pressure'))
    got = xa.ncape(p, t, td, z, cc['lfc_pressure'], cc['el_pressure'])
    torch.cuda.synchronize()
    st = got['status']
    assert bool(((st == 0) | (st == R.ST_NO_LAYER)).all()) and bool(torch.isfinite(got['ncape'][st == 0]).all())
    cols = np.random.default_rng(0).choice(ncol, 4000, replace=False)
    idx = torch.from_numpy(cols).cuda()
    ps, ts, tds, zs = (x[:, idx].cpu().numpy() for x in (p, t, td, z))
    lfc, el = (cc[k][idx].cpu().numpy() for k in ('lfc_pressure', 'el_pressure'))
    sub = {k: got[k][idx].cpu().numpy() for k in L.NCAPE_OUT}
    del p, t, td, z
    ref = R.grid(ps, ts, tds, zs, lfc, el)
    compare(sub, ref, False, 'full grid sample')
    assert np.isfinite(ref['lfc_height']).sum() >= 1000 and np.count_nonzero(np.isfinite(ref['ncape']) & (ref['ncape'] != 0.0)) >= 1000
