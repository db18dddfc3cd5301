"""The classic sounding indices and the CCL on the device (xp_sounding_indices) against the NumPy restatement
tests/sounding_indices_restatement.py, the entry points it shares its code with, and its own argument checks.  The inputs and
what they hold are counted on the CPU (tests/test_sounding_indices_cpu.py::test_input_census).
Measured on an MI355X, the largest difference from the restatement over the three exact-mode grids (and over the 4,000
sampled columns of the full grid): K / TT / CT / VT 6.3e-13 K (8.0e-13), SWEAT 1.9e-11 (2.0e-11), Showalter 5.7e-13 K
(5.1e-13), ccl_pressure 3.5e-15 relative (3.7e-15), ccl_temperature 1.1e-13 K (1.7e-13), convective temperature 2.3e-13 K
(2.8e-13); against the 'ode' restatement Showalter differs by 2.2e-5 K."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import sounding_indices_cases as K
from tests import sounding_indices_restatement as R
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu
KEYS = R.KEYS
# |device - restatement| per output: absolute [K; 1 for SWEAT], except ccl_pressure: relative
TOL = {'k_index': 1e-10, 'total_totals': 1e-10, 'cross_totals': 1e-10, 'vertical_totals': 1e-10, 'sweat_index': 1e-9,
       'showalter_index': 1e-8, 'ccl_pressure': 1e-7, 'ccl_temperature': 1e-6, 'convective_temperature': 1e-6}


def restate(p, t, td, u=None, v=None, cols=None, **kw):
    p, t, td = (np.asarray(a, dtype=np.float64) for a in (p, t, td))
    u, v = (None if a is None else np.asarray(a, dtype=np.float64) for a in (u, v))
    cols = list(range(p.shape[1])) if cols is None else list(cols)
    ref = R.grid(p, t, td, u, v, cols=cols, **kw)
    depth = kw.get('mixed_layer_depth', 0.0)
    tie = np.array([R.near_tie(p[:, c], t[:, c], td[:, c], None if u is None else u[:, c], None if v is None else v[:, c],
                               mixed_layer_depth=depth, col=r if depth == 0 else None) for c, r in zip(cols, ref['columns'])])
    assert tie.sum() <= 0.01 * len(cols), tie.sum()
    return ref, tie


def compare(got, ref, keep, f32=False, keys=KEYS, tol=TOL, label=''):
    """Status and NaN patterns equal, every output within its tolerance; prints the largest difference of each."""
    assert np.array_equal(np.asarray(got['status'])[keep], ref['status'][keep]), label
    for k in keys:
        gk, rk = np.asarray(got[k]).astype(np.float64)[keep], ref[k][keep]
        assert np.array_equal(np.isnan(gk), np.isnan(rk)), (label, k, np.argwhere(np.isnan(gk) != np.isnan(rk))[:5])
        ok = ~np.isnan(rk)
        err = np.abs(gk[ok] - rk[ok])
        bound = tol[k] * (np.abs(rk[ok]) if k == 'ccl_pressure' else 1.0) + np.zeros(ok.sum())
        if f32:
            bound = bound + np.spacing(np.abs(rk[ok]).astype(np.float32)).astype(np.float64)
        scaled = err / np.abs(rk[ok]) if k == 'ccl_pressure' else err
        print('%s %-24s n = %5d  max = %.3e' % (label, k, ok.sum(), scaled.max() if ok.any() else 0.0))
        assert np.all(err <= bound), (label, k, float(err.max()), np.argwhere(ok)[np.argmax(err - bound)])


@pytest.mark.parametrize('name', ['12x640', '40x640', '7x65'])
def test_exact_mode_vs_rk4_restatement(name):
    p, t, td, u, v = K.inputs(*K.GRIDS[name])
    got = xa.sounding_indices(p, t, td, u, v, moist='exact')
    ref, tie = restate(p, t, td, u, v)
    compare(got, ref, ~tie, label=name)
    n = p.shape[1]
    assert np.isfinite(got['k_index']).sum() >= 0.6 * n and np.isfinite(got['sweat_index']).sum() >= 0.5 * n
    assert np.isfinite(got['ccl_pressure']).sum() >= 0.8 * n and (np.asarray(got['status']) & L.ST_NO_CCL != 0).any()


def test_exact_mode_vs_ode_restatement():
    p, t, td, u, v = K.inputs(*K.GRIDS['40x96'])
    got = xa.sounding_indices(p, t, td, u, v, moist='exact')
    ref, tie = restate(p, t, td, u, v, moist='ode')
    compare(got, ref, ~tie, tol=dict(TOL, showalter_index=1e-3), label='ode')


@pytest.fixture(scope='module')
def oracle_tables():
    from oracle import parcel_oracle as po
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    adiabat_tables.set_tables(tab.index, tab.adiabats)       # both sides look up the SAME arrays
    po.set_moist_lapse('ode', tab)
    yield tab
    po.set_moist_lapse('ode')


def test_table_mode_vs_table_restatement(oracle_tables):
    p, t, td, u, v = K.inputs(*K.GRIDS['40x320'])
    got = xa.sounding_indices(p, t, td, u, v, moist='table')
    ref, tie = restate(p, t, td, u, v, moist='table')
    compare(got, ref, ~tie, label='table')
    assert np.isfinite(got['showalter_index']).sum() >= 150


def test_fp32_inputs_round_like_the_restatement():
    p, t, td, u, v = K.inputs(*K.GRIDS['40x480'], dtype=np.float32)
    got = xa.sounding_indices(p, t, td, u, v, moist='exact')
    assert all(np.asarray(got[k]).dtype == np.float32 for k in KEYS)
    ref, tie = restate(p, t, td, u, v)
    compare(got, ref, ~tie, f32=True, label='f32')


def test_top_and_bottom_differ_where_the_census_says():
    p, t, td, u, v = K.inputs(*K.GRIDS['40x640'])
    top, bot = (xa.ccl(p, t, td, which=w) for w in ('top', 'bottom'))
    ref_b, tie = restate(p, t, td, which='bottom')
    ref_t = R.grid(p, t, td, which='top')
    keep = ~tie
    for got, ref, w in ((top, ref_t, 'top'), (bot, ref_b, 'bottom')):
        compare(dict(zip(R.CCL_KEYS, got), status=ref['status']), ref, keep, keys=R.CCL_KEYS, label=w)
    multi = np.array([len(set(r['crossings'])) >= 2 for r in ref_t['columns']])
    assert multi[keep].sum() >= 5
    with np.errstate(invalid='ignore'):
        assert np.array_equal((top[0] < bot[0])[keep], multi[keep])
    same = keep & ~multi
    assert all(np.array_equal(a[same], b[same], equal_nan=True) for a, b in zip(top, bot))


def test_mixed_layer_ccl_vs_restatement():
    p, t, td, u, v = K.inputs(*K.GRIDS['40x320'])
    got = xa.sounding_indices(p, t, td, mixed_layer_depth=100, want=R.CCL_KEYS)
    ref, tie = restate(p, t, td, mixed_layer_depth=100.0)
    ref['status'] = ref['status'] & R.ST_NO_CCL                 # (the bits of the outputs asked for)
    compare(got, ref, ~tie, keys=R.CCL_KEYS, label='mixed')
    sfc = xa.ccl(p, t, td)[0]
    assert np.isfinite(got['ccl_pressure']).sum() >= 250 and np.nanmax(np.abs(sfc - got['ccl_pressure'])) > 10.0


@pytest.mark.parametrize('moist', ['exact', 'table'])
def test_bit_identity_on_mandatory_levels(moist, oracle_tables):
    p, t, td, u, v = K.mandatory_columns()
    got = xa.sounding_indices(p, t, td, u, v, moist=moist)
    t850, t700, t500, td850, td700 = t[2], t[3], t[4], td[2], td[3]
    assert np.array_equal(got['vertical_totals'], t850 - t500) and np.array_equal(got['cross_totals'], td850 - t500)
    assert np.array_equal(got['total_totals'], (t850 - t500) + (td850 - t500))
    assert np.array_equal(got['k_index'], ((t850 - t500) + (td850 - 273.15)) - (t700 - td700))
    lcl = xa.lcl(np.full(3, 850.0), t850, td850)
    assert np.all(lcl['lcl_pressure'] > 500.0)
    tp = xa.moist_lapse(np.full((1, 3), 500.0), lcl['lcl_temperature'], lcl['lcl_pressure'], moist=moist)[0]
    assert np.isfinite(tp).all() and np.array_equal(got['showalter_index'], t500 - tp)
    assert np.all(got['status'] == 0)
    # SWEAT from the level winds as they are: the restatement's terms on them
    for c in range(3):
        s = R.sweat_terms(td850[c], float(got['total_totals'][c]), u[2, c], v[2, c], u[4, c], v[4, c])
        assert abs(got['sweat_index'][c] - s['sweat_index']) <= 1e-9


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_saturated_surface_is_its_own_ccl(dtype):
    """Td0 == T0: rt - T is exactly 0 at the start level, the lowest crossing IS that level -- its pressure and dewpoint as
    they are, no round trip through ln p -- whatever the surface pressure (the kernel's branch for a level on the crossing)."""
    p0 = np.array([1003.7, 987.3, 1013.25, 961.9], dtype=dtype)
    p = np.concatenate([p0[None, :], np.array([950.0, 900.0, 800.0, 650.0, 500.0], dtype=dtype)[:, None] * np.ones((1, 4), dtype)])
    t = (np.array([297.3, 294.0, 291.0, 285.0, 275.0, 262.0])[:, None] + np.array([0.0, -1.5, 2.25, -3.0])[None, :]).astype(dtype)
    td = (t - np.array([0.0, 4.0, 5.0, 8.0, 12.0, 20.0], dtype=dtype)[:, None]).astype(dtype)
    got = xa.sounding_indices(p, t, td, which='bottom')
    assert got['ccl_pressure'].dtype == dtype and np.all(got['status'] == 0)
    assert np.array_equal(got['ccl_pressure'], p0) and np.array_equal(got['ccl_temperature'], td[0])
    # (p0 / ccl_pressure)^kappa = exp(kappa ln 1): within the library exponential's 3e-16 of 1, i.e. 1e-13 K; one f32 spacing more there
    tol = 1e-12 + (np.spacing(np.float32(300.0)) if dtype == np.float32 else 0.0)
    assert np.all(np.abs(got['convective_temperature'].astype(np.float64) - t[0].astype(np.float64)) <= tol)
    ref = R.grid(p.astype(np.float64), t.astype(np.float64), td.astype(np.float64), which='bottom')
    assert np.array_equal(ref['ccl_pressure'], p0.astype(np.float64)) and np.all(ref['n_crossings'] == 1)
    assert np.array_equal(xa.ccl(p, t, td, which='top')[0], p0)              # the only crossing: the highest too


def test_input_kinds_and_strided_views():
    import torch
    p, t, td, u, v = K.inputs(*K.GRIDS['24x300'])
    ref = xa.sounding_indices(p, t, td, u, v)
    cpu = xa.sounding_indices(*(torch.from_numpy(a) for a in (p, t, td, u, v)))
    dev = xa.sounding_indices(*(torch.from_numpy(a).cuda() for a in (p, t, td, u, v)))
    for k in KEYS + ('status',):
        assert np.array_equal(np.asarray(cpu[k]), ref[k], equal_nan=True), k
        assert np.array_equal(dev[k].cpu().numpy(), ref[k], equal_nan=True), k
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev, ncol = p.shape
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (p, t, td, u, v)]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    outs = {k: torch.empty(ncol, dtype=torch.int32 if k == 'status' else torch.float64, device='cuda') for k in KEYS + ('status',)}
    o = L.SoundingOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, **{k: x.data_ptr() for k, x in outs.items()})
    L.check(lib.xp_sounding_indices(*views, L.SoundingOpts(L.MOIST['exact'], 0, 0.0), o, None))
    torch.cuda.synchronize()
    for k in KEYS + ('status',):
        assert np.array_equal(outs[k].cpu().numpy(), ref[k], equal_nan=True), k


def _status_mask(keys):
    m = 0
    if set(keys) & set(R.INDEX_KEYS):
        m |= L.XP_ST_NO_LAYER
    if 'showalter_index' in keys:
        m |= L.ST_LCL_NOT_CONVERGED
    if set(keys) & set(R.CCL_KEYS):
        m |= L.ST_NO_CCL
    return m


@pytest.mark.parametrize('which', ['top', 'bottom'])
def test_any_subset_of_outputs_equals_the_full_call(which):
    """NULL outputs skip their work (the early exits: past 500 hPa, the first crossing, no winds read) without changing a
    bit of the others; the status carries the bits of the outputs asked for."""
    p, t, td, u, v = K.inputs(*K.GRIDS['24x300'])
    full = xa.sounding_indices(p, t, td, u, v, which=which)
    subsets = [(k,) for k in KEYS] + [R.INDEX_KEYS, R.CCL_KEYS, R.INDEX_KEYS[:4], ('k_index', 'ccl_pressure'),
                                      ('sweat_index', 'convective_temperature'), ('showalter_index', 'sweat_index'), ()]
    for keys in subsets:
        for winds in ((u, v), (None, None)):
            if winds[0] is None and 'sweat_index' in keys:
                continue
            got = xa.sounding_indices(p, t, td, *winds, which=which, want=keys)
            assert set(got) == set(keys) | {'status'}
            for k in keys:
                assert np.array_equal(got[k], full[k], equal_nan=True), (keys, k, winds[0] is None)
            assert np.array_equal(got['status'], full['status'] & _status_mask(keys)), keys
    ml = xa.sounding_indices(p, t, td, u, v, which=which, mixed_layer_depth=100.0)
    got = xa.sounding_indices(p, t, td, which=which, mixed_layer_depth=100.0, want=('ccl_temperature',))
    assert np.array_equal(got['ccl_temperature'], ml['ccl_temperature'], equal_nan=True)
    for k in R.INDEX_KEYS:
        assert np.array_equal(ml[k], full[k], equal_nan=True), k


def test_thin_functions_equal_the_dict_entries():
    p, t, td, u, v = K.inputs(*K.GRIDS['24x300'])
    full = xa.sounding_indices(p, t, td, u, v)
    for fn, k in ((xa.k_index, 'k_index'), (xa.total_totals_index, 'total_totals'), (xa.cross_totals, 'cross_totals'),
                  (xa.vertical_totals, 'vertical_totals'), (xa.showalter_index, 'showalter_index')):
        assert np.array_equal(fn(p, t, td), full[k], equal_nan=True), k
    assert np.array_equal(xa.sweat_index(p, t, td, u, v), full['sweat_index'], equal_nan=True)
    for a, k in zip(xa.ccl(p, t, td), R.CCL_KEYS):
        assert np.array_equal(a, full[k], equal_nan=True), k
    from xarray_parcel_amd import sounding_indices as mirror
    from xarray_parcel_amd._xr import DataArray
    da = [DataArray(a.reshape(24, 15, 20), dims=('model_level_number', 'y', 'x')) for a in (p, t, td, u, v)]
    ds = mirror.sounding_indices(*da)
    for k in KEYS + ('status',):
        assert np.array_equal(np.asarray(ds[k].values).reshape(-1), full[k], equal_nan=True), k


def test_raw_abi_errors():
    lib = L.init(0)
    arrs = [np.ascontiguousarray(a) for a in K.inputs(12, 8, seed=2)]
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 12, 8, 8, 1) for a in arrs]
    k, sw = np.empty(8), np.empty(8)
    good = dict(dtype=L.XP_F64, mem=L.XP_MEM_HOST, k_index=k.ctypes.data)

    def call(u=True, v=True, mode=L.MOIST['exact'], which=0, depth=0.0, out=True, views=views, **o):
        return lib.xp_sounding_indices(*views[:3], views[3] if u else None, views[4] if v else None, L.SoundingOpts(mode, which, depth),
                                       L.SoundingOut(**{**good, **o}) if out else None, None)
    assert call() == L.XP_OK and np.isfinite(k).any()
    assert call(u=False, v=False) == L.XP_OK and call(sweat_index=sw.ctypes.data) == L.XP_OK and np.isfinite(sw).any()
    short = views[:2] + [L.View(arrs[2].ctypes.data, L.XP_F64, L.XP_MEM_HOST, 6, 8, 8, 1)] + views[3:]
    for kw, word in (({'out': False}, 'out'), ({'dtype': L.XP_F32}, 'out'), ({'mem': L.XP_MEM_DEVICE}, 'out'),
                     ({'u': False}, '(u is null)'), ({'v': False}, '(v is null)'), ({'u': False, 'v': False, 'sweat_index': sw.ctypes.data}, 'sweat_index'),
                     ({'mode': 7}, 'moist_mode'), ({'which': 2}, 'ccl_which'), ({'which': -1}, 'ccl_which'),
                     ({'depth': -1.0}, 'ccl_mixed_layer_depth'), ({'depth': float('nan')}, 'ccl_mixed_layer_depth'),
                     ({'depth': float('inf')}, 'ccl_mixed_layer_depth'), ({'views': short}, 'dewpoint')):
        assert call(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())
    if not lib.xp_tables_loaded():
        assert call(mode=L.MOIST['table']) == L.XP_E_NO_TABLES


def test_raw_abi_without_tables():
    """XP_E_NO_TABLES in table mode while no tables are loaded (run in a fresh process: other tests load them)."""
    code = ('import numpy as np; from xarray_parcel_amd import _lib as L; lib = L.init(0); a = np.full((2, 1), 800.0); '
            'v = L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 2, 1, 1, 1); d = np.empty(1); '
            'o = L.SoundingOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, showalter_index=d.ctypes.data); '
            'print(lib.xp_tables_loaded(), lib.xp_sounding_indices(v, v, v, None, None, L.SoundingOpts(L.MOIST["table"], 0, 0.0), o, None))')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ['0', str(L.XP_E_NO_TABLES)], out.stdout


def test_full_grid_64_levels_by_1mi_columns():
    import torch
    ncol = 1 << 20
    p, t, td = synth.columns_torch(64, ncol, 'cuda', dtype=torch.float64)
    # winds on the device: speed and direction linear in ln p through hashed draws at 850 and 500 hPa (sounding_indices_cases.winds)
    h = torch.from_numpy(synth.column_uniforms(ncol, 99)[:4]).cuda()
    d850, d500, f850, f500 = 100.0 + 180.0 * h[0], 180.0 + 160.0 * h[1], 5.0 + 35.0 * h[2], 5.0 + 55.0 * h[3]
    s = (np.log(850.0) - torch.log(p)) / (np.log(850.0) - np.log(500.0))
    spd, ang = torch.clamp(f850 + (f500 - f850) * s, min=0.0) * K.KNOT, torch.deg2rad(d850 + (d500 - d850) * s)
    u, v = -spd * torch.sin(ang), -spd * torch.cos(ang)
    del s, spd, ang
    got = xa.sounding_indices(p, t, td, u, v, moist='exact')
    torch.cuda.synchronize()
    for k in KEYS:
        assert bool(torch.isfinite(got[k]).all()), k
    # by construction Td0 < T0 at the surface and the depression grows to 30 K at the top, so rt crosses T; every column spans
    assert bool((got['status'] & (L.ST_NO_CCL | L.XP_ST_NO_LAYER) == 0).all())
    cols = np.random.default_rng(0).choice(ncol, 4000, replace=False)
    idx = torch.from_numpy(cols).cuda()
    ps, ts, tds, us, vs = (x[:, idx].cpu().numpy() for x in (p, t, td, u, v))
    del p, t, td, u, v
    ref, tie = restate(ps, ts, tds, us, vs)
    compare({k: got[k][idx].cpu().numpy() for k in KEYS + ('status',)}, ref, ~tie, label='full')
