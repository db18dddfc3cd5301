"""Lookup-table moist mode (XP_MOIST_TABLE, pf.py:525-607) on the GPU: every k_cape_cin instantiation of MODE 1 against
the C oracle, and the table's own arithmetic (Moist::start / Moist::at, csrc/xp_device.hpp) at the edges of the table.
Both sides are handed the SAME arrays (the oracle_tables fixture of tests/test_gpu_parity.py).  The inputs come from
tests/table_mode_cases.py; tests/test_table_mode_cases_cpu.py keeps them honest without a GPU.

Bars (the project's own, nothing new): _compare of tests/test_gpu_parity.py -- CAPE / CIN 1e-6 J/kg, pressures and
temperatures 1e-7, indices and status identical, its float32 rule and its tie bounds; primitive temperatures 1e-7 K
(tests/test_gpu_components.py); profile rows 1e-8, the lifted index 1e-9 (float32 2e-4) against the composition, as in
test_profile_vs_oracle / test_lifted_index_in_the_same_pass.

The 48 instantiations k_cape_cin<T, PM, PROFILE, MODE = 1, HUM, DEF, LEAN, false> that launch_p (csrc/xp_cape_tu.hip) can
pick, and the parametrisation that launches each.  T: f64 / f32 = the `dtype` parameter; PM: surface / most_unstable /
mixed_layer / explicit = the `parcel` parameter; so each line below stands for 2 x 4 = 8 instantiations, 6 x 8 = 48:

  launch_p branch                  PROFILE HUM DEF LEAN   launched by
  a.hum && profile                    1     1   0   0     test_specific_humidity[parcel-profile-dtype]
  a.hum                               0     1   0   0     test_specific_humidity[parcel-scalars-dtype]
  profile                             1     0   0   0     test_profile_rows[parcel-dtype], test_lifted_index[parcel-dtype]
  dflt && lean                        0     0   1   1     test_cape_cin_only[parcel-dtype]
  dflt                                0     0   1   0     test_matrix[parcel-0-dtype]
  otherwise (generic)                 0     0   0   0     test_matrix[parcel-1..4-dtype]

(The ids as pytest prints them, e.g. test_specific_humidity[surface-scalars-float64], test_matrix[explicit-3-float32].
MODE 1 has no persistent and no LAZY instantiation: both belong to MODE 2.)  All 48 are reachable from the public API.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import thermo as th
from tests import table_mode_cases as tm
from tests.test_gpu_components import _close
from tests.test_gpu_parity import MODES, _compare, _log_counts, _saturated_tie_columns, oracle_tables  # noqa: F401  (oracle_tables: a fixture)
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu

xa = None
DTYPES = [np.float64, np.float32]
PARCELS = ['surface', 'most_unstable', 'mixed_layer', 'explicit']
LEAN_WANT = ('cape', 'cin', 'lfc_pressure', 'el_pressure', 'parcel_index', 'lcl_pressure', 'parcel_pressure')


@pytest.fixture(scope='module', autouse=True)
def _api(oracle_tables):
    global xa
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from xarray_parcel_amd import numpy_api
    xa = numpy_api
    yield


# ---- (a) the instantiation matrix ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid(dtype):
    """33 x 1337 soundings in `dtype`, the explicit parcel of each column, and the same values in float64."""
    p, t, td = synth.columns(nlev=tm.NLEV, ncol=tm.NCOL, seed=71, nan_fraction=0.08, dtype=dtype)
    pv = (p[0] + dtype(5.0), t[0] + dtype(1.0), td[0] - dtype(1.0))
    return (p, t, td), pv, tuple(v.astype(np.float64) for v in (p, t, td)), tuple(v.astype(np.float64) for v in pv)


def _pkw(parcel, pv):
    return {'parcel': parcel, 'parcel_values': pv} if parcel == 'explicit' else {'parcel': parcel}


def _okw(parcel, pv):
    return {'parcel': parcel, 'parcel_values': np.stack(pv)} if parcel == 'explicit' else {'parcel': parcel}


@functools.lru_cache(maxsize=None)
def _ref(dtype, parcel, mode, profile=False):
    """The C oracle in table mode on _grid(dtype): once per (dtype, parcel, option set), shared and left unchanged."""
    _, _, o, opv = _grid(dtype)
    return co.cape_cin_grid(*o, moist='table', want_profile=profile, **_okw(parcel, opv), **MODES[mode])


def _check_profile(got, ref, dtype, what):
    """The rule of test_profile_vs_oracle: NaN pattern identical, 1e-8 (float32: after rounding the oracle's rows)."""
    for k in ref:
        _close(got[k], ref[k], dtype, 1e-8, '%s %s' % (what, k))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', range(len(MODES)))
@pytest.mark.parametrize('parcel', PARCELS)
def test_matrix(parcel, mode, dtype):
    """All outputs, the five option sets: DEF (option set 0) and the generic kernel (1 ... 4)."""
    g, pv, _, _ = _grid(dtype)
    got = xa.cape_cin_columns(*g, moist='table', **_pkw(parcel, pv), **MODES[mode])
    ref = _ref(dtype, parcel, mode)
    _compare(got, ref, dtype, 1e-6)
    assert np.nanmax(ref['cape']) > 100.0 and np.isnan(ref['cape']).sum() == 0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('parcel', PARCELS)
def test_cape_cin_only(parcel, dtype):
    """DEF + LEAN: bit for bit the all-outputs call, status likewise, and CAPE / CIN against the oracle (the rule of
    test_cape_cin_only_kernels_vs_oracle)."""
    g, pv, _, _ = _grid(dtype)
    kw = _pkw(parcel, pv)
    got = xa.cape_cin_columns(*g, moist='table', want=LEAN_WANT, **kw)
    full = xa.cape_cin_columns(*g, moist='table', **kw)
    for k in LEAN_WANT:
        a, b = np.asarray(got[k]), np.asarray(full[k])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), k
    status = xa.cape_cin_columns(*g, moist='table', want=('cape', 'cin', 'status'), **kw)['status']
    assert np.array_equal(np.asarray(status), np.asarray(full['status']))
    ref = _ref(dtype, parcel, 0)
    _, excluded = _saturated_tie_columns(full, ref)
    keep = ~excluded
    for k in ('cape', 'cin'):
        a, b = np.asarray(got[k], dtype=np.float64)[keep], ref[k][keep]
        if dtype == np.float32:
            b = b.astype(np.float32).astype(np.float64)
        tol = 1e-6 if dtype == np.float64 else 2e-7 * np.maximum(np.abs(b), 1.0) + 1e-6
        assert np.all(np.abs(a - b) <= tol), (k, float(np.max(np.abs(a - b))))
    assert np.array_equal(np.asarray(status)[keep], ref['status'][keep])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('parcel', PARCELS)
def test_profile_rows(parcel, dtype):
    """PROFILE: all six rows against the oracle's, and a subset (the rows not named are not written, the others and the
    scalars do not change)."""
    g, pv, _, _ = _grid(dtype)
    kw = _pkw(parcel, pv)
    ref = _ref(dtype, parcel, 0, True)
    full = xa.cape_cin_columns(*g, moist='table', want_profile=True, **kw)
    _check_profile(full['profile'], ref['profile'], dtype, 'profile %s %s' % (parcel, dtype.__name__))
    _compare(full, ref, dtype, 1e-6)
    part = xa.cape_cin_columns(*g, moist='table', want_profile=xa.LIFTED_INDEX_VARS, **kw)
    assert set(part['profile']) == set(xa.LIFTED_INDEX_VARS)
    for k in xa.LIFTED_INDEX_VARS:
        assert np.array_equal(part['profile'][k], full['profile'][k], equal_nan=True), k
    for k in ('cape', 'cin', 'lfc_index', 'el_index'):
        assert np.array_equal(part[k], full[k], equal_nan=True), k


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('parcel', PARCELS)
def test_lifted_index(parcel, dtype):
    """The lifted index in the same pass against the composition on the written profile (the rule of
    test_lifted_index_in_the_same_pass), which in turn is the oracle's profile to 1e-8 (test_profile_rows)."""
    g, pv, _, _ = _grid(dtype)
    kw = _pkw(parcel, pv)
    full = xa.cape_cin_columns(*g, moist='table', want_profile=True, **kw)
    got = xa.cape_cin_columns(*g, moist='table', lifted_index_at=500.0, **kw)
    assert 'profile' not in got
    want, li = xa.lifted_index(full['profile']), got['lifted_index']
    assert np.array_equal(np.isnan(li), np.isnan(want))
    ok = ~np.isnan(want)
    assert li.dtype == dtype and ok.sum() > 1000
    assert np.max(np.abs(li[ok] - want[ok])) <= (1e-9 if dtype == np.float64 else 2e-4), float(np.max(np.abs(li[ok] - want[ok])))
    for k in ('cape', 'cin', 'lfc_index', 'el_index'):
        assert np.array_equal(got[k], full[k], equal_nan=True), k


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('profile', [False, True], ids=['scalars', 'profile'])
@pytest.mark.parametrize('parcel', PARCELS)
def test_specific_humidity(parcel, profile, dtype):
    """HUM, with and without profile: the moisture array holds specific humidity; the oracle runs on
    dewpoint_from_specific_humidity of the same (rounded) values."""
    (p, t, td), pv, (po, to, tdo), opv = _grid(dtype)
    e = th.saturation_vapor_pressure(tdo)
    w = th.EPSILON * e / (po - e)
    q = (w / (1.0 + w)).astype(dtype)
    with np.errstate(all='ignore'):
        # Rounding q to float32 can lift a saturated level a few 1e-9 K above saturation, outside the input contract
        # Td <= T: such a value takes the next float32 towards zero.  What went wrong without it was the ORACLE, before any
        # kernel was compared: on this grid in float32, column 1011 (surface level, Td - T = 9.4e-9 K; surface and
        # most-unstable parcel) has its LCL and its LFC on the parcel level (962.2763 hPa, lfc_index 0) and the C oracle
        # returns lfc_temperature = +inf there, CAPE finite: nothing a kernel could be held to.
        over = th.dewpoint_from_specific_humidity(po, to, q.astype(np.float64)) > to
        q[over] = np.nextafter(q[over], dtype(0.0))
        td_ref = th.dewpoint_from_specific_humidity(po, to, q.astype(np.float64))
    assert not (td_ref > to).any() and over.sum() <= 0.01 * over.size
    got = xa.cape_cin_columns(p, t, q, moist='table', humidity='specific', want_profile=profile, **_pkw(parcel, pv))
    ref = co.cape_cin_grid(po, to, td_ref, moist='table', want_profile=profile, **_okw(parcel, opv))
    _compare(got, ref, dtype, 1e-6)
    assert np.nanmax(ref['cape']) > 100.0
    if profile:
        _check_profile(got['profile'], ref['profile'], dtype, 'specific humidity %s %s' % (parcel, dtype.__name__))


# ---- (b) start-cell and range rules through the primitives ----------------------------------------------------------------
def _to(where, *xs):
    if where == 'host':
        return xs
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('nlev', tm.EVAL_LENGTHS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_start_cells_through_moist_lapse(dtype, nlev, where, oracle_tables):
    """start_cells x eval_pressures against moist_lapse_table: NaN masks identical, 1e-7 K, no column left out.  A tie
    resolved the other way, a missing clamp or a level outside the table that is not NaN is a difference of >= 0.004 K or
    of the NaN mask.  The six tie classes select the oracle's cell: the result is that cell's adiabat, and the adiabat of
    the other candidate is visibly another one."""
    tab = oracle_tables
    s = tm.start_cells(dtype, tab)
    p, t0, p0, which = tm.cross(s, tm.eval_pressures(dtype)[nlev])
    got = _host(xa.moist_lapse(*_to(where, p, t0, p0), moist='table'))
    ref = tm.table_lapse(tab, p, t0, p0)
    assert got.dtype == dtype
    _close(got, ref, dtype, 1e-7, 'moist_lapse table start cells %s nlev %d %s' % (dtype.__name__, nlev, where))
    assert np.isnan(ref).sum() > 0.1 * ref.size and (~np.isnan(ref)).sum() > 0.1 * ref.size
    ties = np.nonzero(s['cells'][which, 0] >= 0)[0]
    ip, jt = tm.raw_cell(tab, p0.astype(np.float64), t0.astype(np.float64))
    seen = 0
    for c in ties:
        i0, j0 = s['cells'][which[c]]
        pair = ((i0, j0), (i0 + 1, j0)) if tm.START_CLASSES[s['kind'][which[c]]].startswith('p_') else ((i0, j0), (i0, j0 + 1))
        win = (int(ip[c]), int(jt[c]))
        assert win in pair
        lose = pair[1] if win == pair[0] else pair[0]
        a = tm.table_lapse(tab, p[:, c:c + 1], [tm.node_temperature(tab, win[1])], [tm.node_pressure(tab, win[0])])[:, 0]
        b = tm.table_lapse(tab, p[:, c:c + 1], [tm.node_temperature(tab, lose[1])], [tm.node_pressure(tab, lose[0])])[:, 0]
        ok = ~np.isnan(a)
        if not ok.any():
            continue
        if dtype == np.float32:
            a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        g = got[:, c].astype(np.float64)
        assert np.all(np.abs(g[ok] - a[ok]) <= 1e-7 + (2e-7 * np.abs(a[ok]) if dtype == np.float32 else 0.0)), (c, win)
        if nlev == 24:
            assert np.max(np.abs(g[ok] - b[ok])) >= 0.004, (c, win, lose)
        seen += 1
    assert seen >= 100


@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('nlev', tm.EVAL_LENGTHS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_start_cells_through_parcel_profile(dtype, nlev, where, oracle_tables):
    """The same start cells as SATURATED parcels of parcel_profile: the LCL is the parcel's own level, so the adiabat starts
    from (p_ref, T_lcl) with T_lcl = T_ref to an ulp or two of the dewpoint formula.  Which side of a temperature tie that
    falls on is the LCL's rounding, not the rule under test: the three temperature-tie classes are moved a quarter of a
    cell up (0.005 K) for this entry point; every other class, the pressure ties and their one-ulp neighbours included, is
    the same point.  Against the C oracle's parcel_profile in table mode (1e-7, NaN masks identical, every column)."""
    from tests import component_cases as cc
    tab = oracle_tables
    s = tm.start_cells(dtype, tab)
    t_tie = np.isin(s['kind'], [tm.START_CLASSES.index(k) for k in ('t_tie', 't_tie_minus', 't_tie_plus')])
    s['temperature'] = np.where(t_tie, s['temperature'] + dtype(0.25 * tab.t_step), s['temperature']).astype(dtype)
    p, t0, p0, which = tm.cross(s, tm.eval_pressures(dtype)[nlev])
    got = xa.parcel_profile(*_to(where, p, p0, t0, t0), moist='table')
    co.set_moist_lapse('table')
    try:
        ref = cc.run_parcel_profile(co, *(v.astype(np.float64) for v in (p, p0, t0, t0)))
    finally:
        co.set_moist_lapse('rk4')
    near = tm.near_cell_boundary(tab, ref['lcl_pressure'], ref['lcl_temperature'], tol=1e-9)
    kinds = s['kind'][which]
    p_ties = np.isin(kinds, [tm.START_CLASSES.index(k) for k in ('p_tie', 'p_tie_minus', 'p_tie_plus')])
    assert not near[~p_ties].any()                  # only the pressure ties sit on a boundary, and those on purpose
    for k in ('temperature', 'virtual_temperature') + cc.LCL_KEYS:
        _close(_host(got[k]), ref[k], dtype, 1e-7, 'parcel_profile table start cells %s nlev %d %s %s' % (dtype.__name__, nlev, where, k))
    with np.errstate(invalid='ignore'):
        above = p.astype(np.float64) < ref['lcl_pressure'][None, :]
    assert np.isnan(ref['temperature'][above]).sum() > 100 and (~np.isnan(ref['temperature'][above])).sum() > (100 if nlev > 1 else 10)


# ---- (c) the same rules through the CAPE / CIN kernels ------------------------------------------------------------------
def _keep_off_boundaries(tab, got, ref):
    """Drop the columns whose ORACLE LCL lies within 1e-6 (hPa, K) of a cell boundary -- at most 0.1 %, asserted."""
    near = tm.near_cell_boundary(tab, ref['lcl_pressure'], ref['lcl_temperature'])
    _log_counts('cell_boundary=%d n=%d' % (int(near.sum()), near.size))        # next to the tie counts of _compare
    assert near.sum() <= near.size // 1000, ('too many LCLs on a cell boundary', int(near.sum()))
    keep = ~near
    return {k: np.asarray(v)[keep] for k, v in got.items() if k != 'profile'}, {k: v[keep] for k, v in ref.items() if k != 'profile'}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('parcel', PARCELS)
def test_tall_columns(parcel, dtype, oracle_tables):
    """Soundings from 1104 to 1 hPa: levels below the table's 1100 hPa and above its 2.5 hPa in every column; explicit parcels
    whose LCL falls in a filled cell, in an empty one, or outside the index grid (clamped).  All outputs against the C
    oracle, and the CAPE / CIN-only call bit for bit the all-outputs one."""
    tab = oracle_tables
    d = tm.tall_columns(tab=tab)
    g, o = tm.cast3((d['pressure'], d['temperature'], d['dewpoint']), dtype)
    pv, opv = tm.cast3(d['parcel'], dtype)
    ref = co.cape_cin_grid(*o, moist='table', **_okw(parcel, opv))
    # the classes, from the oracle
    assert np.all(o[0][0] > tab.p_max) and np.all((o[0] < 2.5).sum(axis=0) == 2)
    assert np.all(np.isfinite(ref['cape'])) and np.all(np.isfinite(ref['cin'])) and (ref['cape'] > 0).sum() >= 20
    cls = tm.cell_class(tab, ref['lcl_pressure'], ref['lcl_temperature'])
    if parcel == 'explicit':
        for name in tm.TALL_CLASSES:
            assert (cls == name).sum() >= 20, name
        e = cls == 'empty'
        assert np.all(ref['cape'][e] == 0.0) and np.all(ref['cin'][e] == 0.0)
        assert np.all(np.isnan(ref['lfc_pressure'][e])) and np.all(np.isnan(ref['el_pressure'][e]))
        assert np.all(ref['lfc_index'][e] == -1) and np.all(ref['el_index'][e] == -1)
    kw = _pkw(parcel, pv)
    full = xa.cape_cin_columns(*g, moist='table', **kw)
    _compare(*_keep_off_boundaries(tab, full, ref), dtype, 1e-6)
    lean = xa.cape_cin_columns(*g, moist='table', want=LEAN_WANT, **kw)
    for k in LEAN_WANT:
        a, b = np.asarray(lean[k]), np.asarray(full[k])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), k
    status = xa.cape_cin_columns(*g, moist='table', want=('cape', 'cin', 'status'), **kw)['status']
    assert np.array_equal(np.asarray(status), np.asarray(full['status']))


# ---- (d) the edge tests that the other moist modes have -------------------------------------------------------------------
# (truncated columns and NaN pressure levels: the 'table' cases of tests/test_gpu_parity.py)
@pytest.mark.parametrize('nlev', [1, 2, 3, 8])
def test_explicit_parcel_on_ragged_shapes(nlev):
    for ncol in (1, 63, 65, 1025):
        p, t, td = synth.columns(nlev=nlev, ncol=ncol, seed=3, nan_fraction=0.05, dtype=np.float64)
        pv = np.stack([p[0] + 5.0, t[0] + 1.0, td[0] - 1.0])
        got = xa.cape_cin_columns(p, t, td, parcel='explicit', parcel_values=tuple(pv), moist='table')
        ref = co.cape_cin_grid(p, t, td, parcel='explicit', parcel_values=pv, moist='table')
        _compare(got, ref, np.float64, 1e-6)


def test_strided_device_views_through_the_raw_abi():
    """(ncol, nlev)-major device arrays (lev_stride = 1, col_stride = nlev) straight to xp_cape_cin in table mode: bit for
    bit the dense call."""
    import torch
    from xarray_parcel_amd import _lib as L
    nlev, ncol = 24, 1000
    p, t, td = synth.columns(nlev=nlev, ncol=ncol, seed=9, nan_fraction=0.05, dtype=np.float64)
    dense = xa.cape_cin_columns(p, t, td, moist='table', want=('cape', 'cin', 'lfc_index'))
    lib = L.init(0)
    dev = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in (p, t, td)]            # (ncol, nlev)
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in dev]
    cape = torch.empty(ncol, dtype=torch.float64, device='cuda')
    cin = torch.empty_like(cape)
    idx = torch.empty(ncol, dtype=torch.int32, device='cuda')
    so = L.ScalarsOut()
    so.dtype, so.mem = L.XP_F64, L.XP_MEM_DEVICE
    so.cape, so.cin, so.lfc_index = cape.data_ptr(), cin.data_ptr(), idx.data_ptr()
    pc = L.Parcel(L.PARCEL['surface'], 0, 0.0, None, None, None)
    o = L.Opts(1, 1, 1, 0, L.MOIST['table'], L.XP_F64, 0, 0)
    L.check(lib.xp_cape_cin(C.byref(views[0]), C.byref(views[1]), C.byref(views[2]), C.byref(pc), C.byref(o),
                            C.byref(so), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(cape.cpu().numpy(), dense['cape']) and np.array_equal(cin.cpu().numpy(), dense['cin'])
    assert np.array_equal(idx.cpu().numpy(), dense['lfc_index'])
    assert np.nanmax(dense['cape']) > 100.0


# ---- (e) another geometry -----------------------------------------------------------------------------------------------
def test_small_table_of_another_geometry(oracle_tables):
    """23 pressures x 31 temperatures, p_max 1000, p_step 40, t_min 200, t_step 3.5, through the raw xp_set_tables: the
    geometry fields of the ABI are read, not assumed.  moist_lapse against the closed form (independent of both oracles),
    one CAPE / CIN grid against the C oracle on the same table; the full tables are put back on both sides, and one case of
    the matrix shows that they are."""
    from xarray_parcel_amd import _lib as L, adiabat_tables
    small = tm.small_table()
    lib = L.init()
    st = L.Tables(small.n_p, small.n_t, small.n_adiabat, small.p_max, small.p_step, small.t_min, small.t_step,
                  small.index.ctypes.data, small.adiabats.ctypes.data)
    try:
        L.check(lib.xp_set_tables(C.byref(st)))
        co.set_tables(small)
        for dtype in DTYPES:
            p, t0, p0 = tm.small_cases(dtype)
            want = tm.small_closed_form(small, p, t0, p0)
            assert np.isnan(want).sum() > 500 and (~np.isnan(want)).sum() > 500
            for where in ('host', 'device'):
                got = _host(xa.moist_lapse(*_to(where, p, t0, p0), moist='table'))
                _close(got, want, dtype, 1e-7, 'moist_lapse small table %s %s' % (dtype.__name__, where))
        g, _, o, _ = _grid(np.float64)
        ref = co.cape_cin_grid(*o, moist='table')
        cls = tm.cell_class(small, ref['lcl_pressure'], ref['lcl_temperature'])
        assert (cls == 'ordinary').sum() >= 100 and (cls == 'empty').sum() >= 20 and (ref['cape'] > 0).sum() >= 100
        got = xa.cape_cin_columns(*g, moist='table')
        _compare(*_keep_off_boundaries(small, got, ref), np.float64, 1e-6)
        assert not np.array_equal(ref['cape'], _ref(np.float64, 'surface', 0)['cape'])        # another table, another answer
    finally:
        adiabat_tables.set_tables(oracle_tables.index, oracle_tables.adiabats)
        co.set_tables(oracle_tables)
    g, _, o, _ = _grid(np.float64)
    again = co.cape_cin_grid(*o, moist='table')
    assert np.array_equal(again['cape'], _ref(np.float64, 'surface', 0)['cape'], equal_nan=True)
    _compare(xa.cape_cin_columns(*g, moist='table'), again, np.float64, 1e-6)
