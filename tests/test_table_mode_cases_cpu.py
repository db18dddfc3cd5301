"""The inputs of tests/test_gpu_table_mode.py, checked without a GPU: the builders are deterministic, every class of input
is populated, the three descriptions of table mode (oracle.tables.moist_lapse_table, the C oracle, oracle.parcel_oracle)
agree on all of them, and the closed form of the small table is what moist_lapse_table gives on it."""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import parcel_oracle as po
from tests import table_mode_cases as tm

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope='module')
def tables():
    tab = tm.full_tables()
    co.set_tables(tab)
    return tab


def _c_lapse(pressure, t_ref, p_ref):
    """The C oracle's moist_lapse in table mode, column by column."""
    p = np.asarray(pressure, dtype=np.float64)
    co.set_moist_lapse('table')
    try:
        return np.stack([co.moist_lapse(p[:, c], float(t_ref[c]), float(p_ref[c])) for c in range(p.shape[1])], axis=1)
    finally:
        co.set_moist_lapse('rk4')


def test_builders_are_deterministic(tables):
    for dtype in DTYPES:
        a, b = tm.start_cells(dtype, tables), tm.start_cells(dtype, tables)
        assert all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f') for k in a)
        assert a['pressure'].dtype == dtype
        ea, eb = tm.eval_pressures(dtype), tm.eval_pressures(dtype)
        assert sorted(ea) == list(tm.EVAL_LENGTHS) and all(np.array_equal(ea[n], eb[n], equal_nan=True) and ea[n].dtype == dtype for n in ea)
    a, b = tm.tall_columns(tab=tables), tm.tall_columns(tab=tables)
    for k in ('pressure', 'temperature', 'dewpoint'):
        assert np.array_equal(a[k], b[k])
    assert all(np.array_equal(x, y) for x, y in zip(a['parcel'], b['parcel']))
    assert not np.array_equal(a['temperature'], tm.tall_columns(seed=tm.TALL_SEED + 1, tab=tables)['temperature'])
    s, t = tm.small_table(), tm.small_table()
    assert np.array_equal(s.index, t.index) and np.array_equal(s.adiabats, t.adiabats)


@pytest.mark.parametrize('dtype', DTYPES)
def test_start_cell_classes_are_populated_and_are_what_they_claim(dtype, tables):
    s = tm.start_cells(dtype, tables)
    count = np.bincount(s['kind'], minlength=len(tm.START_CLASSES))
    for k, name in enumerate(tm.START_CLASSES):
        assert count[k] >= (1 if name in tm.SINGLE_POINT_CLASSES else 20), (name, count[k])
    p, t = s['pressure'].astype(np.float64), s['temperature'].astype(np.float64)
    cls = tm.cell_class(tables, p, t)
    of = lambda name: cls[s['kind'] == tm.START_CLASSES.index(name)]
    for name in ('p_tie', 'p_tie_minus', 'p_tie_plus', 't_tie', 't_tie_minus', 't_tie_plus', 'filled_edge'):
        assert np.all(of(name) == 'ordinary'), name
    assert (of('node') == 'ordinary').sum() >= 20
    assert np.all(of('empty_first') == 'empty')
    for name in ('p_above_max', 't_below_min'):
        assert np.all(of(name) == 'clamped'), name
    for name in ('p_below_min', 't_above_max'):            # half a cell beyond the edge still belongs to the edge cell
        assert (of(name) == 'clamped').sum() >= 12, name
    for name in tm.SINGLE_POINT_CLASSES:
        assert np.all(of(name) == 'nan')
    # a clamped start can land on a filled cell and on an empty one: both occur
    out = tm.table_lapse(tables, np.full((1, p.size), 1000.0), t, p)[0]
    clamped = cls == 'clamped'
    assert np.isnan(out[clamped]).sum() >= 20 and (~np.isnan(out[clamped])).sum() >= 20
    # the ties: the cell pandas' rules give them, from the class alone, is the one the oracle's arithmetic selects, and
    # the other candidate holds another adiabat (a wrong tie direction is visible).  float32 cannot hold a temperature
    # tie: there the class only has to stay between its two cells.
    ip, jt = tm.raw_cell(tables, p, t)
    n_exact = 0
    for c in np.nonzero(s['cells'][:, 0] >= 0)[0]:
        name = tm.START_CLASSES[s['kind'][c]]
        i0, j0 = s['cells'][c]
        got = (int(ip[c]), int(jt[c]))
        if name.startswith('p_'):
            assert tables.index[i0, j0] != tables.index[i0 + 1, j0] and got in ((i0, j0), (i0 + 1, j0))
        else:
            assert tables.index[i0, j0] != tables.index[i0, j0 + 1] and got in ((i0, j0), (i0, j0 + 1))
        if dtype == np.float64 or name.startswith('p_'):
            assert got == tuple(int(v) for v in tm.tie_winner(tables, s['cells'][c], s['kind'][c])), (name, c, got)
            n_exact += 1
    assert n_exact >= (144 if dtype == np.float64 else 72)
    if dtype == np.float64:                                 # the computed temperature ties are ties
        k = s['kind'] == tm.START_CLASSES.index('t_tie')
        f = (t[k] - tables.t_min) / tables.t_step
        assert np.all(f - np.floor(f) == 0.5)
    k = s['kind'] == tm.START_CLASSES.index('p_tie')
    f = (tables.p_max - p[k]) / tables.p_step
    assert np.all(f - np.floor(f) == 0.5)


@pytest.mark.parametrize('dtype', DTYPES)
def test_eval_pressures_hold_every_edge(dtype):
    ev = tm.eval_pressures(dtype)
    for n, lev in ev.items():
        assert lev.shape[0] == n
        v = lev.astype(np.float64)
        with np.errstate(invalid='ignore'):
            assert np.isnan(v).any() and (v == 2.5).any() and (v == 1100.0).any() and (v == 1104.0).any()
            assert ((v > 1100.0) & (v < 1100.001)).any() and ((v < 2.5) & (v > 2.499)).any()
            assert (v == 2.0).any() and (v == 1.0).any() and (v == 1000.0).any()
    col = ev[24][:, 0].astype(np.float64)
    col = col[~np.isnan(col)]
    assert np.all(np.diff(col) < 0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_moist_lapse_table_and_the_c_oracle_agree_on_every_start_cell(dtype, tables):
    """start_cells x eval_pressures: 1e-9 K, identical NaN masks; every class of level gives both a value and a NaN."""
    s, ev = tm.start_cells(dtype, tables), tm.eval_pressures(dtype)
    for n in tm.EVAL_LENGTHS:
        p, t0, p0, which = tm.cross(s, ev[n])
        a, b = tm.table_lapse(tables, p, t0, p0), _c_lapse(p, t0, p0)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (n, np.argwhere(np.isnan(a) != np.isnan(b))[:10])
        ok = ~np.isnan(a)
        assert ok.sum() > 0.2 * ok.size and np.max(np.abs(a[ok] - b[ok])) <= 1e-9
        pv = p.astype(np.float64)
        with np.errstate(invalid='ignore'):
            outside = np.isnan(pv) | (pv > 1100.0) | (pv < 2.5)
        assert np.all(np.isnan(a[outside]))
        with np.errstate(invalid='ignore'):
            assert (~np.isnan(a[pv == 1100.0])).any() and (~np.isnan(a[pv == 2.5])).any()
        cls = tm.cell_class(tables, p0.astype(np.float64), t0.astype(np.float64))
        assert np.all(np.isnan(a[:, (cls == 'empty') | (cls == 'nan')]))
        # the value on the table's lowest pressure is the row's first entry, on its highest the last one (the lo >= n_p - 1 case)
        filled = np.nonzero(~np.isnan(a).all(axis=0))[0]
        assert filled.size >= 20


def test_a_wrong_tie_direction_is_a_hundredth_of_a_kelvin(tables):
    """What the 1e-7 K bar of the GPU test has to tell apart: the two adiabats around each tie are >= 0.004 K apart
    somewhere on the 24-level column (and 0.01 K for most)."""
    s = tm.start_cells(np.float64, tables)
    lev = tm.eval_pressures(np.float64)[24][:, 0]
    gaps = []
    for c in np.nonzero(s['cells'][:, 0] >= 0)[0]:
        i0, j0 = s['cells'][c]
        i1, j1 = (i0 + 1, j0) if tm.START_CLASSES[s['kind'][c]].startswith('p_') else (i0, j0 + 1)
        a = tm.table_lapse(tables, lev[:, None], [tm.node_temperature(tables, j0)], [tm.node_pressure(tables, i0)])
        b = tm.table_lapse(tables, lev[:, None], [tm.node_temperature(tables, j1)], [tm.node_pressure(tables, i1)])
        gaps.append(float(np.nanmax(np.abs(a - b))))
    assert min(gaps) >= 0.004 and np.median(gaps) >= 0.009, (min(gaps), np.median(gaps))


PARCELS = ('surface', 'most_unstable', 'mixed_layer', 'explicit')


def _tall_reference(tables, dtype, parcel):
    d = tm.tall_columns(tab=tables)
    _, (p, t, td) = tm.cast3((d['pressure'], d['temperature'], d['dewpoint']), dtype)
    _, pv = tm.cast3(d['parcel'], dtype)
    ref = co.cape_cin_grid(p, t, td, parcel=parcel, moist='table', parcel_values=np.stack(pv) if parcel == 'explicit' else None)
    return (p, t, td), pv, ref


@pytest.mark.parametrize('dtype', DTYPES)
def test_tall_columns_classes_and_boundary_rule(dtype, tables):
    d = tm.tall_columns(tab=tables)
    assert d['pressure'].shape == (tm.NLEV, tm.NCOL)
    assert np.all(np.diff(d['pressure'], axis=0) < 0) and np.all(d['temperature'] - d['dewpoint'] >= 0.5 - 1e-9)
    assert np.all(d['pressure'][0] > 1100.0) and np.all((d['pressure'] < 2.5).sum(axis=0) == 2)
    assert (d['pressure'][0] == 1104.0).sum() >= 20 and np.all(d['pressure'][-1] == 1.0)
    for parcel in PARCELS:
        _, _, ref = _tall_reference(tables, dtype, parcel)
        cls = tm.cell_class(tables, ref['lcl_pressure'], ref['lcl_temperature'])
        near = tm.near_cell_boundary(tables, ref['lcl_pressure'], ref['lcl_temperature'])
        assert near.sum() <= tm.NCOL // 1000, (parcel, int(near.sum()))           # at most 0.1 %; this seed: none
        assert near.sum() == 0, (parcel, int(near.sum()))
        assert np.all(np.isfinite(ref['cape'])) and np.all(np.isfinite(ref['cin']))
        if parcel != 'explicit':
            # three levels outside the table, a finite result all the same
            assert np.all(cls == 'ordinary') and np.nanmax(ref['cape']) > 100.0 and (ref['cape'] > 0).sum() > 100
            continue
        for name in tm.TALL_CLASSES:
            assert (cls == name).sum() >= 20, (name, int((cls == name).sum()))
        e = cls == 'empty'
        assert np.all(ref['cape'][e] == 0.0) and np.all(ref['cin'][e] == 0.0)
        assert np.all(np.isnan(ref['lfc_pressure'][e])) and np.all(np.isnan(ref['el_pressure'][e]))
        assert np.all(ref['lfc_index'][e] == -1) and np.all(ref['el_index'][e] == -1)
        c = cls == 'clamped'
        assert (ref['cape'][c] > 0).sum() >= 20 and (ref['cape'][c] == 0).sum() >= 20     # clamped onto a filled and onto an empty cell
        for sub in range(4):
            assert np.all(c[(d['parcel_kind'] == 2) & ((np.arange(tm.NCOL) // 4) % 4 == sub)])


@pytest.mark.parametrize('parcel', PARCELS)
def test_c_and_python_oracle_agree_on_the_tall_columns(parcel, tables):
    """Indices identical, CAPE / CIN within 1e-9 J/kg (absolute), on every column -- every class of LCL among them."""
    (p, t, td), pv, ref = _tall_reference(tables, np.float64, parcel)
    cls = tm.cell_class(tables, ref['lcl_pressure'], ref['lcl_temperature'])
    cols = np.arange(tm.NCOL)
    if parcel == 'explicit':
        for name in tm.TALL_CLASSES:
            assert (cls[cols] == name).sum() >= 20
    po.set_moist_lapse('table', tables)
    try:
        for c in cols:
            with np.errstate(all='ignore'):
                if parcel == 'explicit':
                    res = po.cape_cin(p[:, c], t[:, c], td[:, c], parcel_temperature=pv[1][c], parcel_pressure=pv[0][c],
                                      parcel_dewpoint=pv[2][c], per_column_lcl=True)
                else:
                    fn = {'surface': po.surface_based_cape_cin, 'most_unstable': po.most_unstable_cape_cin,
                          'mixed_layer': po.mixed_layer_cape_cin}[parcel]
                    res = fn(p[:, c], t[:, c], td[:, c], per_column_lcl=True)
            cc, prof = res[0], res[1]
            for k in ('cape', 'cin'):
                assert abs(ref[k][c] - cc[k]) <= 1e-9, (c, k, ref[k][c], cc[k], cls[c])
            assert ref['lfc_index'][c] == prof['lfc_index'] and ref['el_index'][c] == prof['el_index'], (c, cls[c])
    finally:
        po.set_moist_lapse('ode')


@pytest.mark.parametrize('dtype', DTYPES)
def test_small_table_closed_form(dtype, tables):
    """moist_lapse_table on the hand-made table equals A + B p of the selected adiabat to 1e-12 K, NaN masks identical; so
    does the C oracle once it is handed that table (and the full tables are put back)."""
    small = tm.small_table()
    assert small.index.shape == (tm.SMALL_N_P, tm.SMALL_N_T) and small.adiabats.shape == (tm.SMALL_N_ADIABAT, tm.SMALL_N_P)
    assert 0.05 < (small.index == 0).mean() < 0.6 and len(set(small.index.ravel())) == tm.SMALL_N_ADIABAT + 1
    p, t0, p0 = tm.small_cases(dtype)
    want = tm.small_closed_form(small, p, t0, p0)
    got = tm.table_lapse(small, p, t0, p0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert ok.sum() > 500 and np.isnan(want).sum() > 500
    assert np.max(np.abs(got[ok] - want[ok])) <= 1e-12
    co.set_tables(small)
    try:
        c = _c_lapse(p, t0, p0)
    finally:
        co.set_tables(tables)
    assert np.array_equal(np.isnan(c), np.isnan(want)) and np.max(np.abs(c[ok] - want[ok])) <= 1e-12
    # every start class of the small table is in the sample: both ties, every edge clamped, an empty cell, NaN
    cls = tm.cell_class(small, p0.astype(np.float64), t0.astype(np.float64))
    for name in ('ordinary', 'empty', 'clamped', 'nan'):
        assert (cls == name).sum() >= 3, name
