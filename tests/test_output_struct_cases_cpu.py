"""tests/output_struct_cases.py without a GPU: the guarded buffer against NumPy (and three simulated bad kernels it must
catch), the census of the case tables, and the grids."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import layered_soundings as ls
from tests import output_struct_cases as oc

SHAPES = [(5, 7), (1, 13), (4, 1)]


def simulated_kernel(g, values, n_rows=None, ncol=None, ls_=None, cs=None, dtype=None, shift=0):
    """What a kernel does with the address of element (0, 0): one store of `dtype` per element at the strides it believes in."""
    n_rows, ncol = g.n_rows if n_rows is None else n_rows, g.ncol if ncol is None else ncol
    ls_, cs, dtype = g.ls if ls_ is None else ls_, g.cs if cs is None else cs, np.dtype(g.dtype if dtype is None else dtype)
    for j in range(n_rows):
        for c in range(ncol):
            off = g.guard + (j * ls_ + c * cs + shift) * dtype.itemsize
            g.buf[off:off + dtype.itemsize] = np.array([values[j, c]], dtype=dtype).view(np.uint8)


@pytest.mark.parametrize('layout', oc.LAYOUTS)
@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.int32])
@pytest.mark.parametrize('shape', SHAPES)
def test_a_correct_kernel_writes_exactly_the_logical_elements(layout, dtype, shape):
    n_rows, ncol = shape
    ls_, cs = oc.layout_strides(layout, n_rows, ncol)
    g = oc.Guarded(n_rows, ncol, dtype, ls_, cs)
    assert g.pristine() and g.untouched() and not g.written()
    assert g.ptr == g.buf.ctypes.data + oc.GUARD and oc.GUARD >= 256 and g.ptr % 8 == 0
    assert g.nbytes == 2 * oc.GUARD + ((n_rows - 1) * ls_ + (ncol - 1) * cs + 1) * np.dtype(dtype).itemsize
    values = np.arange(n_rows * ncol).reshape(n_rows, ncol).astype(dtype) + 1
    if np.dtype(dtype).kind == 'f':
        values[0, 0] = np.nan                                           # the outputs legitimately hold NaN
    simulated_kernel(g, values)
    assert g.untouched() and g.written() and not g.pristine()
    got = g.read()
    assert got.dtype == np.dtype(dtype) and got.shape == (n_rows, ncol) and np.array_equal(got, values, equal_nan=np.dtype(dtype).kind == 'f')
    # against NumPy's own strided view of the same bytes
    view = np.lib.stride_tricks.as_strided(g.buf[oc.GUARD:].view(dtype), (n_rows, ncol), (ls_ * got.itemsize, cs * got.itemsize))
    assert np.array_equal(view, got, equal_nan=np.dtype(dtype).kind == 'f')


def test_the_one_row_forms():
    for dtype in (np.float32, np.float64, np.int32):
        g = oc.Guarded.row(9, dtype)
        assert (g.n_rows, g.ncol, g.ls, g.cs) == (1, 9, 9, 1) and g.read().shape == (1, 9) and g.read().dtype == np.dtype(dtype)
        simulated_kernel(g, np.arange(9).reshape(1, 9))
        assert g.untouched() and np.array_equal(g.read()[0], np.arange(9))


def test_a_write_one_element_past_the_end_is_caught():
    for layout in oc.LAYOUTS:
        g = oc.Guarded(4, 6, np.float64, *oc.layout_strides(layout, 4, 6))
        simulated_kernel(g, np.ones((5, 6)), n_rows=5) if layout == 'dense' else simulated_kernel(g, np.ones((4, 6)), shift=1)
        assert not g.untouched(), layout
    g = oc.Guarded.row(8, np.float32)
    simulated_kernel(g, np.ones((1, 9)), ncol=9)                       # ncol + 1 columns
    assert not g.untouched()
    g = oc.Guarded.row(8, np.float32)
    simulated_kernel(g, np.ones((1, 8)), shift=-1)                     # and one before the start
    assert not g.untouched()


def test_an_8_byte_store_into_a_4_byte_slot_is_caught():
    """st() with the wrong dtype flag: doubles at double strides into a float buffer."""
    for layout in oc.LAYOUTS:
        g = oc.Guarded(3, 5, np.float32, *oc.layout_strides(layout, 3, 5))
        simulated_kernel(g, np.ones((3, 5)), dtype=np.float64)
        assert not g.untouched(), layout
    g = oc.Guarded.row(1, np.float32)                                  # a single element: the store's upper half lands in the guard
    simulated_kernel(g, np.ones((1, 1)), dtype=np.float64)
    assert not g.untouched()
    # and the converse, a 4-byte store into an 8-byte slot, leaves half of every element unwritten: a value mismatch
    g = oc.Guarded(3, 5, np.float64)
    simulated_kernel(g, np.full((3, 5), 2.0), dtype=np.float32)
    assert not np.array_equal(g.read(), np.full((3, 5), 2.0)) and not g.written()


def test_a_dense_write_into_a_padded_layout_is_caught():
    n_rows, ncol = 4, 6
    g = oc.Guarded(n_rows, ncol, np.float64, *oc.layout_strides('padded', n_rows, ncol))
    simulated_kernel(g, np.ones((n_rows, ncol)), ls_=ncol, cs=1)
    assert not g.untouched()
    g = oc.Guarded(n_rows, ncol, np.float64, *oc.layout_strides('second_column', n_rows, ncol))
    simulated_kernel(g, np.ones((n_rows, ncol)), ls_=ncol, cs=1)
    assert not g.untouched()
    g = oc.Guarded(n_rows, ncol, np.float64, *oc.layout_strides('column_major', n_rows, ncol))
    simulated_kernel(g, np.arange(24.0).reshape(n_rows, ncol), ls_=ncol, cs=1)        # same span: the values land in the wrong places
    assert g.untouched() and not np.array_equal(g.read(), np.arange(24.0).reshape(n_rows, ncol))


# ---- census ------------------------------------------------------------------------------------------------------------------------
def crossed(case):
    """Some output struct of the call has another dtype than the views."""
    return any(s['dtype'] != case['view_dtype'] for s in case['scalars']) or any(
        pr is not None and pr['dtype'] != case['view_dtype'] for pr in case['profiles'])


def test_case_ids_are_unique_and_complete():
    cases = oc.ALL_CALL_CASES
    assert len({c['id'] for c in cases}) == len(cases)
    for c in cases:
        assert c['entry'] in ('xp_cape_cin', 'xp_cape_cin_multi') and c['grid'] in oc.GRID_NAMES and c['moist'] in ('exact', 'family', 'table')
        assert c['view_dtype'] in oc.DTYPES and c['view_mem'] in oc.MEMS and c['opt'] in range(len(ls.OPTION_SETS))
        assert len(c['parcels']) == len(c['scalars']) == len(c['profiles'])
        assert set(c['reaches']) <= set(oc.KERNEL_FAMILIES) | set(oc.SINK_BRANCHES)
        for s in c['scalars']:
            assert s['dtype'] in oc.DTYPES and s['mem'] in oc.MEMS and set(s['want']) <= set(oc.ALL_SCALARS)
        for pr in c['profiles']:
            if pr is not None:
                assert pr['dtype'] in oc.DTYPES and pr['mem'] in oc.MEMS and pr['layout'] in oc.LAYOUTS and pr['extra'] in oc.EXTRA_ROWS
                assert set(pr['vars']) <= set(oc.PROFILE_VARS) and (pr['vars'] or pr['lifted_index'])
                assert pr['mem'] == 'device' or pr['layout'] == 'dense'                       # a host profile is dense


def test_what_a_case_says_it_reaches_follows_from_its_request():
    """The dispatch rules of csrc/xp_cape_tu.hip and stage_cape_out, restated."""
    for c in oc.ALL_CALL_CASES:
        r = set(c['reaches'])
        for i, (s, pr) in enumerate(zip(c['scalars'], c['profiles'])):
            lean = not any(k in oc.FULL_ONLY for k in s['want'])
            if c['entry'] == 'xp_cape_cin':
                assert ('cape_cin_only' in r) == (lean and c['compute'] == 'f64'), c['id']
                assert ('all_outputs' in r) == (not lean), c['id']
                assert ('compute32' in r) == (c['compute'] == 'f32'), c['id']
                assert ('lazy_lifted_index' in r) == oc.lazy_request(c), c['id']
                if pr is not None and pr['vars']:
                    native = len(pr['vars']) == 6 and pr['dtype'] == c['view_dtype']
                    assert ('native6' in r) == native and ('generic' in r) == (not native), c['id']
                    assert ('finish_padding' in r) == (pr['extra'] > 0), c['id']
                assert ('blank' in r) == (c['grid'] == 'nan_surface' and pr is not None), c['id']
            assert ('rk4_redo' in r) <= (c['moist'] == 'family'), c['id']
            assert ('rk4_redo' in r) == (c['grid'] == 'off_table' and c['moist'] == 'family'), c['id']
        if c['compute'] == 'f32':
            assert c['view_dtype'] == 'f32' and c['scalars'][0]['dtype'] == 'f64' and c['parcels'] == ('surface',) and c['moist'] == 'family'
        assert ('fused_multi' in r) == bool(c['fused']), c['id']
        if c['grid'] == 'persistent':
            assert c['view_dtype'] == 'f32' and c['moist'] == 'family' and c['parcels'] == ('surface',)


def test_every_kernel_family_and_sink_branch_is_reached_by_a_crossed_case():
    for what in oc.KERNEL_FAMILIES + oc.SINK_BRANCHES:
        hits = [c['id'] for c in oc.ALL_CALL_CASES if what in c['reaches'] and (crossed(c) or what == 'native6')]
        print('%-18s %d cases, e.g. %s' % (what, len(hits), hits[:3]))
        assert hits, what
    # native6 is by definition the profile in the views' dtype: it is reached with the SCALARS crossed
    assert any('native6' in c['reaches'] and c['scalars'][0]['dtype'] != c['view_dtype'] for c in oc.CAPE_CASES)
    # both directions of the crossing for the two kernel families of xp_cape_cin, in every moist mode they have
    for fam, modes in (('all_outputs', ('exact', 'family', 'table')), ('cape_cin_only', ('exact', 'family'))):
        for moist in modes:
            pairs = {(c['view_dtype'], c['scalars'][0]['dtype']) for c in oc.CAPE_CASES if fam in c['reaches'] and c['moist'] == moist and c['profiles'][0] is None}
            assert {('f32', 'f64'), ('f64', 'f32')} <= pairs, (fam, moist, pairs)
    plain = [c for c in oc.CAPE_CASES if c['profiles'][0] is None and 'all_outputs' in c['reaches']]
    assert {c['parcels'][0] for c in plain} == {'surface', 'most_unstable', 'mixed_layer', 'explicit'}
    assert {c['opt'] for c in plain} == {0, 4}
    lean = [c for c in oc.CAPE_CASES if 'cape_cin_only' in c['reaches'] and c['profiles'][0] is None]
    assert {'off_table', 'persistent'} <= {c['grid'] for c in lean}
    assert sum(c['grid'] == 'persistent' for c in oc.ALL_CALL_CASES) == 1
    assert {c['parcels'][0] for c in oc.ORACLE_CASES} == set(ls.PARCELS) and all(c['grid'] == 'B' and c['moist'] == 'family' for c in oc.ORACLE_CASES)


def test_every_layout_nlev_out_mem_pairing_and_multi_path_occurs():
    profs = [(c, pr) for c in oc.CAPE_CASES for pr in c['profiles'] if pr is not None]
    rows = [(c, pr) for c, pr in profs if pr['vars']]
    assert {pr['layout'] for _, pr in rows} == set(oc.LAYOUTS)
    assert {pr['extra'] for _, pr in rows} == set(oc.EXTRA_ROWS)
    assert {(c['view_dtype'], pr['dtype']) for c, pr in rows if len(pr['vars']) == 6} == {(a, b) for a in oc.DTYPES for b in oc.DTYPES}
    assert {(c['view_dtype'], pr['dtype']) for c, pr in rows if pr['vars'] == oc.LIFTED_INDEX_VARS} == {(a, b) for a in oc.DTYPES for b in oc.DTYPES}
    assert {pr['layout'] for c, pr in rows if c['grid'] == 'nan_surface'} == set(oc.LAYOUTS)            # blank() under every layout
    assert {c['grid'] for c, _ in rows} >= {'R', 'R1', 'R2', 'one', 'nan_surface', 'off_table'}
    assert {c['parcels'][0] for c, _ in rows} >= {'surface', 'most_unstable', 'mixed_layer'}
    assert any(pr['lifted_index'] and pr['vars'] for _, pr in profs) and any(pr['lifted_index'] and not pr['vars'] for _, pr in profs)
    assert any(pr['dtype'] != c['scalars'][0]['dtype'] for c, pr in profs)
    # the six pairings of (views, scalars, profile) memory that are not all the same
    mems = {(c['view_mem'], c['scalars'][0]['mem'], pr['mem']) for c, pr in profs}
    assert {m for m in mems if len(set(m)) > 1} == {(a, b, c) for a in oc.MEMS for b in oc.MEMS for c in oc.MEMS} - {('host',) * 3, ('device',) * 3}
    # xp_cape_cin_multi: fused and one pass per parcel, each with the two structs as stated and swapped, profiles on the per-parcel path
    for fused in (True, False):
        mine = [c for c in oc.MULTI_CASES if c['fused'] == fused]
        firsts = {(c['scalars'][0]['dtype'], c['scalars'][0]['mem'], set(c['scalars'][0]['want']) == set(oc.ALL_SCALARS)) for c in mine}
        assert firsts == {('f32', 'device', False), ('f64', 'host', True)}, (fused, firsts)
        assert all(c['parcels'] == oc.MULTI_PARCELS and c['moist'] == 'family' for c in mine)
        assert all({'status'} <= set(s['want']) for c in mine for s in c['scalars'] if s['mem'] == 'host')
    with_profiles = [c for c in oc.MULTI_CASES if any(c['profiles'])]
    assert with_profiles and all(not c['fused'] for c in with_profiles)
    for c in with_profiles:
        li, six = c['profiles']
        assert li['lifted_index'] and not li['vars'] and len(six['vars']) == 6 and six['layout'] == 'column_major'
        assert six['dtype'] != c['view_dtype']
    assert {c['entry'] for c in oc.SCALARS_ENTRY_CASES} == {'xp_lfc_el', 'xp_select_parcel', 'xp_rebase_profile'}
    for e in ('xp_lfc_el', 'xp_select_parcel', 'xp_rebase_profile'):
        mine = [c for c in oc.SCALARS_ENTRY_CASES if c['entry'] == e]
        assert any(c['view_dtype'] != c['out_dtype'] for c in mine) and any(c['view_mem'] != c['out_mem'] for c in mine)
    assert {'scalars-dtype', 'profile-dtype', 'nlev_out', 'host-profile-not-dense', 'lifted-index-pressure-zero'} <= {r[0] for r in oc.REJECTIONS}


def test_check_out_entry_points_are_the_call_sites_of_the_source():
    """A new entry point cannot hold its out struct to check_out() without a case here."""
    sites = oc.check_out_call_sites()
    assert sites == set(oc.CHECK_OUT_ENTRIES), (sorted(sites - set(oc.CHECK_OUT_ENTRIES)), sorted(set(oc.CHECK_OUT_ENTRIES) - sites))
    for e in oc.CHECK_OUT_ENTRIES:
        assert {c['crossed'] for c in oc.CHECK_OUT_CASES if c['entry'] == e} == {'dtype', 'mem'}
    # the scanner on a made-up source: a direct call and a shared body
    src = ('template <typename O> int check_out(const char *e, const O *o) {\n}\n'
           'template <bool X, typename O>\nint body(const char *entry, O *out) {\n    if ((rc = check_out(entry, out, z))) return rc;\n}\n'
           'int xp_a(int x) {\n    if ((rc = check_out("xp_a", out, p))) return rc;\n}\n'
           'int xp_b(int x) {\n    return body<false>("xp_b", out);\n}\nint xp_c(int x) {\n    return 0;\n}\n')
    assert oc.check_out_call_sites(src) == {'xp_a', 'xp_b'}


# ---- grids -------------------------------------------------------------------------------------------------------------------------
SMALL = [g for g in oc.GRID_NAMES if g != 'persistent']


def test_grids_are_exact_in_float32_and_shaped_as_stated():
    for name in SMALL:
        g64, g32 = oc.grid(name, 'f64'), oc.grid(name, 'f32')
        for a, b in zip(g64, g32):
            assert a.dtype == np.float64 and b.dtype == np.float32 and not a.flags.writeable and not b.flags.writeable
            assert np.array_equal(a, b.astype(np.float64), equal_nan=True), name
            assert np.array_equal(np.round(a * ls.Q), a * ls.Q, equal_nan=True), (name, 'multiples of 1/64')
    assert oc.grid('R')[0].shape == ls.GRID_REPLAY[:2] and oc.grid('B')[0].shape == ls.GRID_B[:2]
    assert oc.grid('R1')[0].shape == (1, 3000) and oc.grid('R2')[0].shape == (2, 3000) and oc.grid('one')[0].shape == (40, 1)
    assert oc.PERSISTENT_SHAPE[:2] == (8, (3 << 18) + 77)
    for name in ('R1', 'R2'):
        assert all(np.array_equal(a, b[:a.shape[0]], equal_nan=True) for a, b in zip(oc.grid(name), oc.grid('R')))
    ex = oc.explicit_parcel('R', 'f32')
    assert all(np.array_equal(a.astype(np.float64), b, equal_nan=True) for a, b in zip(ex, oc.explicit_parcel('R', 'f64')))


def test_the_nan_surface_copy_has_the_stated_blank_columns():
    p, t, td = oc.grid('nan_surface')
    base = oc.grid('R')
    every = np.zeros(p.shape[1], dtype=bool)
    every[::oc.NAN_SURFACE_EVERY] = True
    assert np.all(np.isnan(t[0, every])) and every.sum() == 334
    assert np.array_equal(np.isnan(t[0]), every | np.isnan(base[1][0]))
    assert np.array_equal(t[1:], base[1][1:], equal_nan=True) and np.array_equal(p, base[0]) and np.array_equal(td, base[2], equal_nan=True)
    ref = co.cape_cin_grid(p, t, td, parcel='surface', moist='rk4', want_profile=True)
    blank = np.isnan(ref['lcl_pressure'])
    assert np.array_equal(blank, np.isnan(t[0]) | np.isnan(td[0]))
    assert np.all(ref['cape'][blank] == 0.0) and np.all(np.isnan(ref['profile']['pressure'][:, blank]))


def test_the_off_table_copy_really_leaves_the_family_table():
    """psi, the adiabat's temperature at 1000 hPa, counted with the oracle: beyond the table's 311.95 K in some columns."""
    p, t, td = oc.grid('off_table')
    base = oc.grid('R')
    warm = np.zeros(p.shape[1], dtype=bool)
    warm[::oc.OFF_TABLE_EVERY] = True
    assert np.array_equal(t[:, ~warm], base[1][:, ~warm], equal_nan=True) and np.array_equal(t[:, warm], base[1][:, warm] + 22.0, equal_nan=True)
    with np.errstate(invalid='ignore'):
        assert not np.any(td > t)
    ref = co.cape_cin_grid(p, t, td, parcel='surface', moist='rk4')
    co.set_moist_lapse('rk4')
    cols = np.nonzero(warm & ~np.isnan(ref['lcl_pressure']))[0]
    psi = np.array([co.moist_lapse(np.array([1000.0]), ref['lcl_temperature'][c], ref['lcl_pressure'][c])[0] for c in cols])
    print('%d of %d warmed columns have psi > 311.95 K (largest %.2f K)' % ((psi > 311.95).sum(), cols.size, psi.max()))
    assert (psi > 311.95).sum() >= 100
    cool = np.nonzero(~warm & ~np.isnan(ref['lcl_pressure']))[0][:200]
    psi_cool = np.array([co.moist_lapse(np.array([1000.0]), ref['lcl_temperature'][c], ref['lcl_pressure'][c])[0] for c in cool])
    assert (psi_cool < 311.95).mean() > 0.9
