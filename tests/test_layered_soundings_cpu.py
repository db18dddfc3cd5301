"""CPU guard of tests/layered_soundings.py (no GPU), the counterpart of test_component_cases_cpu.py: the generator is
deterministic and exact in float32, the grids hold -- in numbers -- the classes of ascent tests/test_gpu_layered.py is
about, and the NumPy and the C oracle agree on them, so that the inputs carry no ambiguity a GPU comparison could trip over.

The floors.  On the 48-level grid A they are about half of the shares measured when the recipe was fixed (surface /
most-unstable / mixed-layer of 6000 columns: >= 3 sign changes 1092 / 739 / 1144, >= 5 sign changes 158 / 73 / 127, positive
net-sum CIN 1947 / 3437 / 1708, LCL on the parcel level 195 / 162 / 385; most-unstable index > 0 in 3523, every index
1 ... 19 present).  The 20-level grid B is held to the same floors where they do not depend on the number of levels; the
number of layers an ascent passes through, and the number of levels inside the most-unstable parcel's 300 hPa window, are
proportional to it, so the floor on >= 3 sign changes and the number of distinct most-unstable indices are scaled by
nlev / 48 there, and the floor on >= 5 sign changes holds at 48 levels only."""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import parcel_oracle as po
from tests import layered_soundings as ls

GRIDS = {'A': ls.GRID_A, 'B': ls.GRID_B}


def test_generator_is_deterministic_and_exact_in_float32():
    for shape in ((48, 700, 5), (20, 333, 6), (1, 65, 3), (2, 64, 4)):
        a = ls.layered(*shape, nan_fraction=0.08)
        b = ls.layered(*shape, nan_fraction=0.08)
        c = ls.layered(*shape, nan_fraction=0.08, dtype=np.float32)
        for x, y, z in zip(a, b, c):
            assert x.shape == shape[:2] and x.dtype == np.float64 and z.dtype == np.float32
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z.astype(np.float64), equal_nan=True)
            ok = ~np.isnan(x)
            assert np.array_equal(x[ok] * 64.0, np.round(x[ok] * 64.0))
    p, t, td = ls.layered(48, 3000, 5, nan_fraction=0.08)
    q, u, ud = ls.layered(48, 3000, 5)
    assert np.array_equal(p, q) and not np.isnan(p).any() and np.all(np.diff(p, axis=0) < 0)
    blank = np.isnan(t)
    assert np.array_equal(blank, np.isnan(td)) and 0.005 < blank.mean() < 0.05 and blank.any(axis=0).sum() > 150
    assert np.array_equal(t[~blank], u[~blank]) and np.array_equal(td[~blank], ud[~blank]) and not np.isnan(u).any()
    dd = u - ud
    assert np.all(dd[1:] >= 0.25) and set(np.unique(dd[1:])) == set(ls.DEPRESSIONS)           # only a surface can be saturated
    sat = dd[0] == 0.0
    assert 0.015 < sat.mean() < 0.045 and np.all(dd[0][~sat] >= 0.25)


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_census(name):
    nlev, ncol, seed = GRIDS[name]
    p, t, td = ls.grid(nlev, ncol, seed)
    scale = nlev / 48.0
    for parcel in ls.PARCELS:
        ref = co.cape_cin_grid(p, t, td, parcel=parcel, moist='rk4', want_profile=True)
        net = co.cape_cin_grid(p, t, td, parcel=parcel, moist='rk4', **ls.OPTION_SETS[2])
        clamped = co.cape_cin_grid(p, t, td, parcel=parcel, moist='rk4', **ls.OPTION_SETS[4])
        c = ls.census(ref)
        ge3, ge5 = int((c['changes'] >= 3).sum()), int((c['changes'] >= 5).sum())
        acts = net['cin'] > 0.0
        print('grid %s (%d x %d, seed %d) %s: >= 3 sign changes %d, >= 5 %d, most %d; LFC replaced by LCL %d; positive net-sum '
              'CIN %d; exact-zero nodes %d; LCL on the parcel level %d; LFC without EL %d'
              % (name, nlev, ncol, seed, parcel, ge3, ge5, c['changes'].max(), c['lfc_is_lcl'].sum(), acts.sum(),
                 c['zero_nodes'].sum(), c['lcl_on_parcel'].sum(), c['lfc_no_el'].sum()))
        assert ge3 >= 0.08 * scale * ncol, (parcel, ge3)
        if nlev == 48:
            assert ge5 >= 0.005 * ncol, (parcel, ge5)
        assert acts.sum() >= 0.15 * ncol, (parcel, int(acts.sum()))
        # ... and post_zero_cin clamps exactly those, leaving CAPE and every other column alone
        assert np.all(clamped['cin'][acts] == 0.0) and np.array_equal(clamped['cin'][~acts], net['cin'][~acts], equal_nan=True)
        assert np.array_equal(clamped['cape'], net['cape'], equal_nan=True)
        assert c['zero_nodes'].sum() == 0, parcel
        assert c['lcl_on_parcel'].sum() <= 0.08 * ncol, parcel
        assert c['lfc_is_lcl'].sum() >= 0.15 * ncol and c['lfc_no_el'].sum() >= 20, parcel
        if parcel == 'most_unstable':
            idx = ref['parcel_index']
            counts = np.bincount(idx[idx >= 0])
            print('grid %s most-unstable parcel_index > 0 in %d columns; per index %s' % (name, (idx > 0).sum(), counts.tolist()))
            assert (idx > 0).sum() >= 0.40 * ncol
            assert (counts >= 0.005 * ncol).sum() >= int(10 * scale), counts


def test_sensitivity_to_post_zero_cin():
    """The margin the GPU comparison at O4 rests on: the oracle with the flag dropped (O2) disagrees with the O4 reference, by
    far more than the comparison's 1e-6 J/kg, in >= 15 % of the columns of grid A -- every parcel kind."""
    p, t, td = ls.grid(*ls.GRID_A)
    for parcel in ls.PARCELS:
        o4 = co.cape_cin_grid(p, t, td, parcel=parcel, moist='rk4', **ls.OPTION_SETS[4])
        o2 = co.cape_cin_grid(p, t, td, parcel=parcel, moist='rk4', **ls.OPTION_SETS[2])
        with np.errstate(invalid='ignore'):
            differs = np.abs(o4['cin'] - o2['cin']) > 1e-3
        print('%s: dropping post_zero_cin changes CIN in %d of %d columns' % (parcel, differs.sum(), differs.size))
        assert differs.sum() >= 0.15 * differs.size


def test_numpy_and_c_oracle_agree():
    nlev, ncol, seed = ls.GRID_ORACLES
    p, t, td = (a[:, ::2] for a in ls.grid(nlev, ncol, seed))
    fn = {'surface': po.surface_based_cape_cin, 'most_unstable': po.most_unstable_cape_cin, 'mixed_layer': po.mixed_layer_cape_cin}
    lifts = failed = values = on_parcel = 0
    worst = {'cape': 0.0, 'cin': 0.0, 'lfc_pressure': 0.0, 'el_pressure': 0.0}
    po.set_moist_lapse('rk4')
    try:
        for parcel in ls.PARCELS:
            for kw in ls.OPTION_SETS:
                got = co.cape_cin_grid(p, t, td, parcel=parcel, moist='rk4', **kw)
                for c in range(p.shape[1]):
                    lifts += 1
                    try:
                        with np.errstate(all='ignore'):
                            res = fn[parcel](p[:, c], t[:, c], td[:, c], per_column_lcl=True, **kw)
                    except RuntimeError as e:                     # the NumPy oracle gives up where the C oracle raises a status bit
                        assert 'Failed to converge' in str(e) and parcel == 'mixed_layer', (parcel, c, e)
                        assert got['status'][c] & 2, (parcel, c, got['status'][c])
                        failed += 1
                        continue
                    want = dict(res[0], **{k: res[1][k] for k in ('lfc_pressure', 'el_pressure', 'lfc_index', 'el_index')})
                    for k, tol in (('cape', 1e-6), ('cin', 1e-6), ('lfc_pressure', 1e-7), ('el_pressure', 1e-7)):
                        a, b = got[k][c], want[k]
                        assert np.isnan(a) == np.isnan(b), (parcel, kw, c, k, a, b)
                        if not np.isnan(a):
                            values += 1
                            worst[k] = max(worst[k], abs(a - b))
                            assert abs(a - b) <= tol, (parcel, kw, c, k, a, b)
                    # (the LCL of a saturated parcel is its own level: whether a crossing ON it is labelled with its interval or
                    # as "replaced by the LCL" hangs on the last bit of exp(log p) in NumPy's and in the C library's libm --
                    # tests/test_gpu_parity.py::_saturated_tie_columns, case (a); the values above are held all the same)
                    if got['lcl_pressure'][c] == res[1]['pressure'][0]:
                        on_parcel += 1
                        continue
                    assert got['lfc_index'][c] == want['lfc_index'] and got['el_index'][c] == want['el_index'], (parcel, kw, c)
    finally:
        po.set_moist_lapse('ode')
    print('NumPy against C oracle: %d lifts, %d the NumPy oracle does not converge on, %d values, worst %s'
          % (lifts, failed, values, ', '.join('%s %.3g' % kv for kv in worst.items())))
    assert lifts == 120 * 3 * 5 and failed <= 0.02 * lifts and values >= 3000 and on_parcel <= 0.08 * lifts
