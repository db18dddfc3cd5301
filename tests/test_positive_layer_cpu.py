"""The positive-layer choice of the CAPE / CIN calls (xp_opts.flags, XP_OPT_LAYER_*) without a GPU: the NumPy restatement
(tests/positive_layer_restatement.py) on a profile whose areas are known in closed form, on hand-built event lists and
against the reference's own rule on the layered grid; a census of that grid; the header, the binding and the struct sizes;
the array API and the DataArray module around a stubbed launch; and the kernel's resources (cross-compiled for gfx950)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle.thermo import RD
from tests import positive_layer_cases as K
from tests import positive_layer_restatement as R
from tests.resource_report import needs_hipcc, resources
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd import positive_layer as mirror
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'


# -- the restatement on hand-built input ------------------------------------------------------------------------------------
# y = parcel - environment on nodes 0.1 apart in u = ln(1000 / p), the LCL on node 0:
#   -1, 1, 1, -1, -1, 2, 2, -2: an UP at u = 0.05, a DOWN at 0.25, an UP at 0.4 + 0.1 / 3, a DOWN at 0.65.
# F+ at the four crossings: 0, 0.15, 0.15, 0.15 + 0.2 / 3 + 0.2 + 0.05; F-: -0.025, -0.025, -0.025 - 0.025 - 0.1 - 0.05 / 3.
Y = np.array([-1.0, 1.0, 1.0, -1.0, -1.0, 2.0, 2.0, -2.0])
U = 0.1 * np.arange(Y.size)
P = 1000.0 * np.exp(-U)
ENV = np.full(Y.size, 280.0)


def test_two_humps_have_their_closed_form_layers():
    default = dict(cape=-1.0, cin=-1.0, lfc_pressure=-1.0, lfc_temperature=-1.0, el_pressure=-1.0, el_temperature=-1.0, lfc_index=-9, el_index=-9)
    c = R.column(P, ENV + Y, ENV, P[0], 281.0, default)
    assert c['K'] == 2 and [e['kind'] for e in c['events']] == ['up', 'down', 'up', 'down']
    assert [e['index'] for e in c['events']] == [0, 2, 4, 6]
    low, high = c['layers']
    approx = lambda v: pytest.approx(v, rel=1e-12, abs=1e-13)
    assert np.log(1000.0 / low['L']) == approx(0.05) and np.log(1000.0 / low['E']) == approx(0.25)
    assert np.log(1000.0 / high['L']) == approx(0.4 + 0.1 / 3) and np.log(1000.0 / high['E']) == approx(0.65)
    assert (low['cL'], low['cE'], low['nL']) == (approx(0.0), approx(0.15), approx(-0.025))
    assert (high['cL'], high['cE'], high['nL']) == (approx(0.15), approx(0.15 + 0.2 / 3 + 0.25), approx(-0.15 - 0.05 / 3))
    assert low['tL'] == approx(280.0) and high['tE'] == approx(280.0) and not low['open'] and not high['open']
    assert c['picked'] == {'lowest': 0, 'highest': 1, 'deepest': 1, 'most_cape': 1}
    assert c['lowest']['cape'] == approx(RD * 0.15) and c['lowest']['cin'] == approx(-RD * 0.025)
    assert c['most_cape']['cape'] == approx(RD * (0.2 / 3 + 0.25)) and c['most_cape']['cin'] == approx(-RD * (0.15 + 0.05 / 3))
    assert (c['lowest']['lfc_index'], c['lowest']['el_index'], c['highest']['lfc_index'], c['highest']['el_index']) == (0, 2, 4, 6)
    # equivalently: cape_cin_base for the chosen LFC / EL
    for ch in R.CHOICES:
        b = co.cape_cin_base(P, ENV, c[ch]['lfc_pressure'], c[ch]['el_pressure'], ENV + Y)
        assert c[ch]['cape'] == approx(b['cape']) and c[ch]['cin'] == approx(b['cin'])
    # the first interval is not in the selected set when env[0] == par[0]: the first UP goes, the first DOWN closes a layer from the LCL
    y = Y.copy()
    y[0] = 0.0
    c = R.column(P, ENV + y, ENV, P[0], 281.0, default)
    assert [e['kind'] for e in c['events']] == ['down', 'up', 'down'] and c['K'] == 2
    assert c['layers'][0]['iL'] == -2 and c['layers'][0]['L'] == P[0] and c['layers'][0]['tL'] == 281.0 and c['layers'][0]['cL'] == 0.0
    # one hump only: every choice is the default, whatever it holds
    c = R.column(P[:5], (ENV + Y)[:5], ENV[:5], P[0], 281.0, default)
    assert c['K'] == 1 and all(c[ch] == default for ch in R.CHOICES) and c['picked']['deepest'] == -1
    # a NaN LCL: no walk at all
    assert R.column(P, ENV + Y, ENV, np.nan, np.nan, default)['K'] == 0


def _ev(kind, x, fp, fn=0.0, index=0):
    return dict(kind=kind, x=x, t=250.0 + x, index=index, fp=fp, fn=fn)


def test_layer_rules_on_event_lists():
    lcl_p, lcl_t, min_p = 900.0, 285.0, 100.0
    lay = lambda ev, fp=9.0: R.layers_of(ev, (0.5, -0.25), fp, min_p, lcl_p, lcl_t)
    # a first DOWN closes a layer that began at the LCL; a second DOWN before any UP is ignored
    got = lay([_ev('down', 6.5, 1.5, index=3), _ev('down', 6.4, 1.5, index=4), _ev('up', 6.3, 1.5, -1.0, 5), _ev('down', 6.0, 2.5, -1.0, 7)])
    assert len(got) == 2 and (got[0]['iL'], got[0]['L'], got[0]['tL'], got[0]['cL'], got[0]['nL'], got[0]['iE']) == (-2, lcl_p, lcl_t, 0.5, -0.25, 3)
    assert (got[1]['iL'], got[1]['iE'], got[1]['cL'], got[1]['cE'], got[1]['nL']) == (5, 7, 1.5, 2.5, -1.0)
    # an UP while a layer is open is ignored; a layer open at the top ends at the lowest valid pressure with the final F+
    got = lay([_ev('up', 6.6, 0.0, -0.1, 1), _ev('up', 6.5, 0.7, -0.1, 2), _ev('down', 6.2, 1.0, -0.1, 4), _ev('up', 6.0, 1.0, -0.3, 6)])
    assert len(got) == 2 and (got[0]['iL'], got[0]['cL'], got[0]['iE']) == (1, 0.0, 4)
    top = got[1]
    assert top['open'] and top['E'] == min_p and top['cE'] == 9.0 and top['iE'] == -1 and np.isnan(top['tE'])
    r = R.result(top)
    assert np.isnan(r['el_pressure']) and np.isnan(r['el_temperature']) and r['el_index'] == -1 and r['cape'] == RD * 8.0 and r['cin'] == RD * -0.3
    # a DOWN between two layers is ignored
    got = lay([_ev('up', 6.6, 0.0), _ev('down', 6.5, 1.0), _ev('down', 6.4, 1.0), _ev('up', 6.3, 1.0), _ev('down', 6.2, 3.0)])
    assert [(g['xL'], g['xE']) for g in got] == [(6.6, 6.5), (6.3, 6.2)]
    # a first DOWN ON the LCL (within 2e-9 in ln p) closes nothing: the layer from the LCL would have no depth
    x_lcl = float(np.log(lcl_p))
    got = lay([_ev('down', x_lcl - 1e-10, 0.5, index=1), _ev('up', 6.3, 0.5, -1.0, 5), _ev('down', 6.0, 2.5, -1.0, 7)])
    assert len(got) == 1 and (got[0]['iL'], got[0]['iE']) == (5, 7)
    assert len(lay([_ev('down', x_lcl - 1e-8, 0.5, index=1), _ev('up', 6.3, 0.5, -1.0, 5), _ev('down', 6.0, 2.5, -1.0, 7)])) == 2
    assert lay([]) == []


def test_selection_takes_the_lower_of_equals_and_no_nan():
    mk = lambda xl, xe, cl, ce: dict(xL=xl, xE=xe, cL=cl, cE=ce)
    equal = [mk(6.5, 6.25, 0.0, 2.0), mk(6.0, 5.75, 2.0, 4.0), mk(5.5, 5.25, 4.0, 6.0)]
    assert [R.choose(equal, ch) for ch in R.CHOICES] == [0, 2, 0, 0]
    later = [mk(6.5, 6.25, 0.0, 2.0), mk(6.0, 5.5, 2.0, 4.5), mk(5.25, 4.75, 4.5, 7.0)]
    assert [R.choose(later, ch) for ch in R.CHOICES] == [0, 2, 1, 1]
    nan = [mk(6.5, 6.25, 0.0, 2.0), mk(6.0, np.nan, 2.0, np.nan), mk(5.5, 5.4, 4.0, 4.5)]
    assert R.choose(nan, 'deepest') == 0 and R.choose(nan, 'most_cape') == 0
    assert R.choose([mk(np.nan, 6.0, np.nan, 1.0), mk(6.0, 5.0, 1.0, 3.0)], 'deepest') == 0          # the first is taken, then only a greater one


# -- the restatement against the reference's rule, on the layered grid ------------------------------------------------------
@pytest.mark.parametrize('parcel', K.PARCELS)
def test_restatement_against_the_references_rule(parcel):
    """On GRID_REPLAY: the bottom UP and the top DOWN of the restatement's events are the oracle's LFC and EL wherever the
    oracle labels them with an interval (the events are lfc_el's candidates); for every choice the chosen layer's cape / cin
    equal the oracle's cape_cin_base fed its LFC / EL pressures (tests/test_layer_cape_cpu.py's tolerance for the same
    identity: rel 1e-12, abs 1e-10); and the columns with K <= 1 hold the oracle's default result exactly."""
    g = K.restated(parcel)
    o = g['oracle']
    prof = o['profile']
    n_lfc = n_el = 0
    for j, c in enumerate(g['columns']):
        ups = [e for e in c['events'] if e['kind'] == 'up']
        downs = [e for e in c['events'] if e['kind'] == 'down']
        if o['lfc_index'][j] >= 0:
            n_lfc += 1
            assert ups and ups[0]['index'] == o['lfc_index'][j], j
            assert np.exp(ups[0]['x']) == pytest.approx(o['lfc_pressure'][j], rel=1e-12) and ups[0]['t'] == pytest.approx(o['lfc_temperature'][j], rel=1e-12)
        if o['el_index'][j] >= 0:
            n_el += 1
            assert downs and downs[-1]['index'] == o['el_index'][j], j
            assert np.exp(downs[-1]['x']) == pytest.approx(o['el_pressure'][j], rel=1e-12) and downs[-1]['t'] == pytest.approx(o['el_temperature'][j], rel=1e-12)
    assert n_lfc >= 500 and n_el >= 1000, (n_lfc, n_el)
    many = np.nonzero(g['K'] >= 2)[0]
    few = g['K'] <= 1
    worst = 0.0
    for ch in R.CHOICES:
        r = g[ch]
        for j in many:
            b = co.cape_cin_base(prof['pressure'][:, j], prof['environment_virtual_temperature'][:, j], r['lfc_pressure'][j], r['el_pressure'][j],
                                 prof['virtual_temperature'][:, j])
            for k in ('cape', 'cin'):
                err = abs(r[k][j] - b[k])
                worst = max(worst, err)
                assert err <= 1e-12 * abs(b[k]) + 1e-10, (ch, j, k, r[k][j], b[k])
        for k in R.FIELDS + R.INDICES:
            assert np.array_equal(r[k][few], o[k][few], equal_nan=True), (ch, k)
        assert np.all(r['cape'][many] >= 0.0) and np.all(r['cin'][many] <= 0.0)
    print('%s: %d columns with K >= 2, worst |restatement - cape_cin_base| %.3e J/kg' % (parcel, many.size, worst))


# -- census of the device tests' input ----------------------------------------------------------------------------------------
# parcel -> K >= 2, K >= 3, columns whose cape differs from the default's per choice, columns where deepest != most_cape
MEASURED = {'surface': (495, 59, 495, 434, 442, 441, 18), 'most_unstable': (334, 26, 334, 282, 292, 292, 13),
            'mixed_layer': (524, 62, 524, 474, 477, 479, 30)}


@pytest.mark.parametrize('parcel', K.PARCELS)
def test_census_of_the_layered_grid(parcel):
    """Counted with the restatement on the C oracle's RK4 profiles of GRID_REPLAY (40 x 3000, seed 11), per parcel
    surface / most_unstable / mixed_layer: K >= 2 in 495 / 334 / 524 columns, K >= 3 in 59 / 26 / 62 (most: 5 / 3 / 4);
    the cape differs from the default's for lowest in 495 / 334 / 524 columns, highest 434 / 282 / 474, deepest
    442 / 292 / 477, most_cape 441 / 292 / 479; the deepest layer is not the one with the most CAPE in 18 / 13 / 30.  The
    first event is a DOWN (a layer that began at the LCL) in 1048 / 1755 / 1057 columns, an UP falls into an open layer in
    3 / 2 / 1, and the last layer is open at the top in 12 / 10 / 3.  The floors are the issue's 150 and 12 and half of the
    other counts."""
    c = K.census(K.restated(parcel))
    print(parcel, c)
    m = MEASURED[parcel]
    assert c['K>=2'] >= 150 and c['K>=3'] >= 12
    assert c['K>=2'] >= m[0] // 2 and c['K>=3'] >= m[1] // 2
    for ch, measured in zip(K.CHOICES, m[2:6]):
        assert c[ch] >= measured // 2, (ch, c[ch])
    assert c['deepest!=most_cape'] >= m[6] // 2
    assert c['first_down'] >= 500 and c['up_while_open'] >= 1 and c['open_top'] >= 1
    for a in K.grid():
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64), equal_nan=True)          # exact in float32


# -- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    enum = hdr[hdr.index('enum { XP_OPT_LAYER_SHIFT'):]
    enum = enum[:enum.index('};')]
    values = {k: eval(v) for k, v in re.findall(r'(XP_OPT_LAYER_\w+) = ([0-9 <]+)', enum)}
    assert values == {'XP_OPT_LAYER_SHIFT': 4, 'XP_OPT_LAYER_MASK': 7 << 4, 'XP_OPT_LAYER_ENVELOPE': 0, 'XP_OPT_LAYER_LOWEST': 16,
                      'XP_OPT_LAYER_HIGHEST': 32, 'XP_OPT_LAYER_DEEPEST': 48, 'XP_OPT_LAYER_MOST_CAPE': 64}
    assert L.POSITIVE_LAYER == K.FLAGS == {k[len('XP_OPT_LAYER_'):].lower(): v for k, v in values.items() if k[13:] not in ('SHIFT', 'MASK')}
    assert (L.OPT_LAYER_SHIFT, L.OPT_LAYER_MASK) == (4, 112) and L.OPT_FUSE_PARCELS & L.OPT_LAYER_MASK == 0
    assert L.WHICH_LFC_EL == K.PAIRS
    section = hdr[hdr.index('WHICH POSITIVE LAYER'):hdr.index('enum { XP_OPT_LAYER_SHIFT')]
    for rule in ('EVENTS', 'POSITIVE LAYERS', 'SELECTION', 'RESULT', 'K <= 1', 'an UP while one is open is ignored', 'lfc_index = -2',
                 'el_index = -1', 'ln L - ln E', "NOT MetPy's difference in hPa", 'cE - cL', 'the lower of equals wins', 'a NaN metric never wins',
                 'xp_cape_cin_base', 'XP_OPT_FUSE_PARCELS is ignored', 'XP_MOIST_FAMILY is treated as exact', 'pos_cape_neg_cin must be set',
                 'a value 5 ... 7', 'a non-NULL profile', 'compute = XP_F32', 'xp_cape_cin_layers, xp_effective_inflow_layer, xp_conv_properties',
                 'With the field 0 nothing changes by a bit'):
        assert rule in section, rule


def test_struct_sizes_are_unchanged_and_no_new_entry_point():
    assert C.sizeof(L.Opts) == 32 and C.sizeof(L.Parcel) == 40 and C.sizeof(L.ScalarsOut) == 16 * 8 + 8
    assert [f[0] for f in L.Opts._fields_][-1] == 'flags'
    assert len(L.SYMBOLS) == 56 and not [s for s in L.SYMBOLS if 'pick' in s or 'positive' in s]
    assert [u for u in L.UNITS if u[1] == 'xp_cape_pick_tu.hip'] == [('cape_pick', 'xp_cape_pick_tu.hip', ['-mllvm', '-disable-machine-licm'])]


# -- the array API and the DataArray module around a stubbed launch ---------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def run(self, name, *args):
        opts = args[5] if name == 'xp_cape_cin_multi' else args[4]
        seen.append(dict(name=name, opts=bytes(opts), flags=opts.flags, args=args))
    monkeypatch.setattr(api._Call, 'run', run)
    return seen


def _small(dtype=np.float32, ncol=6):
    return tuple(np.ascontiguousarray(a[:, :ncol], dtype=dtype) for a in K.grid())


def test_default_calls_are_unchanged_and_every_spelling_sets_its_bits(calls):
    p, t, td = _small()
    api.cape_cin_columns(p, t, td)
    assert calls[-1]['flags'] == 0 and calls[-1]['opts'] == bytes(api._opts())
    api.cape_cin_columns(p, t, td, parcel='most_unstable', moist='family', post_zero_cin=True, want_profile=True)
    assert calls[-1]['flags'] == 0 and calls[-1]['opts'] == bytes(api._opts(moist='family', post_zero_cin=True))
    api.cape_cin_multi(p, t, td, ['surface', 'mixed_layer'])
    assert calls[-1]['flags'] == 0
    api.cape_cin_multi(p, t, td, ['surface', 'mixed_layer'], fused=True)
    assert calls[-1]['flags'] == L.OPT_FUSE_PARCELS
    for name, bits in K.FLAGS.items():
        api.cape_cin_columns(p, t, td, positive_layer=name, moist='table')
        want = api._opts(moist='table')
        want.flags = bits
        assert calls[-1]['name'] == 'xp_cape_cin' and calls[-1]['opts'] == bytes(want), name
        api.cape_cin_multi(p, t, td, ['surface', ('most_unstable', 250)], positive_layer=name, fused=True)
        assert calls[-1]['name'] == 'xp_cape_cin_multi' and calls[-1]['flags'] == bits | L.OPT_FUSE_PARCELS
    for (lfc, el), name in K.PAIRS.items():
        api.cape_cin_columns(p, t, td, which_lfc=lfc, which_el=el)
        assert calls[-1]['flags'] == K.FLAGS[name], (lfc, el)
        api.cape_cin_multi(p, t, td, ['surface'], which_lfc=lfc, which_el=el)
        assert calls[-1]['flags'] == K.FLAGS[name], (lfc, el)
    n = len(calls)
    for lfc, el in K.BAD_PAIRS:
        for fn, args in ((api.cape_cin_columns, ()), (api.cape_cin_multi, (['surface'],))):
            with pytest.raises(ValueError, match=r"\('bottom', 'top'\).*\('most_cape', 'most_cape'\)"):
                fn(p, t, td, *args, which_lfc=lfc, which_el=el)
    with pytest.raises(ValueError, match='not both'):
        api.cape_cin_columns(p, t, td, positive_layer='lowest', which_lfc='bottom', which_el='bottom')
    with pytest.raises(ValueError, match="'envelope', 'lowest', 'highest', 'deepest', 'most_cape'"):
        api.cape_cin_columns(p, t, td, positive_layer='widest')
    assert len(calls) == n                                                    # nothing was launched
    # a set_compute('float32') preference leaves a layer call in fp64
    api.set_compute('float32')
    try:
        api.cape_cin_columns(p, t, td, moist='family', positive_layer='highest')
        assert C.cast(calls[-1]['opts'], C.POINTER(L.Opts)).contents.compute == L.XP_F64 and calls[-1]['flags'] == 32
    finally:
        api.set_compute('float64')


def test_dataarray_module(calls):
    p, t, td = _small(np.float64)
    hc = {'lat': [10.0, 20.0], 'lon': [1.0, 2.0, 3.0]}
    on_grid = lambda a: DataArray(a.reshape(40, 2, 3).transpose(1, 0, 2), dims=('lat', VD, 'lon'), coords={**hc, VD: np.arange(40)})
    ds = mirror.cape_cin(on_grid(p), on_grid(t), on_grid(td), parcel='mixed_layer', positive_layer='most_cape')
    c = calls[-1]
    assert c['name'] == 'xp_cape_cin' and c['flags'] == 64 and c['args'][3].mode == L.PARCEL['mixed_layer'] and c['args'][6] is None
    assert (c['args'][0].nlev, c['args'][0].ncol, c['args'][0].dtype) == (40, 6, L.XP_F64)
    assert set(ds.keys()) == {'cape', 'cin', 'lfc_pressure', 'lfc_temperature', 'el_pressure', 'el_temperature'}
    assert ds['cape'].dims == ('lat', 'lon') and ds['cape'].shape == (2, 3) and ds['cape'].attrs['units'] == 'J kg$^{-1}$'
    assert ds['el_pressure'].attrs['units'] == 'hPa' and 'chosen positive layer' in ds['lfc_pressure'].attrs['long_name']
    mirror.cape_cin(on_grid(p), on_grid(t), on_grid(td), which_lfc='top', which_el='top', moist='table')
    assert calls[-1]['flags'] == 32 and calls[-1]['args'][3].mode == L.PARCEL['surface']
    mirror.cape_cin(on_grid(p), on_grid(t), on_grid(td))
    assert calls[-1]['flags'] == 0
    rh = on_grid(np.full_like(p, 0.5))
    mirror.cape_cin(on_grid(p), on_grid(t), rh, positive_layer='deepest', humidity='relative')
    assert C.cast(calls[-1]['opts'], C.POINTER(L.Opts)).contents.humidity == L.HUMIDITY['relative']
    rh.attrs['units'] = '%'
    with pytest.raises(ValueError, match='fraction'):
        mirror.cape_cin(on_grid(p), on_grid(t), rh, positive_layer='deepest', humidity='relative')
    sfc = tuple(DataArray(a[0].reshape(2, 3), dims=('lat', 'lon'), coords=hc) for a in (p, t, td))
    mirror.cape_cin(on_grid(p), on_grid(t), on_grid(td), parcel='most_unstable', positive_layer='lowest', ground=sfc)
    assert calls[-1]['args'][3].mode == L.PARCEL['most_unstable'] | L.PARCEL_OVER_GROUND and calls[-1]['flags'] == 16
    with pytest.raises(ValueError):
        mirror.cape_cin(on_grid(p), on_grid(t), on_grid(td), which_lfc='top', which_el='bottom')


def test_parcel_functions_gains_nothing():
    from xarray_parcel_amd import parcel_functions as pf
    assert not hasattr(pf, 'positive_layer') and not hasattr(pf, 'cape_cin_positive_layer') and hasattr(mirror, 'cape_cin')


# -- kernel resources -----------------------------------------------------------------------------------------------------------
@needs_hipcc
def test_kernel_resources(tmp_path):
    """The eight instantiations (f64 / f32 x RK4 / lookup tables x dewpoint / specific humidity), compiled as the library
    compiles them: ScratchSize 0 and no spilled VGPR, at most 128 VGPRs, and the LDS -- the e_s / ln table, the scan's 13
    slots and the 14 record slots per thread -- within 80 KB: two workgroups per CU.  From the compiler's resource remarks
    alone."""
    unit = [u for u in L.UNITS if u[1] == 'xp_cape_pick_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    kernels = [n for n in rec if 'k_cape_pickI' in n]
    assert len(kernels) == 8, sorted(rec)
    for n in kernels:
        r = rec[n]
        print(n, {k: r[k] for k in ('vgprs', 'vgpr_spill', 'scratch', 'occupancy', 'lds')})
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['vgprs'] <= 128, (n, r)
        assert r['lds'] <= 80 * 1024 and r['occupancy'] >= 2, (n, r)
