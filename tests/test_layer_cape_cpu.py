"""CAPE / CIN over per-column layers without a GPU: the NumPy restatement on hand-built profiles whose areas are known in
closed form and on the edge rules, the C ABI declaration against ctypes, the array API and the DataArray module around a
stubbed launch, and the operating point of the kernel (cross-compiled for gfx950)."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle.thermo import RD
from tests import layer_cape_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from tests.test_effective_layer_cpu import VD, _grid, _horiz
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import layer_cape
from xarray_parcel_amd import numpy_api as api

# -- hand-built profiles ------------------------------------------------------------------------------------------------------
# y = parcel - environment = -2 + 10 u, u = ln(1000 / p): linear in ln p through every node, zero (the LFC) at u = 0.2, no EL.
# With G+(u) = 5 (u - 0.2)^2 for u > 0.2 and G-(u) = 5 u^2 - 2 u for u < 0.2 (-0.2 from there on):
#   CAPE between the bounds = Rd (G+(u_top) - G+(u_bottom)),  CIN = Rd (G-(u_top) - G-(u_bottom)).
P = np.array([1000.0, 950.0, 900.0, 850.0, 800.0, 700.0, 600.0, 500.0, 400.0])
U = np.log(1000.0 / P)
ENV = np.full(P.size, 280.0)
PAR = ENV - 2.0 + 10.0 * U
LFC = 1000.0 * np.exp(-0.2)


def g_pos(p):
    u = np.log(1000.0 / p)
    return 5.0 * max(u - 0.2, 0.0) ** 2


def g_neg(p):
    u = min(np.log(1000.0 / p), 0.2)
    return 5.0 * u * u - 2.0 * u


def layer(pb, pt, p=P, par=PAR, env=ENV, lfc=LFC, el=np.nan):
    return R.layer_column(p, par, env, lfc, el, pb, pt)


@pytest.mark.parametrize('pb,pt', [(975.0, 620.0), (900.0, 850.0), (830.0, 810.0), (990.0, 960.0), (640.0, 450.0),
                                   (LFC, 500.0), (1000.0, LFC), (850.0, 700.0)])
def test_linear_profile_has_its_closed_form_areas(pb, pt):
    cape, cin = layer(pb, pt)
    assert cape == pytest.approx(RD * (g_pos(pt) - g_pos(pb)), rel=1e-12, abs=1e-10)
    assert cin == pytest.approx(RD * (g_neg(pt) - g_neg(pb)), rel=1e-12, abs=1e-10)
    assert cape >= 0.0 and cin <= 0.0


def test_abutting_layers_sum_to_the_whole_ascent():
    total = R.c_oracle.cape_cin_base(P, ENV, LFC, np.nan, PAR)
    assert total['cape'] == pytest.approx(RD * g_pos(400.0), rel=1e-12) and total['cin'] == pytest.approx(-0.2 * RD, rel=1e-12)
    parts = [layer(None, 870.0), layer(870.0, 655.0), layer(655.0, 1e-3)]
    assert sum(c for c, _ in parts) == pytest.approx(total['cape'], rel=1e-12)
    assert sum(n for _, n in parts) == pytest.approx(total['cin'], rel=1e-12)
    assert layer(None, 1e-3) == (total['cape'], total['cin'])


def test_an_el_caps_the_layer():
    """An EL at u = 0.6 on a profile that turns around at 600 hPa: nothing above the EL counts, whatever the top."""
    y = np.where(U <= np.log(1000.0 / 600.0), -2.0 + 10.0 * U, np.nan)
    u6 = np.log(1000.0 / 600.0)
    y = np.where(np.isnan(y), (-2.0 + 10.0 * u6) * (1.0 - (U - u6) / 0.1), y)      # falls to 0 at u6 + 0.1, negative above
    el = 1000.0 * np.exp(-(u6 + 0.1))
    whole = R.c_oracle.cape_cin_base(P, ENV, LFC, el, ENV + y)['cape']
    assert layer(None, 300.0, par=ENV + y, el=el)[0] == pytest.approx(whole, rel=1e-12)
    assert layer(700.0, 450.0, par=ENV + y, el=el)[0] == pytest.approx(whole - RD * g_pos(700.0), rel=1e-12)
    assert layer(el - 1.0, 410.0, par=ENV + y, el=el) == (0.0, 0.0)            # wholly above the EL
    assert layer(990.0, 900.0, par=ENV + y, el=el)[0] == 0.0                     # wholly below the LFC


def test_edge_rules():
    nan = np.nan
    assert np.isnan(layer(900.0, nan)).all() and np.isnan(layer(None, nan)).all()          # NaN top: no layer
    assert np.isnan(layer(800.0, 800.0)).all() and np.isnan(layer(700.0, 900.0)).all()     # top >= bottom: no layer
    assert layer(nan, 700.0) == layer(None, 700.0) == layer(1050.0, 700.0) == layer(1000.0, 700.0)   # from the first node
    assert layer(800.0, 300.0) == layer(800.0, 400.0) == layer(800.0, 1e-3)                # to the top
    assert layer(350.0, 300.0) == (0.0, 0.0)                                               # above the column
    assert layer(900.0, 700.0, lfc=nan) == (0.0, 0.0)                                      # no LFC: no CAPE, no CIN
    # an interval with a NaN end contributes nothing, and a bound inside it takes the sum below it
    par = PAR.copy()
    par[5] = nan                                                                           # 700 hPa: (800, 700) and (700, 600) drop out
    cape, cin = layer(None, 1e-3, par=par)
    assert cape == pytest.approx(RD * (g_pos(800.0) + g_pos(400.0) - g_pos(600.0)), rel=1e-12)
    assert layer(None, 750.0, par=par)[0] == pytest.approx(RD * g_pos(800.0), rel=1e-12)
    assert layer(650.0, 1e-3, par=par)[0] == pytest.approx(RD * (g_pos(400.0) - g_pos(600.0)), rel=1e-12)
    p = P.copy()
    p[5] = nan                                                                             # the same with the pressure missing
    assert layer(None, 750.0, p=p, par=par)[0] == pytest.approx(RD * g_pos(800.0), rel=1e-12)


def test_grid_marks_no_layer_and_blanks():
    """layers_grid on three columns: an ordinary one, one whose surface is missing a dewpoint (NaN parcel: 0.0), and the
    status bit of a NaN top."""
    from tests.test_effective_layer_cpu import sounding
    p, t, td, z = sounding()
    p3, t3, td3 = (np.repeat(a[:, None], 3, axis=1) for a in (p, t, td))
    td3[0, 1] = np.nan
    top = np.array([600.0, 600.0, np.nan])
    r = R.layers_grid(p3, t3, td3, [None, np.full(3, 800.0)], [top, np.full(3, 500.0)], parcel='surface', moist='rk4')
    assert r['cape'].shape == (2, 3) and r['cape'][0, 0] > 0.0 and r['cape'][1, 0] > 0.0
    assert r['cape'][0, 0] + 1e-9 < r['total_cape'][0] and r['cape'][:, 1].tolist() == [0.0, 0.0] and r['cin'][:, 1].tolist() == [0.0, 0.0]
    assert np.isnan(r['cape'][0, 2]) and r['cape'][1, 2] == r['cape'][1, 0]
    assert (r['status'] & R.ST_NO_LAYER).tolist() == [0, 0, R.ST_NO_LAYER]


# -- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_follows_the_header():
    assert _struct_fields('xp_cape_layers_out') == [f[0] for f in L.CapeLayersOut._fields_]
    assert C.sizeof(L.CapeLayersOut) == 8 * (2 * L.CAPE_MAX_LAYERS + 5 + 1) + 8
    kinds = _prototypes()['xp_cape_cin_layers']
    got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES['xp_cape_cin_layers']]
    assert got == kinds == ['pointer'] * 5 + ['int32'] + ['pointer'] * 4
    assert 'xp_cape_cin_layers' in L.SYMBOLS and L.XP_ST_NO_LAYER == R.ST_NO_LAYER


# -- the array API and the DataArray module around a stubbed launch -------------------------------------------------------------
def test_array_api_arguments(monkeypatch):
    seen = []

    def run(self, name, *args):
        seen.append((name, args))
    monkeypatch.setattr(api._Call, 'run', run)
    p = np.linspace(1000.0, 200.0, 9, dtype=np.float32)[:, None] * np.ones((1, 5), np.float32)
    tops = np.arange(5.0) * 10 + 600
    res = api.cape_cin_layers(p, p, p, [{'top': tops}, {'bottom': 900.0, 'top': 500.0}], parcel='most_unstable', moist='table')
    name, (pv, tv, tdv, pc, o, n, bottom, top, out) = seen[-1]
    assert name == 'xp_cape_cin_layers' and (pv.nlev, pv.ncol, pv.dtype) == (9, 5, L.XP_F32) and n == 2
    assert pc.mode == L.PARCEL['most_unstable'] and pc.depth == 300.0 and o.moist_mode == L.MOIST['table'] and o.pos_cape_neg_cin == 1
    assert bottom[0] is None and bottom[1] is not None and top[0] is not None and len(top) == 2
    assert set(res) == {'cape', 'cin', 'bottom_pressure', 'top_pressure', 'status'} | set(R.TOTALS)
    assert res['cape'].shape == (2, 5) and res['cape'].dtype == np.float32 and res['status'].dtype == np.int32
    assert out.cape[1] == res['cape'][1].ctypes.data and out.cin[0] == res['cin'][0].ctypes.data and out.cape[2] is None
    assert out.total_cape == res['total_cape'].ctypes.data and out.dtype == L.XP_F32 and out.mem == L.XP_MEM_HOST
    assert np.isnan(res['bottom_pressure'][0]).all() and np.all(res['bottom_pressure'][1] == 900.0)
    assert np.array_equal(res['top_pressure'][0], tops.astype(np.float32))
    # bounds by height and temperature go through interp_level / crossing_level first
    seen.clear()
    z = np.linspace(0.0, 12000.0, 9, dtype=np.float32)[:, None] * np.ones((1, 5), np.float32)
    api.hail_growth_zone_cape(p, p, p, z)
    assert [s[0] for s in seen] == ['xp_crossing_level', 'xp_interp_level', 'xp_crossing_level', 'xp_interp_level', 'xp_cape_cin_layers']
    assert seen[0][1][2] == 263.15 and seen[2][1][2] == 243.15
    seen.clear()
    api.cape_3km(p, p, p, z, parcel='mixed_layer')
    assert [s[0] for s in seen] == ['xp_interp_level', 'xp_cape_cin_layers'] and seen[1][1][6][0] is None and seen[1][1][5] == 1
    assert np.all(seen[0][1][2] == 3000.0)                                               # z0 + 3000 m with z0 = 0
    for bad in ([], [{'top': 500.0}] * 5, [{'bottom': 900.0}], [{'top': 500.0, 'top_height': 3000.0}], [{'top_height': 3000.0}],
                [{'top': 500.0, 'depth': 100.0}]):
        with pytest.raises(AssertionError):
            api.cape_cin_layers(p, p, p, bad)
    with pytest.raises(AssertionError):
        api.cape_cin_layers(p, p, p, [{'top': 500.0}], humidity='specific')


def test_mirror_wraps_the_array_api(monkeypatch):
    calls = []

    def run(self, name, *args):
        calls.append((name, args))
    monkeypatch.setattr(api._Call, 'run', run)
    lev = np.arange(1., 10.)
    args = (_grid(1000. - 50 * lev, 'p'), _grid(300. - lev, 't'), _grid(290. - lev, 'td'))
    ds = layer_cape.cape_cin_layers(*args, [{'top': _horiz(700.0, 'pt')}, {'bottom': 900.0, 'top': 600.0}], parcel='mixed_layer')
    name, a = calls[-1]
    assert name == 'xp_cape_cin_layers' and (a[0].nlev, a[0].ncol) == (9, 6) and a[5] == 2 and a[3].mode == L.PARCEL['mixed_layer']
    assert ds['cape'].dims == ('layer', 'lat', 'lon') and ds['cape'].shape == (2, 2, 3) and ds['cape'].attrs['units'] == 'J kg$^{-1}$'
    assert list(ds['cin'].coords['layer']) == [0, 1] and ds['top_pressure'].attrs['units'] == 'hPa'
    assert ds['total_cape'].dims == ('lat', 'lon') and ds['status'].values.dtype == np.int32 and ds['lcl_pressure'].attrs['long_name']
    z = _grid(500. * lev, 'z')
    da = layer_cape.cape_3km(*args, z)
    assert da.dims == ('lat', 'lon') and da.name == 'cape_3km' and da.attrs['units'] == 'J kg$^{-1}$'
    da = layer_cape.hail_growth_zone_cape(*args, z, parcel='most_unstable')
    assert da.name == 'hail_growth_zone_cape' and 'long_name' in da.attrs and calls[-1][1][3].mode == L.PARCEL['most_unstable']


def test_parcel_functions_gains_nothing():
    from xarray_parcel_amd import parcel_functions as pf
    for name in ('cape_cin_layers', 'cape_3km', 'hail_growth_zone_cape'):
        assert not hasattr(pf, name) and hasattr(layer_cape, name) and hasattr(api, name)


# -- kernel resources -----------------------------------------------------------------------------------------------------------
@needs_hipcc
def test_kernel_keeps_128_vgprs_without_spills_and_two_workgroups_per_cu(tmp_path):
    """The four instantiations (f64 / f32 x RK4 / lookup tables), compiled as the library compiles them, in the unit's own
    flags: at most 128 VGPRs, no scratch at all (ScratchSize 0, no scratch instruction in the body), and the LDS -- the
    e_s / ln table, 13 Scan slots and 16 bound slots per thread -- within 80 KB, i.e. two workgroups per CU."""
    unit = [u for u in L.UNITS if u[1] == 'xp_cape_layers_tu.hip']
    assert len(unit) == 1 and '-disable-machine-licm' in unit[0][2]
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    kernels = [n for n in rec if re.search(r'k_cape_layersI', n)]
    assert len(kernels) == 4, sorted(rec)
    for n in kernels:
        print(n, rec[n])
        assert rec[n]['in_asm'] and not rec[n]['scratch_insts'], n
        assert rec[n]['vgprs'] <= 128 and rec[n]['scratch'] == 0 and rec[n]['vgpr_spill'] == 0, (n, rec[n])
        assert rec[n]['lds'] <= 80 * 1024, (n, rec[n])
