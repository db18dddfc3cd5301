"""Argument errors through the raw C ABI (include/xparcel.h): for each family of entry points a representative invalid
call and the code it must return, and xp_cape_cin_multi checking every parcel before it runs any of them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from xarray_parcel_amd import _lib as L
from xarray_parcel_amd._lib import XP_E_ARG, XP_E_INTERP, XP_E_NO_TABLES, XP_E_NOT_INIT
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEV, NCOL = 12, 40


@pytest.fixture(scope='module')
def lib():
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return L.init(0)


def _view(a, dtype=None):
    nlev, ncol = a.shape
    return L.View(a.ctypes.data, L.XP_F64 if dtype is None else dtype, L.XP_MEM_HOST, nlev, ncol, ncol, 1)


def _opts(**kw):
    o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST['exact'], L.XP_F64, L.HUMIDITY['dewpoint'], 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _scalars(ncol, fill):
    """host CAPE / CIN / LFC-index outputs, filled with a sentinel"""
    arrs = {'cape': np.full(ncol, fill), 'cin': np.full(ncol, fill), 'lfc_index': np.full(ncol, -7, dtype=np.int32)}
    so = L.ScalarsOut()
    so.dtype, so.mem = L.XP_F64, L.XP_MEM_HOST
    for k, a in arrs.items():
        setattr(so, k, a.ctypes.data)
    return so, arrs


def _columns():
    return synth.columns(nlev=NLEV, ncol=NCOL, seed=3, dtype=np.float64)


def _expect(lib, rc, code, *words):
    msg = lib.xp_last_error().decode()
    assert rc == code, (rc, code, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_cape_cin_argument_errors(lib):
    p, t, td = _columns()
    vp, vt, vtd = _view(p), _view(t), _view(td)
    pc = L.Parcel(L.PARCEL['surface'], 0, 0.0, None, None, None)
    so, _ = _scalars(NCOL, np.nan)

    def call(p_=vp, t_=vt, td_=vtd, parcel=pc, o=None):
        return lib.xp_cape_cin(C.byref(p_) if p_ is not None else None, C.byref(t_), C.byref(td_), C.byref(parcel),
                               C.byref(o if o is not None else _opts()), C.byref(so), None, None)

    _expect(lib, call(p_=None), XP_E_ARG, 'pressure', 'null view')
    narrow = np.ascontiguousarray(t[:, :-1])
    _expect(lib, call(t_=_view(narrow)), XP_E_ARG, 'pressure/temperature')
    _expect(lib, call(td_=L.View(td.ctypes.data, 7, L.XP_MEM_HOST, NLEV, NCOL, NCOL, 1)), XP_E_ARG, 'dewpoint', 'dtype')
    _expect(lib, call(td_=_view(td.astype(np.float32), L.XP_F32)), XP_E_ARG, 'pressure/dewpoint')
    _expect(lib, call(parcel=L.Parcel(9, 0, 0.0, None, None, None)), XP_E_ARG, 'parcel')
    _expect(lib, call(parcel=L.Parcel(L.PARCEL['explicit'], 0, 0.0, None, None, None)), XP_E_ARG, 'explicit parcel')
    _expect(lib, call(o=_opts(lcl_interp=5)), XP_E_INTERP, 'linear or log')
    _expect(lib, call(o=_opts(moist_mode=9)), XP_E_ARG, 'moist_mode')
    _expect(lib, call(o=_opts(humidity=4)), XP_E_ARG, 'humidity')
    assert call() == 0, lib.xp_last_error()


def test_component_and_primitive_argument_errors(lib):
    p, t, td = _columns()
    vp, vt, vtd = _view(p), _view(t), _view(td)
    row = np.zeros(NCOL)
    out = np.zeros_like(p)
    narrow = _view(np.ascontiguousarray(t[:, :-1]))
    _expect(lib, lib.xp_wet_bulb_temperature(C.byref(vp), C.byref(narrow), C.byref(vtd), C.c_int32(0),
                                             C.c_void_p(out.ctypes.data), None), XP_E_ARG, 'pressure/temperature')
    _expect(lib, lib.xp_mixed_layer(None, C.byref(vt), C.c_double(100.0), C.c_void_p(row.ctypes.data), None),
            XP_E_ARG, 'pressure', 'null view')
    _expect(lib, lib.xp_lcl(C.c_int64(NCOL), C.c_int32(5), C.c_int32(L.XP_MEM_HOST), C.c_void_p(row.ctypes.data),
                            C.c_void_p(row.ctypes.data), C.c_void_p(row.ctypes.data), None, None, None, None, None),
            XP_E_ARG, 'dtype')
    _expect(lib, lib.xp_trapz(C.byref(vt), C.byref(narrow), None, C.c_int32(0), C.c_int32(0),
                              C.c_void_p(row.ctypes.data), None), XP_E_ARG, 'dat/x')
    _expect(lib, lib.xp_significant_hail_parameter(C.c_int64(NCOL), C.c_int32(3), C.c_int32(L.XP_MEM_HOST),
                                                   *[C.c_void_p(row.ctypes.data)] * 7, None), XP_E_ARG, 'dtype')
    # xp_interp_levels serves 1..4 variables and 1..4 target coordinates
    at = (C.c_double * 1)(500.0)
    for nvar, ntarget in ((0, 1), (5, 1), (1, 0), (1, 5)):
        vs = (C.POINTER(L.View) * 5)(*([C.pointer(vt)] * 5))
        outs = (C.c_void_p * 20)(*([row.ctypes.data] * 20))
        _expect(lib, lib.xp_interp_levels(C.byref(vp), C.c_int32(nvar), vs, C.c_int32(ntarget), at, C.c_int32(1), outs, None),
                XP_E_ARG, '1..4')
    vs = (C.POINTER(L.View) * 1)(C.pointer(narrow))
    _expect(lib, lib.xp_interp_levels(C.byref(vp), C.c_int32(1), vs, C.c_int32(1), at, C.c_int32(1),
                                      (C.c_void_p * 1)(row.ctypes.data), None), XP_E_ARG, 'coords/variable')
    # xp_conv_properties: the wind views must agree among themselves
    q = np.full_like(p, 0.005)
    z = np.cumsum(np.full_like(p, 500.0), axis=0)
    views = [vp, vt, _view(q), _view(z), vt, narrow, _view(z)]
    ci = L.ConvIn(*[C.pointer(v) for v in views], row.ctypes.data, row.ctypes.data)
    co = L.ConvOut()
    _expect(lib, lib.xp_conv_properties(C.byref(ci), None, C.c_int32(0), C.byref(co), None), XP_E_ARG, 'wind_u/wind_v')


def test_multi_checks_every_parcel_before_running_any(lib):
    """A bad parcels[1] must be reported before parcels[0] has produced anything: parcel 0's host outputs keep their
    sentinel."""
    p, t, td = _columns()
    vp, vt, vtd = _view(p), _view(t), _view(td)
    sos = (L.ScalarsOut * 2)()
    arrs = []
    for i in range(2):
        so, a = _scalars(NCOL, -12345.0)
        sos[i] = so
        arrs.append(a)
    for moist in ('exact', 'family'):
        for bad in (L.Parcel(9, 0, 0.0, None, None, None), L.Parcel(L.PARCEL['explicit'], 0, 0.0, None, None, None)):
            pcs = (L.Parcel * 2)(L.Parcel(L.PARCEL['surface'], 0, 0.0, None, None, None), bad)
            rc = lib.xp_cape_cin_multi(C.byref(vp), C.byref(vt), C.byref(vtd), C.c_int32(2), pcs,
                                       C.byref(_opts(moist_mode=L.MOIST[moist])), sos, None, None)
            _expect(lib, rc, XP_E_ARG, 'parcel')
            for a in arrs:
                assert (a['cape'] == -12345.0).all() and (a['cin'] == -12345.0).all() and (a['lfc_index'] == -7).all(), moist
    # and a valid pair writes both
    pcs = (L.Parcel * 2)(L.Parcel(L.PARCEL['surface'], 0, 0.0, None, None, None),
                         L.Parcel(L.PARCEL['most_unstable'], 0, 300.0, None, None, None))
    L.check(lib.xp_cape_cin_multi(C.byref(vp), C.byref(vt), C.byref(vtd), C.c_int32(2), pcs, C.byref(_opts()), sos, None, None))
    for a in arrs:
        assert not (a['cape'] == -12345.0).any() and not (a['lfc_index'] == -7).any()


def test_init_and_table_errors_in_a_fresh_process():
    """XP_E_NOT_INIT comes before any argument error, and table mode without tables is XP_E_NO_TABLES in the CAPE entry
    point and in the component ones -- in a process where nothing has initialised the library or loaded tables."""
    code = r'''
import ctypes as C
import numpy as np
from xarray_parcel_amd import _lib as L, synth
lib = L.load()
print('NOT_INIT', lib.xp_cape_cin(None, None, None, None, None, None, None, None),
      lib.xp_cape_cin_multi(None, None, None, C.c_int32(0), None, None, None, None, None),
      lib.xp_trapz(None, None, None, C.c_int32(1), C.c_int32(1), None, None))
L.check(lib.xp_init(0))
p, t, td = synth.columns(nlev=8, ncol=4, seed=1, dtype=np.float64)
v = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 8, 4, 4, 1) for a in (p, t, td)]
row, grid = np.zeros(4), np.zeros((8, 4))
so = L.ScalarsOut(); so.dtype, so.mem = L.XP_F64, L.XP_MEM_HOST; so.cape = row.ctypes.data
o = L.Opts(1, 1, 1, 0, L.MOIST['table'], L.XP_F64, 0, 0)
pc = L.Parcel(0, 0, 0.0, None, None, None)
print('NO_TABLES', lib.xp_cape_cin(C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(pc), C.byref(o), C.byref(so), None, None),
      lib.xp_moist_lapse(C.byref(v[0]), C.c_void_p(row.ctypes.data), C.c_void_p(row.ctypes.data), C.c_int32(1),
                         C.c_void_p(grid.ctypes.data), None),
      lib.xp_parcel_profile(C.byref(v[0]), C.c_void_p(row.ctypes.data), C.c_void_p(row.ctypes.data), C.c_void_p(row.ctypes.data),
                            C.c_int32(1), C.c_void_p(grid.ctypes.data), None, None, None, None, None),
      lib.xp_wet_bulb_temperature(C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.c_int32(1), C.c_void_p(grid.ctypes.data), None))
print('MESSAGE', lib.xp_last_error().decode())
'''
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln.strip()}
    assert lines['NOT_INIT'] == [str(XP_E_NOT_INIT)] * 3, out.stdout
    assert lines['NO_TABLES'] == [str(XP_E_NO_TABLES)] * 4, out.stdout
    assert 'load_moist_adiabat_lookups' in out.stdout, out.stdout
