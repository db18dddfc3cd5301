"""xp_scalars_out and xp_profile_out as include/xparcel.h describes them: a dtype and a mem of their own, the profile's own
nlev_out and strides, every pointer nullable -- through the raw ctypes ABI, since numpy_api always passes the views' dtype
and mem, nlev + 1 dense rows and one `want` set for every parcel.  The cases are tests/output_struct_cases.py's.

Expected values.  R64 is numpy_api.cape_cin_columns on the float64 grid with everything wanted and the profile included:
the dense same-dtype call the rest of the suite holds to the oracle.  Arithmetic is fp64 and the grids are exact in float32,
so for either view dtype an fp64 output equals R64 bit for bit (NaNs in the same places), an fp32 output equals
R64.astype(float32) bit for bit, and the int32 outputs are equal.  The lifted index is compared with numpy_api's answer to
the SAME request (the same `want`, the same rows) on the float64 grid: the kernel that derives the parcel temperature only at
the two nodes around the level and the one that derives it at every node agree to 1e-9 K, not to the bit
(tests/test_gpu_layered.py::test_profile_and_lifted_index), and the request decides which of them runs.

Every buffer a call is given lies inside guard bands (output_struct_cases.Guarded): after the call every byte outside its
logical elements must still hold the pattern, and the buffer of a pointer left NULL every byte.  Host outputs are read
before the test synchronises anything."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import layered_soundings as ls
from tests import output_struct_cases as oc
from tests import test_gpu_layered as TL
from tests.test_gpu_layered import _oracle_family_table, oracle_tables  # noqa: F401  (module fixtures: the oracle's tables on both sides)
from tests.test_gpu_parity import _compare
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa

pytestmark = pytest.mark.gpu
XP = {'f32': L.XP_F32, 'f64': L.XP_F64}
MEM = {'host': L.XP_MEM_HOST, 'device': L.XP_MEM_DEVICE}
CODES = {'XP_E_ARG': L.XP_E_ARG}


def ids(cases):
    return [c['id'] for c in cases]


def stage(a, mem):
    """A contiguous copy of `a` in host or device memory."""
    if mem == 'host':
        return np.array(a, copy=True, order='C')
    import torch
    return torch.as_tensor(np.array(a, copy=True, order='C')).cuda()


def addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def sync():
    import torch
    torch.cuda.synchronize()


def depth_of(pc):
    name, depth = (pc, None) if isinstance(pc, str) else pc
    return name, float(depth if depth is not None else 300.0 if name == 'most_unstable' else 100.0)


def expect(ref, dtype):
    """R64's array as an output of `dtype` holds it: rounded once (int32 as it is)."""
    ref = np.asarray(ref)
    return ref if ref.dtype == np.int32 else ref.astype(np.float64).astype(dtype)


def same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'):
        bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
        raise AssertionError((tag, 'differs at', bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], len(bad)))


# ---- R64 -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def r64(grid, parcel, depth, moist, opt):
    p, t, td = oc.grid(grid)
    kw = dict(ls.OPTION_SETS[opt])
    if parcel == 'explicit':
        kw['parcel_values'] = oc.explicit_parcel(grid)
    # (the one persistent-launch grid is used by a CAPE/CIN-only case: 340 MB of profile rows are not asked for)
    out = xa.cape_cin_columns(p, t, td, parcel=parcel, depth=depth, moist=moist, want_profile=grid != 'persistent', **kw)
    assert set(out) - {'profile'} == set(oc.ALL_SCALARS) and all(np.asarray(v).dtype != np.float32 for v in out.values() if not isinstance(v, dict))
    return out


@functools.lru_cache(maxsize=None)
def r64_lifted_index(grid, parcel, depth, moist, opt, want, rows):
    """The lifted index of the same request on the float64 grid."""
    p, t, td = oc.grid(grid)
    kw = dict(ls.OPTION_SETS[opt])
    if parcel == 'explicit':
        kw['parcel_values'] = oc.explicit_parcel(grid)
    return xa.cape_cin_columns(p, t, td, parcel=parcel, depth=depth, moist=moist, want=want, want_profile=rows or False,
                               lifted_index_at=oc.LIFTED_INDEX_AT, **kw)['lifted_index']


# ---- the caller's buffers ----------------------------------------------------------------------------------------------------------
class ScalarBufs:
    """One guarded buffer per field of xp_scalars_out, wanted or not; only the wanted ones get their pointer."""

    def __init__(self, ncol, spec):
        self.spec, self.mem, self.want = spec, spec['mem'], tuple(spec['want'])
        self.dtype = oc.DTYPES[spec['dtype']]
        self.buf = {k: oc.Guarded.row(ncol, np.int32 if k in oc.SCALAR_I else self.dtype, self.mem) for k in oc.ALL_SCALARS}

    def struct(self, **over):
        so = L.ScalarsOut(dtype=over.get('dtype', XP[self.spec['dtype']]), mem=over.get('mem', MEM[self.mem]))
        for k in self.want:
            setattr(so, k, self.buf[k].ptr)
        return so

    def buffers(self):
        return list(self.buf.values())

    def read(self):
        return {k: self.buf[k].read()[0] for k in self.want}

    def check(self, ref, tag, skip=()):
        for k, g in self.buf.items():
            if k not in self.want:
                assert g.pristine(), (tag, k, 'the buffer of a NULL pointer was written')
                continue
            assert g.untouched(), (tag, k, 'written outside the logical elements')
            if k not in skip:
                same(g.read()[0], expect(np.asarray(ref[k]).reshape(-1), g.dtype), (tag, k))


class ProfileBufs:
    """The six arrays and the lifted index of xp_profile_out, each guarded, in the case's layout."""

    def __init__(self, nlev, ncol, spec):
        self.spec, self.mem, self.vars, self.nlev, self.ncol = spec, spec['mem'], tuple(spec['vars']), nlev, ncol
        self.dtype = oc.DTYPES[spec['dtype']]
        self.nlev_out = nlev + 1 + spec['extra']
        self.ls, self.cs = oc.layout_strides(spec['layout'], self.nlev_out, ncol)
        rows = max(self.nlev_out, 1)
        self.buf = {k: oc.Guarded(rows, ncol, self.dtype, self.ls, self.cs, self.mem) for k in oc.PROFILE_VARS}
        self.li = oc.Guarded.row(ncol, self.dtype, self.mem)

    def struct(self, **over):
        po = L.ProfileOut(dtype=over.get('dtype', XP[self.spec['dtype']]), mem=over.get('mem', MEM[self.mem]), nlev_out=self.nlev_out,
                          lev_stride=over.get('lev_stride', self.ls), col_stride=over.get('col_stride', self.cs))
        for k in self.vars:
            setattr(po, k, self.buf[k].ptr)
        if self.spec['lifted_index']:
            po.lifted_index, po.lifted_index_pressure = self.li.ptr, over.get('lifted_index_pressure', oc.LIFTED_INDEX_AT)
        return po

    def buffers(self):
        return list(self.buf.values()) + [self.li]

    def check(self, ref_profile, ref_li, tag):
        for k, g in self.buf.items():
            if k not in self.vars:
                assert g.pristine(), (tag, 'profile', k, 'the buffer of a NULL pointer was written')
                continue
            assert g.untouched(), (tag, 'profile', k, 'written outside the logical elements')
            want = np.full((self.nlev_out, self.ncol), np.nan)           # rows beyond nlev + 1: all NaN
            want[:self.nlev + 1] = np.asarray(ref_profile[k]).reshape(self.nlev + 1, self.ncol)
            same(g.read(), want.astype(self.dtype), (tag, 'profile', k))
        if not self.spec['lifted_index']:
            assert self.li.pristine(), (tag, 'lifted_index', 'the buffer of a NULL pointer was written')
        else:
            assert self.li.untouched(), (tag, 'lifted_index', 'written outside the logical elements')
            same(self.li.read()[0], expect(np.asarray(ref_li).reshape(-1), self.dtype), (tag, 'lifted_index'))


class Call:
    """One case of CAPE_CASES / MULTI_CASES ... staged and run; the inputs stay alive with it."""

    def __init__(self, case, scalars=None):
        self.case = case
        vd, vm = case['view_dtype'], case['view_mem']
        p, t, td = oc.grid(case['grid'], vd)
        self.nlev, self.ncol = p.shape
        self.keep = [stage(a, vm) for a in (p, t, td)]
        self.views = [L.View(addr(a), XP[vd], MEM[vm], self.nlev, self.ncol, self.ncol, 1) for a in self.keep]
        self.parcels = [depth_of(pc) for pc in case['parcels']]
        n = len(self.parcels)
        self.pcs = (L.Parcel * n)()
        for i, (name, depth) in enumerate(self.parcels):
            self.pcs[i] = L.Parcel(L.PARCEL[name], 0, depth, None, None, None)
            if name == 'explicit':
                ex = [stage(a, vm) for a in oc.explicit_parcel(case['grid'], vd)]
                self.keep += ex
                self.pcs[i].pressure, self.pcs[i].temperature, self.pcs[i].dewpoint = (addr(a) for a in ex)
        self.opts = xa._opts(moist=case['moist'], compute={'f32': 'float32', 'f64': 'float64'}[case['compute']], **ls.OPTION_SETS[case['opt']])
        self.opts.flags = L.OPT_FUSE_PARCELS if case['fused'] else 0
        self.S = [ScalarBufs(self.ncol, s) for s in (scalars or case['scalars'])]
        self.P = [ProfileBufs(self.nlev, self.ncol, pr) if pr is not None else None for pr in case['profiles']]

    def run(self, lib, scalars_over=None, profile_over=None):
        n = len(self.parcels)
        sos = (L.ScalarsOut * n)(*[s.struct(**(scalars_over or {})) for s in self.S])
        pos = (L.ProfileOut * n)(*[pr.struct(**(profile_over or {})) for pr in self.P]) if all(pr is not None for pr in self.P) else None
        v = [C.byref(x) for x in self.views]
        if self.case['entry'] == 'xp_cape_cin':
            return lib.xp_cape_cin(v[0], v[1], v[2], C.byref(self.pcs[0]), C.byref(self.opts), C.byref(sos[0]),
                                   C.byref(pos[0]) if pos is not None else None, None)
        return lib.xp_cape_cin_multi(v[0], v[1], v[2], n, self.pcs, C.byref(self.opts), sos, pos, None)

    def reference(self, i):
        name, depth = self.parcels[i]
        c = self.case
        ref = r64(c['grid'], name, depth, c['moist'], c['opt'])
        pr, li = self.P[i], None
        if pr is not None and pr.spec['lifted_index']:
            li = r64_lifted_index(c['grid'], name, depth, c['moist'], c['opt'], self.S[i].want, pr.vars)
        return ref, li

    def check(self, skip=()):
        """Host buffers first, before anything is synchronised: Stager::finish has done that when any buffer is host memory."""
        for mem in ('host', 'device'):
            if mem == 'device':
                sync()
            for i in range(len(self.parcels)):
                ref, li = self.reference(i)
                tag = (self.case['id'], 'parcel %d' % i)
                if self.S[i].mem == mem:
                    self.S[i].check(ref, tag, skip)
                if self.P[i] is not None and self.P[i].mem == mem:
                    self.P[i].check(ref['profile'], li, tag)

    def all_pristine(self):
        sync()
        return all(g.pristine() for x in self.S + [pr for pr in self.P if pr is not None] for g in x.buffers())


def run_and_check(case):
    lib = L.init(0)
    call = Call(case)
    rc = call.run(lib)
    assert rc == L.XP_OK, (case['id'], rc, lib.xp_last_error())
    call.check()
    return call


# ---- xp_cape_cin: the all-outputs and the CAPE/CIN-only kernels, the profile, the memory spaces --------------------------------------
NOT_TABLE = [c for c in oc.CAPE_CASES if c['moist'] != 'table']
TABLE = [c for c in oc.CAPE_CASES if c['moist'] == 'table']


@pytest.mark.parametrize('case', NOT_TABLE, ids=ids(NOT_TABLE))
def test_cape_cin_output_structs(case):
    run_and_check(case)


@pytest.mark.parametrize('case', TABLE, ids=ids(TABLE))
def test_cape_cin_output_structs_in_table_mode(case, oracle_tables):
    run_and_check(case)


@pytest.mark.parametrize('case', oc.MULTI_CASES, ids=ids(oc.MULTI_CASES))
def test_cape_cin_multi_output_structs_per_parcel(case):
    """Each parcel's own dtype, mem and `want`, fused and one pass per parcel: each parcel's outputs equal its R64."""
    call = run_and_check(case)
    if not any(call.P):                                                # and the multi call's own answer on the float64 grid
        p, t, td = oc.grid(case['grid'])
        multi = xa.cape_cin_multi(p, t, td, list(case['parcels']), moist=case['moist'], fused=case['fused'])
        for s, m in zip(call.S, multi):
            s.check(m, (case['id'], 'against cape_cin_multi'))


# ---- xp_opts.compute = XP_F32 with fp64 scalars ----------------------------------------------------------------------------------------
PROLOGUE = ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature', 'parcel_index', 'parcel_pressure', 'parcel_temperature',
            'parcel_dewpoint')


@pytest.mark.parametrize('case', oc.COMPUTE32_CASES, ids=ids(oc.COMPUTE32_CASES))
def test_compute32_with_fp64_scalars(case):
    """Accepted; rounded to float32 it is the same call with f32 scalars (same grid, same column order, so the same wavefront
    neighbours); the prologue's outputs are R64's bit for bit; cape / cin lie within the header's 0.5 J/kg of R64."""
    lib = L.init(0)
    wide = Call(case)
    rc = wide.run(lib)
    assert rc == L.XP_OK, (case['id'], rc, lib.xp_last_error())
    walk = ('cape', 'cin', 'lfc_pressure', 'el_pressure')
    wide.check(skip=walk)                                              # guards, NULL pointers, and the prologue against R64
    assert set(PROLOGUE) <= set(wide.S[0].want)
    narrow = Call(case, scalars=(dict(case['scalars'][0], dtype='f32'),))
    assert narrow.run(lib) == L.XP_OK, lib.xp_last_error()
    narrow.check(skip=walk)
    got64, got32 = wide.S[0].read(), narrow.S[0].read()
    for k in wide.S[0].want:
        assert got64[k].dtype == (np.int32 if k in oc.SCALAR_I else np.float64)
        same(got64[k].astype(got32[k].dtype), got32[k], (case['id'], k, 'f64 scalars rounded against f32 scalars'))
    ref = r64(case['grid'], 'surface', 100.0, 'family', 0)
    for k in walk:
        a, b = got64[k], np.asarray(ref[k])
        assert np.array_equal(np.isnan(a), np.isnan(b)), (case['id'], k)
    for k in ('cape', 'cin'):
        err = np.abs(got64[k] - np.asarray(ref[k]))
        print('%s %s: worst difference from R64 %.3g J/kg' % (case['id'], k, np.nanmax(err)))
        assert np.nanmax(err) <= 0.5, (case['id'], k, float(np.nanmax(err)))


# ---- one fp32 grid with fp64 outputs against the C oracle, at the fp64 tolerance -------------------------------------------------------
@pytest.mark.parametrize('case', oc.ORACLE_CASES, ids=ids(oc.ORACLE_CASES))
def test_f32_grid_with_f64_outputs_vs_oracle(case):
    """With fp64 outputs an fp32 grid is held to the oracle at 1e-6 / 1e-7, not at the 2e-7-relative rule that output
    rounding forces on _compare; the tie caps are the float64 run's, to which this result is bit-equal."""
    call = run_and_check(case)
    got = call.S[0].read()
    assert all(got[k].dtype == np.float64 for k in oc.SCALAR_F + oc.SCALAR_P)
    _compare(got, TL.reference(case['grid'], case['parcels'][0], 0, 'family'), np.float64, 1e-6)


# ---- xp_lfc_el, xp_select_parcel, xp_rebase_profile --------------------------------------------------------------------------------
LFC_EL_WANT = ('lfc_pressure', 'lfc_temperature', 'el_pressure', 'el_temperature', 'lfc_index', 'el_index', 'status')


def _through_f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _scalars_entry(entry, vd, vm, od, om, parcel):
    """One call; returns (ScalarBufs, the other outputs as host arrays, every Guarded)."""
    lib = L.init(0)
    dt = oc.DTYPES[vd]
    if entry == 'xp_lfc_el':
        # the profile R64 wrote, as numbers both dtypes hold
        ref = r64('R', 'surface', 100.0, 'exact', 0)
        rows = [_through_f32(ref['profile'][k]) for k in ('pressure', 'temperature', 'environment_temperature')]
        lcl = [_through_f32(ref[k]) for k in ('lcl_pressure', 'lcl_temperature')]
        nrow, ncol = rows[0].shape
        keep = [stage(a.astype(dt), vm) for a in rows + lcl]
        views = [L.View(addr(a), XP[vd], MEM[vm], nrow, ncol, ncol, 1) for a in keep[:3]]
        S = ScalarBufs(ncol, dict(dtype=od, mem=om, want=LFC_EL_WANT))
        rc = lib.xp_lfc_el(views[0], views[1], views[2], addr(keep[3]), addr(keep[4]), S.struct(), None)
        assert rc == L.XP_OK, (entry, rc, lib.xp_last_error())
        return S, {}, S.buffers()
    p, t, td = oc.grid('R', vd)
    nlev, ncol = p.shape
    keep = [stage(a, vm) for a in (p, t, td)]
    views = [L.View(addr(a), XP[vd], MEM[vm], nlev, ncol, ncol, 1) for a in keep]
    name, depth = depth_of(parcel)
    pc = L.Parcel(L.PARCEL[name], 0, depth, None, None, None)
    S = ScalarBufs(ncol, dict(dtype=od, mem=om, want=oc.PARCEL_ONLY))
    if entry == 'xp_select_parcel':
        rc = lib.xp_select_parcel(views[0], views[1], views[2], pc, S.struct(), None)
        assert rc == L.XP_OK, (entry, rc, lib.xp_last_error())
        return S, {}, S.buffers()
    rows = nlev + (1 if name == 'mixed_layer' else 0)
    outs = [oc.Guarded(rows, ncol, dt, ncol, 1, vm) for _ in range(3)]   # the re-based profile: the views' dtype and mem
    kept = np.full(nlev, -7, dtype=np.int32)
    n_out = C.c_int64(-1)
    rc = lib.xp_rebase_profile(views[0], views[1], views[2], pc, outs[0].ptr, outs[1].ptr, outs[2].ptr, S.struct(), kept.ctypes.data,
                               C.byref(n_out), None)
    assert rc == L.XP_OK, (entry, rc, lib.xp_last_error())
    host = {} if S.mem == 'device' else {k: S.buf[k].read()[0].copy() for k in S.want}       # complete before any synchronisation
    sync()
    for k, v in host.items():
        assert np.array_equal(v, S.buf[k].read()[0], equal_nan=True), (entry, k, 'host output incomplete when the call returned')
    other = {'level_kept': kept, 'nlev_out': np.array([n_out.value]), 'pressure': outs[0].read(), 'temperature': outs[1].read(),
             'dewpoint': outs[2].read()}
    return S, other, S.buffers() + outs


SCALARS_ENTRY_RUNS = [(c, pc) for c in oc.SCALARS_ENTRY_CASES                    # xp_lfc_el takes no parcel: one run
                      for pc in (('most_unstable', 'mixed_layer') if c['entry'] != 'xp_lfc_el' else ('none',))]


@pytest.mark.parametrize('case,parcel', SCALARS_ENTRY_RUNS, ids=['%s-%s' % (c['id'], pc) for c, pc in SCALARS_ENTRY_RUNS])
def test_other_entry_points_with_a_scalars_out(case, parcel):
    """dtype- and mem-crossed calls against the same-dtype call (float64 views, float64 outputs, all on the device; the inputs
    are exact in float32): an output of the other dtype is that call's, rounded once; the re-based profile does not depend
    on parcel_out's dtype or mem."""
    entry = case['entry']
    S, other, bufs = _scalars_entry(entry, case['view_dtype'], case['view_mem'], case['out_dtype'], case['out_mem'], parcel)
    host = {k: S.buf[k].read()[0].copy() for k in S.want} if S.mem == 'host' else None
    R, rother, _ = _scalars_entry(entry, 'f64', 'device', 'f64', 'device', parcel)
    sync()
    ref = R.read()
    assert any(np.isfinite(ref[k].astype(np.float64)).any() for k in R.want if k not in oc.SCALAR_I), 'the reference call wrote nothing'
    S.check(ref, (case['id'], parcel))
    if host is not None:
        for k, v in host.items():
            assert np.array_equal(v, S.buf[k].read()[0], equal_nan=True), (case['id'], k, 'host output incomplete when the call returned')
    assert all(g.untouched() for g in bufs), case['id']
    for k, v in other.items():
        same(v, expect(rother[k], v.dtype) if v.dtype.kind == 'f' else rother[k], (case['id'], parcel, k))


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rid,wrong,code,word', oc.REJECTIONS, ids=[r[0] for r in oc.REJECTIONS])
@pytest.mark.parametrize('entry', ['xp_cape_cin', 'xp_cape_cin_multi'])
def test_rejections_leave_every_buffer_untouched(entry, rid, wrong, code, word):
    lib = L.init(0)
    prof = dict(dtype='f64', mem=wrong['profile_mem'] if isinstance(wrong.get('profile_mem'), str) else 'device',
                layout=wrong.get('layout', 'dense'), extra=wrong.get('extra', 0), vars=oc.PROFILE_VARS, lifted_index=True)
    n = 1 if entry == 'xp_cape_cin' else 2
    case = dict(id=rid, entry=entry, grid='R2', moist='exact', parcels=('surface', 'most_unstable')[:n], opt=0, compute='f64',
                view_dtype='f64', view_mem='device', scalars=(dict(dtype='f64', mem='device', want=oc.ALL_SCALARS),) * n,
                profiles=(prof,) * n, fused=False)
    call = Call(case)
    so, po = {}, {}
    if 'scalars_dtype' in wrong:
        so['dtype'] = wrong['scalars_dtype']
    if 'scalars_mem' in wrong:
        so['mem'] = wrong['scalars_mem']
    if 'profile_dtype' in wrong:
        po['dtype'] = wrong['profile_dtype']
    if isinstance(wrong.get('profile_mem'), int):
        po['mem'] = wrong['profile_mem']
    for k in ('lev_stride', 'col_stride', 'lifted_index_pressure'):
        if k in wrong:
            po[k] = wrong[k]
    rc = call.run(lib, so, po)
    msg = lib.xp_last_error().decode()
    assert rc == CODES[code] and word in msg, (rid, rc, msg)
    assert call.all_pristine(), (rid, 'a rejected call wrote to a buffer')
    if so or po:                                                       # the same call without the mistake runs
        assert call.run(lib) == L.XP_OK, (rid, lib.xp_last_error())
        call.check()


# ---- the entry points whose out struct must match the views --------------------------------------------------------------------------
def _check_out_call(lib, entry, out_dtype, out_mem):
    """A small valid host float64 call of `entry` whose out struct says (out_dtype, out_mem); every output pointer is given
    and guarded.  Returns (rc, buffers)."""
    p, t, td = (np.array(a[:, :8]) for a in oc.grid('R'))
    nlev, ncol = p.shape
    z = np.ascontiguousarray(29.27 * 260.0 * np.log(p[0] / p))
    u = np.ascontiguousarray(5.0 + 0.01 * z)
    v = np.ascontiguousarray(2.0 - 0.005 * z)
    row = np.ascontiguousarray(p[3])
    view = lambda a: L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, nlev, ncol, ncol, 1)
    P, T, TD, Z, U, V = (view(a) for a in (p, t, td, z, u, v))
    dt = np.float32 if out_dtype == L.XP_F32 else np.float64
    mem = 'device' if out_mem == L.XP_MEM_DEVICE else 'host'
    bufs = []

    def g(rows=1, int32=False):
        bufs.append(oc.Guarded(rows, ncol, np.int32 if int32 else dt, ncol, 1, mem))
        return bufs[-1].ptr

    def four():
        return (C.c_void_p * 4)(*[g() for _ in range(4)])
    head = dict(dtype=out_dtype, mem=out_mem, status=g(int32=True))
    one = (C.c_void_p * 1)(row.ctypes.data)
    layer = (L.WindLayer * 1)(L.WindLayer(L.LAYER_PRESSURE, 0, float('nan'), 500.0))
    pc = L.Parcel(L.PARCEL['surface'], 0, 0.0, None, None, None)
    if entry == 'xp_downdraft_cape':
        o = L.DcapeOut(dcape=g(), start_pressure=g(), start_temperature=g(), parcel_temperature=g(nlev), **head)
        rc = lib.xp_downdraft_cape(P, T, TD, 700.0, 200.0, L.MOIST['exact'], o, None)
    elif entry == 'xp_effective_inflow_layer':
        o = L.EffectiveLayerOut(base_pressure=g(), top_pressure=g(), base_height=g(), top_height=g(), base_index=g(int32=True),
                                top_index=g(int32=True), candidate_cape=g(nlev), candidate_cin=g(nlev), **head)
        rc = lib.xp_effective_inflow_layer(P, T, TD, Z, 100.0, -250.0, 300.0, None, o, None)
    elif entry == 'xp_cape_cin_layers':
        o = L.CapeLayersOut(cape=four(), cin=four(), total_cape=g(), total_cin=g(), lfc_pressure=g(), el_pressure=g(), lcl_pressure=g(), **head)
        rc = lib.xp_cape_cin_layers(P, T, TD, pc, None, 1, None, one, o, None)
    elif entry == 'xp_bunkers_storm_motion':
        o = L.StormMotionOut(right_u=g(), right_v=g(), left_u=g(), left_v=g(), mean_u=g(), mean_v=g(), **head)
        rc = lib.xp_bunkers_storm_motion(P, U, V, Z, o, None)
    elif entry == 'xp_storm_relative_helicity':
        o = L.SrhOut(positive=four(), negative=four(), total=four(), **head)
        rc = lib.xp_storm_relative_helicity(Z, U, V, None, None, None, None, 0.0, 1, (C.c_double * 1)(1000.0), o, None)
    elif entry == 'xp_storm_relative_helicity_layers':
        o = L.SrhLayersOut(positive=four(), negative=four(), total=four(), shear_u=four(), shear_v=four(), **head)
        bottom = np.zeros(ncol)
        top = np.full(ncol, 1000.0)
        rc = lib.xp_storm_relative_helicity_layers(Z, U, V, None, None, None, None, bottom.ctypes.data, 1,
                                                   (C.c_void_p * 1)(top.ctypes.data), o, None)
    elif entry == 'xp_wind_layers':
        o = L.WindLayersOut(**{k: four() for k in L.WIND_LAYERS_OUT}, **head)
        rc = lib.xp_wind_layers(P, U, V, Z, 1, layer, o, None)
    elif entry == 'xp_thermo_layers':
        o = L.ThermoLayersOut(**{k: four() for k in L.THERMO_LAYERS_OUT}, **head)
        rc = lib.xp_thermo_layers(P, T, TD, Z, 1, layer, None, None, o, None)
    elif entry == 'xp_sounding_indices':
        o = L.SoundingOut(**{k: g() for k in L.SOUNDING_OUT}, **head)
        rc = lib.xp_sounding_indices(P, T, TD, U, V, None, o, None)
    elif entry == 'xp_isentropic_interpolation':
        o = L.IsentropicOut(pressure=g(2), temperature=g(2), **head)
        rc = lib.xp_isentropic_interpolation(P, T, 0, None, 2, (C.c_double * 2)(300.0, 320.0), None, o, None)
    elif entry == 'xp_hydrostatic_height':
        o = L.HydrostaticOut(height=g(nlev), thickness=(C.c_void_p * 4)(g()), **head)           # one layer: thickness[1:] stay NULL
        rc = lib.xp_hydrostatic_height(P, T, TD, None, 1, layer, None, o, None)
    elif entry == 'xp_ncape':
        o = L.NcapeOut(ncape=g(), lfc_height=g(), el_height=g(), **head)
        lfc, el = np.full(ncol, 800.0), np.full(ncol, 300.0)
        rc = lib.xp_ncape(P, T, TD, Z, lfc.ctypes.data, el.ctypes.data, o, None)
    else:
        raise KeyError(entry)
    return rc, bufs


@pytest.mark.parametrize('case', oc.CHECK_OUT_CASES, ids=ids(oc.CHECK_OUT_CASES))
def test_entry_points_that_forbid_the_crossing(case):
    """check_out: XP_E_ARG, the out struct named, nothing written -- and the same call with a matching out struct runs."""
    lib = L.init(0)
    crossed = (L.XP_F32, L.XP_MEM_HOST) if case['crossed'] == 'dtype' else (L.XP_F64, L.XP_MEM_DEVICE)
    rc, bufs = _check_out_call(lib, case['entry'], *crossed)
    msg = lib.xp_last_error().decode()
    assert rc == L.XP_E_ARG and case['entry'] in msg and 'out' in msg and 'differ from the views' in msg, (case['id'], rc, msg)
    sync()
    assert all(b.pristine() for b in bufs), (case['id'], 'a rejected call wrote to a buffer')
    rc, bufs = _check_out_call(lib, case['entry'], L.XP_F64, L.XP_MEM_HOST)
    assert rc == L.XP_OK, (case['id'], rc, lib.xp_last_error())
    assert all(b.untouched() for b in bufs) and not all(b.pristine() for b in bufs), case['id']
