"""The output-struct contract of the CAPE entry points (TEST INFRASTRUCTURE, importable without a GPU).

include/xparcel.h gives xp_scalars_out and xp_profile_out a dtype and a mem of their own, the profile its own nlev_out and
strides, and makes every pointer nullable.  tests/test_gpu_output_structs.py drives those freedoms through the raw ctypes
ABI; this module holds what it and tests/test_output_struct_cases_cpu.py share:

  Guarded     a caller's output buffer with a guard band on either side, filled with one BYTE pattern (the outputs
              legitimately hold NaN, so no float sentinel): read() gives the logical array back, untouched() says, byte by
              byte, that nothing but the logical elements was written -- the guards and the gaps between strided elements;
  grid()      the grids, exact in float32, cached and read-only;
  *_CASES     the case tables, one dict per call, which name the kernel family and the ProfileSink branches a case is meant
              to reach, so that the GPU file and the census read one list."""
import functools
import os
import re

import numpy as np

from tests import layered_soundings as ls

PATTERN = 0xA5
GUARD = 256                                                            # bytes on either side of the span
DTYPES = {'f32': np.float32, 'f64': np.float64}
OTHER = {'f32': 'f64', 'f64': 'f32'}
MEMS = ('host', 'device')

SCALAR_F = ('cape', 'cin', 'lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature', 'lfc_pressure', 'lfc_temperature',
            'el_pressure', 'el_temperature')
SCALAR_I = ('lfc_index', 'el_index', 'status', 'parcel_index')
SCALAR_P = ('parcel_pressure', 'parcel_temperature', 'parcel_dewpoint')
ALL_SCALARS = SCALAR_F + SCALAR_I + SCALAR_P
# any of these five selects the all-outputs kernels (include/xparcel.h at xp_scalars_out)
FULL_ONLY = ('lfc_temperature', 'el_temperature', 'lfc_index', 'el_index', 'status')
LEAN = tuple(k for k in ALL_SCALARS if k not in FULL_ONLY)
PARCEL_ONLY = SCALAR_P + ('parcel_index',)
PROFILE_VARS = ('pressure', 'temperature', 'virtual_temperature', 'environment_temperature',
                'environment_virtual_temperature', 'environment_dewpoint')
LIFTED_INDEX_VARS = ('pressure', 'temperature', 'environment_temperature')      # numpy_api.LIFTED_INDEX_VARS
LIFTED_INDEX_AT = 500.0

KERNEL_FAMILIES = ('all_outputs', 'cape_cin_only', 'fused_multi', 'compute32', 'rk4_redo')
SINK_BRANCHES = ('native6', 'generic', 'blank', 'finish_padding', 'lazy_lifted_index')
LAYOUTS = ('dense', 'padded', 'column_major', 'second_column')
EXTRA_ROWS = (0, 3)                                                    # nlev_out = nlev + 1 + extra


def layout_strides(layout, nlev_out, ncol):
    """(lev_stride, col_stride) in elements."""
    return {'dense': (ncol, 1), 'padded': (ncol + 5, 1), 'column_major': (1, nlev_out), 'second_column': (2 * ncol, 2)}[layout]


class Guarded:
    """n_rows x ncol elements of `dtype`, element (j, c) at base + (j * ls + c * cs) elements, inside a byte buffer that
    covers the span plus GUARD bytes before and after it, every byte PATTERN.  mem 'host': a NumPy array; 'device': a
    torch.uint8 CUDA tensor."""

    def __init__(self, n_rows, ncol, dtype, ls=None, cs=1, mem='host', guard=GUARD):
        assert mem in MEMS and guard >= 256 and guard % 16 == 0
        self.n_rows, self.ncol, self.dtype, self.mem, self.guard = int(n_rows), int(ncol), np.dtype(dtype), mem, guard
        self.ls, self.cs = (self.ncol if ls is None else int(ls)), int(cs)
        assert self.ls >= 0 and self.cs >= 0
        self.span = ((self.n_rows - 1) * self.ls + (self.ncol - 1) * self.cs + 1) if self.n_rows and self.ncol else 0
        self.nbytes = self.span * self.dtype.itemsize + 2 * guard
        if mem == 'host':
            self.buf = np.full(self.nbytes, PATTERN, dtype=np.uint8)
            base = self.buf.ctypes.data
        else:
            import torch
            self.buf = torch.full((self.nbytes,), PATTERN, dtype=torch.uint8, device='cuda')
            base = self.buf.data_ptr()
        assert base % 8 == 0
        self.ptr = base + guard                                        # the address of element (0, 0)

    @classmethod
    def row(cls, ncol, dtype, mem='host'):
        """The one-row form: a per-column scalar output (np.int32 for the indices and the status word)."""
        return cls(1, ncol, dtype, ncol, 1, mem)

    def bytes(self):
        """The whole buffer, guards included, as host bytes (a device buffer is copied)."""
        return self.buf if self.mem == 'host' else self.buf.cpu().numpy()

    def _offsets(self):
        """Byte offset, from the start of the buffer, of every logical element: (n_rows, ncol)."""
        j, c = np.arange(self.n_rows, dtype=np.int64)[:, None], np.arange(self.ncol, dtype=np.int64)[None, :]
        return self.guard + (j * self.ls + c * self.cs) * self.dtype.itemsize

    def read(self):
        """The logical (n_rows, ncol) array, a copy."""
        b = self.bytes()
        off = self._offsets()[:, :, None] + np.arange(self.dtype.itemsize, dtype=np.int64)
        return np.ascontiguousarray(b[off]).view(self.dtype)[:, :, 0]

    def untouched(self):
        """Every byte outside the logical elements still holds PATTERN."""
        b = self.bytes()
        outside = np.ones(self.nbytes, dtype=bool)
        off = self._offsets().reshape(-1)
        for k in range(self.dtype.itemsize):
            outside[off + k] = False
        return bool(np.all(b[outside] == PATTERN))

    def pristine(self):
        """Every byte, logical elements included, still holds PATTERN: what a NULL pointer's buffer must look like."""
        return bool(np.all(self.bytes() == PATTERN))

    def written(self):
        """No logical element still holds the pattern in all of its bytes."""
        b = self.bytes()
        off = self._offsets()[:, :, None] + np.arange(self.dtype.itemsize, dtype=np.int64)
        return not bool(np.any(np.all(b[off] == PATTERN, axis=2)))


# ---- grids -------------------------------------------------------------------------------------------------------------------
PERSISTENT_SHAPE = (8, (3 << 18) + 77, 13)                             # the persistent launch of family mode (surface parcel)
NAN_SURFACE_EVERY = 9
OFF_TABLE_EVERY = 7
ONE_COLUMN = 5
GRID_NAMES = ('R', 'B', 'R1', 'R2', 'one', 'nan_surface', 'off_table', 'persistent')


def _exact(arrays, dtype):
    out = tuple(np.ascontiguousarray(a.astype(dtype)) for a in arrays)
    for a, b in zip(out, arrays):
        assert np.array_equal(a.astype(np.float64), b, equal_nan=True), 'the grid is not exact in %s' % np.dtype(dtype).name
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _grid64(name):
    if name == 'R':
        return ls.grid(*ls.GRID_REPLAY)
    if name == 'B':
        return ls.grid(*ls.GRID_B)
    if name == 'persistent':
        nlev, ncol, seed = PERSISTENT_SHAPE
        return ls.layered(nlev, ncol, seed, nan_fraction=ls.NAN_FRACTION)
    p, t, td = (a.copy() for a in ls.grid(*ls.GRID_REPLAY))
    if name in ('R1', 'R2'):
        return tuple(np.ascontiguousarray(a[:int(name[1])]) for a in (p, t, td))
    if name == 'one':
        return tuple(np.ascontiguousarray(a[:, ONE_COLUMN:ONE_COLUMN + 1]) for a in (p, t, td))
    if name == 'nan_surface':                                          # a NaN surface parcel: store_blank_column, ProfileSink::blank
        t[0, ::NAN_SURFACE_EVERY] = np.nan
        return p, t, td
    if name == 'off_table':                                            # adiabats warmer than the family table's 312 K edge: the RK4 redo
        t[:, ::OFF_TABLE_EVERY] += 22.0
        td[:, ::OFF_TABLE_EVERY] += 24.0
        td = np.minimum(td, t)
        assert all(np.array_equal(np.round(a * ls.Q), a * ls.Q, equal_nan=True) for a in (t, td)), 'no longer multiples of 1/64'
        return p, t, td
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def grid(name, dtype='f64'):
    """(p, t, td) of a named grid in 'f32' or 'f64': the same numbers in both, read-only."""
    return _exact(_grid64(name), DTYPES[dtype])


def explicit_parcel(name, dtype='f64'):
    """The explicit parcel of a grid (tests/test_gpu_layered.py's): multiples of 1/64 like the grid."""
    p, t, td = grid(name, dtype)
    return tuple(np.ascontiguousarray(a) for a in (p[0] + 5, t[0] + 1, td[0] - 1))


# ---- xp_cape_cin cases ---------------------------------------------------------------------------------------------------------
def _profile(dtype, layout='dense', extra=0, vars=PROFILE_VARS, lifted_index=False, mem=None):
    return dict(dtype=dtype, mem=mem, layout=layout, extra=extra, vars=tuple(vars), lifted_index=lifted_index)


def _cape(id, reaches, grid, moist, parcel, opt, views, scalars, want=ALL_SCALARS, profile=None, view_mem='device',
          scalars_mem=None, compute='f64'):
    """One xp_cape_cin call.  views / scalars: 'f32' | 'f64'; mems default to the views' mem."""
    sm = scalars_mem or view_mem
    prof = None
    if profile is not None:
        prof = dict(profile, mem=profile['mem'] or view_mem)
    return dict(id=id, entry='xp_cape_cin', reaches=tuple(reaches), grid=grid, moist=moist, parcels=(parcel,), opt=opt,
                compute=compute, view_dtype=views, view_mem=view_mem,
                scalars=(dict(dtype=scalars, mem=sm, want=tuple(want)),), profiles=(prof,), fused=False)


def lazy_request(case, i=0):
    """The request that takes the lazy lifted-index kernel (csrc/xp_cape_tu.hip): family mode, default options, a
    CAPE/CIN-only scalars struct, the lifted index and none of the six arrays."""
    pr = case['profiles'][i]
    return (pr is not None and pr['lifted_index'] and not pr['vars'] and case['moist'] == 'family' and case['opt'] == 0 and
            not any(k in FULL_ONLY for k in case['scalars'][i]['want']))


A, C_ = ('all_outputs',), ('cape_cin_only',)
CAPE_CASES = [
    # the all-outputs kernels: every mode, every parcel kind, option sets O0 and O4, the dtype crossed either way
    _cape('all-exact-surface-O0-f32>f64', A, 'R', 'exact', 'surface', 0, 'f32', 'f64'),
    _cape('all-exact-mu-O4-f64>f32', A, 'R', 'exact', 'most_unstable', 4, 'f64', 'f32'),
    _cape('all-exact-ml-O0-f64>f32', A, 'R', 'exact', 'mixed_layer', 0, 'f64', 'f32'),
    _cape('all-exact-explicit-O4-f32>f64', A, 'R', 'exact', 'explicit', 4, 'f32', 'f64'),
    _cape('all-family-surface-O4-f64>f32', A, 'B', 'family', 'surface', 4, 'f64', 'f32'),
    _cape('all-family-mu-O0-f32>f64', A, 'B', 'family', 'most_unstable', 0, 'f32', 'f64'),
    _cape('all-family-ml-O4-f32>f64', A, 'B', 'family', 'mixed_layer', 4, 'f32', 'f64'),
    _cape('all-family-explicit-O0-f64>f32', A, 'B', 'family', 'explicit', 0, 'f64', 'f32'),
    _cape('all-family-offtable-surface-f32>f64', A + ('rk4_redo',), 'off_table', 'family', 'surface', 0, 'f32', 'f64'),
    _cape('all-family-nansurface-f64>f32', A, 'nan_surface', 'family', 'surface', 0, 'f64', 'f32'),
    _cape('all-table-surface-O0-f32>f64', A, 'R', 'table', 'surface', 0, 'f32', 'f64'),
    _cape('all-table-mu-O4-f64>f32', A, 'R', 'table', 'most_unstable', 4, 'f64', 'f32'),
    _cape('all-exact-one-column-f32>f64', A, 'one', 'exact', 'surface', 0, 'f32', 'f64'),
    # the CAPE/CIN-only kernels (late kernargs): the five pointers that select the all-outputs kernels NULL
    _cape('lean-exact-surface-f32>f64', C_, 'R', 'exact', 'surface', 0, 'f32', 'f64', LEAN),
    _cape('lean-exact-ml-f64>f32', C_, 'R', 'exact', 'mixed_layer', 0, 'f64', 'f32', LEAN),
    _cape('lean-family-mu-f32>f64', C_, 'R', 'family', 'most_unstable', 0, 'f32', 'f64', LEAN),
    _cape('lean-family-surface-f64>f32', C_, 'R', 'family', 'surface', 0, 'f64', 'f32', LEAN),
    _cape('lean-family-offtable-surface-f32>f64', C_ + ('rk4_redo',), 'off_table', 'family', 'surface', 0, 'f32', 'f64', LEAN),
    _cape('lean-family-offtable-mu-f64>f32', C_ + ('rk4_redo',), 'off_table', 'family', 'most_unstable', 0, 'f64', 'f32', LEAN),
    _cape('lean-family-nansurface-f32>f64', C_, 'nan_surface', 'family', 'surface', 0, 'f32', 'f64', LEAN),
    _cape('lean-family-persistent-f32>f64', C_, 'persistent', 'family', 'surface', 0, 'f32', 'f64', ('cape', 'cin')),
    _cape('lean-family-one-column-f64>f32', C_, 'one', 'family', 'surface', 0, 'f64', 'f32', LEAN),
    _cape('lean-exact-two-levels-f32>f64', C_, 'R2', 'exact', 'surface', 0, 'f32', 'f64', LEAN),
    # xp_profile_out: dtype equal to / different from the views' (native6 / generic), six arrays / the lifted-index three,
    # nlev_out = nlev + 1 / nlev + 4, every layout, the lifted index with rows and alone, re-based (MU / ML) profiles
    _cape('prof-native6-f64-dense-surface', A + ('native6',), 'R', 'exact', 'surface', 0, 'f64', 'f64', profile=_profile('f64')),
    _cape('prof-native6-f32-padded-mu-pad', A + ('native6', 'finish_padding'), 'R', 'family', 'most_unstable', 0, 'f32', 'f32',
          profile=_profile('f32', 'padded', 3)),
    _cape('prof-generic-f32>f64-colmajor-ml', A + ('generic',), 'R', 'exact', 'mixed_layer', 0, 'f32', 'f32',
          profile=_profile('f64', 'column_major')),
    _cape('prof-generic-f64>f32-second-surface-pad', A + ('generic', 'finish_padding'), 'R', 'family', 'surface', 0, 'f64', 'f64',
          profile=_profile('f32', 'second_column', 3)),
    _cape('prof-subset-f64-dense-mu-pad', A + ('generic', 'finish_padding'), 'R', 'exact', 'most_unstable', 0, 'f64', 'f64',
          profile=_profile('f64', 'dense', 3, LIFTED_INDEX_VARS)),
    _cape('prof-subset-f32>f64-padded-ml-li', A + ('generic',), 'R', 'family', 'mixed_layer', 0, 'f32', 'f64',
          profile=_profile('f64', 'padded', 0, LIFTED_INDEX_VARS, True)),
    _cape('prof-subset-f64>f32-colmajor-surface-li', A + ('generic',), 'R', 'exact', 'surface', 4, 'f64', 'f64',
          profile=_profile('f32', 'column_major', 0, LIFTED_INDEX_VARS, True)),
    _cape('prof-subset-f32-second-mu-pad', A + ('generic', 'finish_padding'), 'R', 'family', 'most_unstable', 0, 'f32', 'f32',
          profile=_profile('f32', 'second_column', 3, LIFTED_INDEX_VARS)),
    _cape('prof-six-li-f32>f64-dense-surface', A + ('generic',), 'R', 'family', 'surface', 0, 'f32', 'f32',
          profile=_profile('f64', 'dense', 0, PROFILE_VARS, True)),
    _cape('prof-native6-li-f32-dense-ml', A + ('native6',), 'R', 'family', 'mixed_layer', 0, 'f32', 'f64',
          profile=_profile('f32', 'dense', 0, PROFILE_VARS, True)),
    # (the scalars' dtype f32, the profile's f64, the views' f32: all three differ where they can)
    _cape('li-alone-lazy-f32-scalars-f32-li-f64', C_ + ('lazy_lifted_index',), 'R', 'family', 'surface', 0, 'f32', 'f32', LEAN,
          profile=_profile('f64', vars=(), lifted_index=True)),
    _cape('li-alone-lazy-f64-scalars-f64-li-f32-mu', C_ + ('lazy_lifted_index',), 'R', 'family', 'most_unstable', 0, 'f64', 'f64',
          ('cape', 'cin'), profile=_profile('f32', vars=(), lifted_index=True)),
    _cape('li-alone-lazy-nansurface', C_ + ('lazy_lifted_index', 'blank'), 'nan_surface', 'family', 'surface', 0, 'f32', 'f64', LEAN,
          profile=_profile('f64', vars=(), lifted_index=True)),
    _cape('li-alone-lazy-offtable', C_ + ('lazy_lifted_index', 'rk4_redo'), 'off_table', 'family', 'surface', 0, 'f32', 'f64', LEAN,
          profile=_profile('f64', vars=(), lifted_index=True)),
    _cape('li-alone-exact-all-scalars-f32>f64', A, 'R', 'exact', 'surface', 0, 'f32', 'f64',
          profile=_profile('f64', vars=(), lifted_index=True)),
    _cape('prof-offtable-f32>f64-dense', A + ('generic', 'finish_padding', 'rk4_redo'), 'off_table', 'family', 'surface', 0, 'f32', 'f64',
          profile=_profile('f64', 'dense', 3)),
    # the NaN-surface grid: blank() under every layout
    _cape('blank-dense-native6-f64', A + ('native6', 'blank'), 'nan_surface', 'exact', 'surface', 0, 'f64', 'f64',
          profile=_profile('f64', 'dense', 0, PROFILE_VARS, True)),
    _cape('blank-padded-f32>f64-pad', A + ('generic', 'blank', 'finish_padding'), 'nan_surface', 'family', 'surface', 0, 'f32', 'f32',
          profile=_profile('f64', 'padded', 3, PROFILE_VARS, True)),
    _cape('blank-colmajor-f64>f32-pad', A + ('generic', 'blank', 'finish_padding'), 'nan_surface', 'exact', 'surface', 0, 'f64', 'f32',
          profile=_profile('f32', 'column_major', 3, LIFTED_INDEX_VARS, True)),
    _cape('blank-second-native6-f32', A + ('native6', 'blank'), 'nan_surface', 'family', 'surface', 0, 'f32', 'f64',
          profile=_profile('f32', 'second_column', 0)),
    # one and two levels, one column
    _cape('prof-one-level-f32>f64-dense-pad', A + ('generic', 'finish_padding'), 'R1', 'exact', 'surface', 0, 'f32', 'f64',
          profile=_profile('f64', 'dense', 3, PROFILE_VARS, True)),
    _cape('prof-one-level-f64-colmajor', A + ('native6',), 'R1', 'family', 'surface', 0, 'f64', 'f32', profile=_profile('f64', 'column_major')),
    _cape('prof-two-levels-f64>f32-colmajor', A + ('generic',), 'R2', 'family', 'mixed_layer', 0, 'f64', 'f64',
          profile=_profile('f32', 'column_major', 0)),
    _cape('prof-two-levels-f32-padded-mu-pad', A + ('native6', 'finish_padding'), 'R2', 'exact', 'most_unstable', 0, 'f32', 'f64',
          profile=_profile('f32', 'padded', 3)),
    _cape('prof-one-column-f32>f64-padded', A + ('generic', 'finish_padding'), 'one', 'exact', 'surface', 0, 'f32', 'f32', profile=_profile('f64', 'padded', 3)),
    # memory spaces: the six pairings of (views, scalars, profile) that are not all the same; a host profile is dense
    _cape('mem-DHH', A + ('generic', 'finish_padding'), 'R', 'family', 'surface', 0, 'f32', 'f64', view_mem='device', scalars_mem='host',
          profile=_profile('f64', 'dense', 3, PROFILE_VARS, True, mem='host')),
    _cape('mem-HDD', A + ('generic', 'finish_padding'), 'R', 'exact', 'most_unstable', 0, 'f64', 'f32', view_mem='host', scalars_mem='device',
          profile=_profile('f32', 'column_major', 3, mem='device')),
    _cape('mem-DHD', A + ('native6',), 'R', 'family', 'mixed_layer', 0, 'f32', 'f64', view_mem='device', scalars_mem='host',
          profile=_profile('f32', 'padded', 0, mem='device')),
    _cape('mem-DDH', A + ('native6',), 'R', 'exact', 'surface', 0, 'f64', 'f32', view_mem='device', scalars_mem='device',
          profile=_profile('f64', 'dense', 0, PROFILE_VARS, True, mem='host')),
    _cape('mem-HHD', C_ + ('lazy_lifted_index',), 'R', 'family', 'surface', 0, 'f32', 'f64', LEAN, view_mem='host', scalars_mem='host',
          profile=_profile('f64', vars=(), lifted_index=True, mem='device')),
    _cape('mem-HDH', A + ('generic', 'blank', 'finish_padding'), 'nan_surface', 'family', 'surface', 0, 'f64', 'f64', view_mem='host', scalars_mem='device',
          profile=_profile('f32', 'dense', 3, LIFTED_INDEX_VARS, True, mem='host')),
    _cape('mem-lean-DH', C_, 'R', 'family', 'most_unstable', 0, 'f32', 'f64', LEAN, view_mem='device', scalars_mem='host'),
    _cape('mem-lean-HD', C_ + ('rk4_redo',), 'off_table', 'family', 'surface', 0, 'f64', 'f32', LEAN, view_mem='host', scalars_mem='device'),
]

# xp_opts.compute = XP_F32 with f64 scalars (f32 views; nothing in the header forbids it)
COMPUTE32_CASES = [
    _cape('compute32-R', ('compute32',), 'R', 'family', 'surface', 0, 'f32', 'f64', LEAN, compute='f32'),
    _cape('compute32-offtable', ('compute32', 'rk4_redo'), 'off_table', 'family', 'surface', 0, 'f32', 'f64', LEAN, compute='f32'),
    _cape('compute32-nansurface-host-scalars', ('compute32',), 'nan_surface', 'family', 'surface', 0, 'f32', 'f64', LEAN, compute='f32',
          scalars_mem='host'),
]

# one fp32-grid-to-fp64-output result against the C oracle: family mode, GRID_B, each parcel kind
ORACLE_CASES = [_cape('oracle-B-family-%s-f32>f64' % pc, A, 'B', 'family', pc, 0, 'f32', 'f64') for pc in ls.PARCELS]


# ---- xp_cape_cin_multi ----------------------------------------------------------------------------------------------------------
MULTI_PARCELS = (('most_unstable', 300.0), ('mixed_layer', 100.0))


def _multi(id, fused, views, swapped, profiles):
    lean = dict(dtype='f32', mem='device', want=('cape', 'cin', 'lfc_pressure', 'el_pressure', 'parcel_index'))
    full = dict(dtype='f64', mem='host', want=ALL_SCALARS)
    sc = (full, lean) if swapped else (lean, full)
    pr = (None, None)
    if profiles:                                                       # parcel 0: a lifted index alone; parcel 1: six column-major rows
        li = dict(_profile(OTHER[views], vars=(), lifted_index=True), mem='device')
        six = dict(_profile(OTHER[views], 'column_major', 3), mem='device')
        pr = (li, six)
    reaches = ('fused_multi',) if fused else ('cape_cin_only', 'all_outputs')
    if profiles:
        reaches = ('all_outputs', 'generic', 'finish_padding') + (() if swapped else ('lazy_lifted_index',))
    return dict(id=id, entry='xp_cape_cin_multi', reaches=reaches, grid='R', moist='family', parcels=MULTI_PARCELS, opt=0, compute='f64',
                view_dtype=views, view_mem='device', scalars=sc, profiles=pr, fused=fused)


MULTI_CASES = [
    _multi('multi-fused-f64', True, 'f64', False, False), _multi('multi-fused-f32-swapped', True, 'f32', True, False),
    _multi('multi-fused-f32', True, 'f32', False, False), _multi('multi-fused-f64-swapped', True, 'f64', True, False),
    _multi('multi-passes-f32', False, 'f32', False, False), _multi('multi-passes-f64-swapped', False, 'f64', True, False),
    _multi('multi-passes-profiles-f64', False, 'f64', False, True), _multi('multi-passes-profiles-f32-swapped', False, 'f32', True, True),
]

# ---- the other entry points that take an xp_scalars_out: one dtype-crossed and one mem-crossed call each --------------------------
SCALARS_ENTRY_CASES = [dict(id='%s-%s' % (e, tag), entry=e, view_dtype=vd, view_mem=vm, out_dtype=od, out_mem=om)
                       for e in ('xp_lfc_el', 'xp_select_parcel', 'xp_rebase_profile')
                       for tag, vd, vm, od, om in (('f64>f32', 'f64', 'device', 'f32', 'device'), ('f32>f64', 'f32', 'device', 'f64', 'device'),
                                                   ('device>host', 'f64', 'device', 'f64', 'host'),
                                                   ('host>device', 'f32', 'host', 'f32', 'device'))]

# ---- rejections: (id, what is wrong, the return code's name, a word of xp_last_error()) ------------------------------------------------
REJECTIONS = [
    ('scalars-dtype', dict(scalars_dtype=7), 'XP_E_ARG', 'scalars: bad dtype'),
    ('profile-dtype', dict(profile_dtype=2), 'XP_E_ARG', 'profile: bad dtype'),
    ('nlev_out', dict(extra=-1), 'XP_E_ARG', 'profile: nlev_out'),
    ('host-profile-not-dense', dict(profile_mem='host', layout='padded'), 'XP_E_ARG', 'profile: host arrays must be dense'),
    ('lifted-index-pressure-zero', dict(lifted_index_pressure=0.0), 'XP_E_ARG', 'profile: lifted_index_pressure'),
    ('lifted-index-pressure-nan', dict(lifted_index_pressure=float('nan')), 'XP_E_ARG', 'profile: lifted_index_pressure'),
    ('scalars-mem', dict(scalars_mem=2), 'XP_E_ARG', 'scalars: mem'),
    ('profile-mem', dict(profile_mem=-1), 'XP_E_ARG', 'profile: mem'),
    ('negative-lev-stride', dict(lev_stride=-1), 'XP_E_ARG', 'profile: lev_stride'),
    ('negative-col-stride', dict(col_stride=-1), 'XP_E_ARG', 'profile: lev_stride and col_stride'),
]

# ---- entry points whose out struct must match the views (check_out in csrc/xparcel.hip) -----------------------------------------------
CHECK_OUT_ENTRIES = ('xp_downdraft_cape', 'xp_effective_inflow_layer', 'xp_cape_cin_layers', 'xp_bunkers_storm_motion',
                     'xp_storm_relative_helicity', 'xp_storm_relative_helicity_layers', 'xp_wind_layers', 'xp_thermo_layers',
                     'xp_sounding_indices', 'xp_isentropic_interpolation', 'xp_hydrostatic_height', 'xp_ncape')
CHECK_OUT_CASES = [dict(id='%s-%s' % (e, kind), entry=e, crossed=kind) for e in CHECK_OUT_ENTRIES for kind in ('dtype', 'mem')]

ALL_CALL_CASES = CAPE_CASES + COMPUTE32_CASES + ORACLE_CASES + MULTI_CASES


def check_out_call_sites(source=None):
    """The entry points that hold their out struct to check_out(), read off csrc/xparcel.hip: the extern "C" function
    around every call, a shared body (a template that takes the entry's name) replaced by the entry points that call it."""
    if source is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, 'xarray_parcel_amd', 'csrc', 'xparcel.hip')) as f:
            source = f.read()
    head = re.compile(r'^(?:static )?(?:int|void|bool) (\w+)\(')
    fn, calls, users = None, set(), {}
    for line in source.split('\n'):
        m = head.match(line)
        if m:
            fn = m.group(1)
        if 'check_out(' in line and 'int check_out(' not in line:
            calls.add(fn)
        for body in re.findall(r'return (\w+)<', line):
            users.setdefault(body, set()).add(fn)
    out = set()
    for fn in calls:
        out |= {fn} if fn.startswith('xp_') else users.get(fn, {fn})
    return out
