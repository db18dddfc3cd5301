"""CPU-only checks of the drop-in boundary: the library loads and exports every symbol that
include/xparcel.h declares; the ctypes structures match the header's field order.  No compute."""
import ctypes as C
import os
import re

import pytest

from xarray_parcel_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'xparcel.h')).read()


def test_library_builds_and_loads():
    L.build()
    lib = L.load()
    assert lib.xp_version() == 100


def test_every_declared_symbol_is_exported():
    L.build()
    lib = L.load()
    declared = set(re.findall(r'^\s*(?:int|const char \*)\s*\*?\s*(xp_\w+)\s*\(', _header(), flags=re.M))
    assert declared == set(L.SYMBOLS), declared ^ set(L.SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s


def _struct_fields(name):
    m = re.search(r'typedef struct \{([^{}]*)\} ' + name + ';', _header(), flags=re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(','):
            names.append(re.sub(r'\[.*\]', '', part.strip().split()[-1].lstrip('*')))
    return names


@pytest.mark.parametrize('cname,ctype', [('xp_view', L.View), ('xp_parcel', L.Parcel), ('xp_opts', L.Opts),
                                          ('xp_scalars_out', L.ScalarsOut), ('xp_profile_out', L.ProfileOut),
                                          ('xp_tables', L.Tables)])
def test_ctypes_structs_follow_header(cname, ctype):
    assert _struct_fields(cname) == [f[0] for f in ctype._fields_]


def test_no_gpu_means_loud_failure():
    """Without a device the product must refuse, not fall back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from xarray_parcel_amd import numpy_api as xa
    import numpy as np
    with pytest.raises(L.XParcelError):
        xa.lcl(1000.0, 300.0, 290.0)
    assert 'oracle' not in open(os.path.join(ROOT, 'xarray_parcel_amd', 'numpy_api.py')).read().replace('# oracle', '')


_KINDS = {C.c_int32: 'int32', C.c_int64: 'int64', C.c_double: 'double'}


def _prototypes():
    """name -> parameter kinds (int32 / int64 / double / pointer) of every function include/xparcel.h declares."""
    body = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    protos = {}
    for name, params in re.findall(r'^\s*(?:int|const char \*)\s*(xp_\w+)\s*\(([^)]*)\)\s*;', body, flags=re.M):
        kinds = []
        for prm in params.split(','):
            prm = prm.strip()
            if prm == 'void':
                continue
            kinds.append('pointer' if '*' in prm else {'int': 'int32', 'int32_t': 'int32', 'int64_t': 'int64',
                                                         'double': 'double'}[prm.split()[0]])
        protos[name] = kinds
    return protos


def test_argtypes_follow_header():
    """_lib.ARGTYPES covers exactly the exported symbols, and every entry point's parameters have the count and kinds of
    its prototype: a scalar passed where the header has an int64_t or a double is converted, not truncated to an int."""
    protos = _prototypes()
    assert set(protos) == set(L.SYMBOLS) == set(L.ARGTYPES)
    for name, kinds in protos.items():
        got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES[name]]
        assert got == kinds, (name, got, kinds)


def test_call_decision_host_inputs():
    """NumPy arrays, CPU torch tensors and a mix of the two make a host call: inputs and outputs are host NumPy arrays
    of the promoted dtype, and nothing touches the library before the launch."""
    import numpy as np
    import torch
    from xarray_parcel_amd import numpy_api as xa
    a32 = np.linspace(1000.0, 300.0, 24, dtype=np.float32).reshape(4, 2, 3)
    cases = [((a32, a32), np.float32), ((a32, a32.astype(np.float64)), np.float64),
             ((torch.from_numpy(a32), torch.from_numpy(a32)), np.float32),
             ((torch.from_numpy(a32), torch.from_numpy(a32).double()), np.float64),
             ((a32, torch.from_numpy(a32)), np.float32), ((torch.from_numpy(a32), a32, 500.0), np.float64)]
    for xs, dt in cases:
        c = xa._Call(*xs)
        assert c.device is None and c.mem == L.XP_MEM_HOST and c.dtype == dt, (xs, dt)
        assert c.xp_dtype == (L.XP_F64 if dt == np.float64 else L.XP_F32)
        assert (c.nlev, c.ncol, c.hshape) == (4, 6, (2, 3))
        for a in c.ins:
            assert isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous
        for a in (c.per_col(torch.full((2, 3), 700.0)), c.per_col(700.0), c.mask(torch.ones(3, 6), (3, 6)),
                  c.out(c.hshape), c.out(c.hshape, np.int32)):
            assert isinstance(a, np.ndarray)
        so, out = c.scalars(('cape', 'lfc_index'), c.hshape)
        assert so.mem == L.XP_MEM_HOST and so.dtype == c.xp_dtype and so.cape == out['cape'].ctypes.data
        assert out['cape'].dtype == dt and out['lfc_index'].dtype == np.int32 and out['cape'].shape == (2, 3)
        po, prof = c.profile(('pressure',), c.nlev + 1, c.hshape, 500.0)
        assert po.mem == L.XP_MEM_HOST and po.nlev_out == 5 and prof['pressure'].shape == (5, 2, 3)
        assert isinstance(prof['lifted_index'], np.ndarray)
        v = c.view(c.ins[0])
        assert (v.mem, v.nlev, v.ncol, v.lev_stride, v.col_stride) == (L.XP_MEM_HOST, 4, 6, 6, 1)
    with pytest.raises(AssertionError, match='per-column argument does not match the grid'):
        xa._Call(a32).per_col(np.ones(5))


def test_error_codes_follow_header():
    """_lib's XP_OK / XP_E_* constants are the header's error-code enum, name for name and value for value."""
    body = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    enum = re.search(r'enum\s*\{([^{}]*\bXP_E_ARG\b[^{}]*)\}', body).group(1)
    declared = {k: int(v) for k, v in re.findall(r'(XP_(?:OK|E_\w+))\s*=\s*(-?\d+)', enum)}
    ours = {k: getattr(L, k) for k in dir(L) if k == 'XP_OK' or k.startswith('XP_E_')}
    assert declared == ours and len(ours) == 7, (declared, ours)
