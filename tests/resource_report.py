"""What the compiler says about the kernels of one translation unit, without a GPU: hipcc cross-compiles the unit for
gfx950 to device assembly with -Rpass-analysis=kernel-resource-usage.  Device assembly instead of an object: the resource
remarks come out the same, and the text shows whether a kernel itself spills (ScratchSize also counts the frames of the
out-of-line slow paths it calls)."""
import os
import re
import shutil
import subprocess

import pytest

from xarray_parcel_amd import _lib

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which('hipcc')), reason='hipcc not available')

_REMARKS = (('vgprs', r' VGPRs: (\d+)'), ('vgpr_spill', r'VGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
            ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)'), ('lds', r'LDS Size \[bytes/block\]: (\d+)'))


def resources(tmp_path, src, flags=()):
    """Compile csrc/`src` with the library's flags plus `flags`.  Returns {mangled kernel name: {'vgprs', 'vgpr_spill',
    'scratch' [bytes/lane], 'occupancy' [waves/SIMD], 'lds' [bytes/block]: the compiler's remarks; 'in_asm': the kernel's
    body was found in the assembly; 'scratch_insts': scratch loads / stores in that body; 'spills': those plus the
    register allocator's folded spills and reloads}}."""
    asm_path = os.path.join(str(tmp_path), 'unit.s')
    cmd = ([HIPCC if os.path.exists(HIPCC) else 'hipcc'] + [f for f in _lib.HIPCC_FLAGS if f != '-fPIC'] + list(flags) +
           ['-S', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-o', asm_path, os.path.join(_lib.SRC_DIR, src)])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(asm_path) as f:
        asm = f.read()
    rec, name = {}, None
    for ln in out.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', ln)
        if m:
            name = m.group(1)
            rec[name] = {}
        for key, pat in _REMARKS:
            m = re.search(pat, ln)
            if m and name:
                rec[name][key] = int(m.group(1))
    for name, r in rec.items():
        i = asm.find('\n' + name + ':')
        body = asm[i:asm.find('.Lfunc_end', i)] if i >= 0 else ''
        r['in_asm'] = i >= 0
        r['scratch_insts'] = len(re.findall(r'scratch_(?:load|store)', body))
        r['spills'] = len(re.findall(r'scratch_(?:load|store)|Folded (?:Spill|Reload)', body))
    return rec
