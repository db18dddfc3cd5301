"""bench.py --dump-outputs writer (bench.dump_outputs) on host tensors: whole arrays under the size cap; above it, the same
fixed, seeded sample of positions in every array, in the arrays' own dtypes, identical from call to call."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)


def test_dump_whole_arrays_under_the_cap(tmp_path):
    arrays = {'surface_cape': torch.arange(1000, dtype=torch.float64), 'surface_cin': -torch.arange(1000, dtype=torch.float64)}
    rec = bench.dump_outputs(str(tmp_path), arrays)
    assert rec['columns'] == rec['columns_total'] == 1000 and rec['sample'] is None and rec['arrays'] == list(arrays)
    for name, v in arrays.items():
        got = np.load(tmp_path / (name + '.npy'))
        assert got.dtype == np.float64 and np.array_equal(got, v.numpy())


def test_dump_samples_the_same_columns_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 8000)          # four float32 arrays: 500 columns fit
    n = 10000
    names = [f'{pc}_{k}' for pc in ('most_unstable', 'mixed_layer') for k in ('cape', 'cin')]
    arrays = {name: torch.arange(n, dtype=torch.float32) + 100000 * i for i, name in enumerate(names)}
    recs = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ('a', 'b')]
    assert recs[0] == dict(recs[1], dir=recs[0]['dir'])
    assert recs[0]['columns'] == 500 and recs[0]['columns_total'] == n and recs[0]['sample']
    pos = None
    for i, name in enumerate(arrays):
        a, b = np.load(tmp_path / 'a' / (name + '.npy')), np.load(tmp_path / 'b' / (name + '.npy'))
        assert a.dtype == np.float32 and a.shape == (500,) and np.array_equal(a, b)
        p = a - 100000 * i                                      # the positions this array kept
        assert np.all(np.diff(p) > 0) and p[0] >= 0 and p[-1] < n
        assert pos is None or np.array_equal(p, pos)
        pos = p
    assert sum(os.path.getsize(tmp_path / 'a' / (name + '.npy')) for name in arrays) <= 8000 + 4 * 256   # + .npy headers
