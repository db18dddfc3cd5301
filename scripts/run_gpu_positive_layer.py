"""Step time of the positive-layer choice of the CAPE / CIN calls (XP_OPT_LAYER_*, csrc/xp_cape_pick.hpp) next to the
exact-mode default call it replaces.

bench.py measures the flagship and is not touched by this feature, so the new path is measured here:
  grid      64 levels x 2^20 float64 columns from synth.columns_torch, device-resident; surface parcel; moist='exact';
  sides     envelope:   cape_cin_columns(want=('cape', 'cin'))  -- the default call, the kernels of the parent commit
                        (their code objects are unchanged by this feature);
            envelope_all: the default call with every scalar (the all-outputs kernel, what the layer kernel tracks too);
            lowest / highest / deepest / most_cape: the same call with positive_layer=, every scalar;
            layers_one: cape_cin_layers with one layer -- the sibling kernel at the same occupancy;
  protocol  one process; warm-up of every side and at least 0.6 s of pre-roll; then ROUNDS rounds, each STEPS steps of each
            side (order rotating), every step between two device events; a side's figure is the median of all its steps,
            its spread the range of its per-round medians;
  output    ms per step of each side and the ratio of each choice to envelope_all, and in how many columns each choice
            moves the CAPE off the default's.
These are STEP times.  The kernels' own times come from a run of this script under a kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/run_gpu_positive_layer.py --rounds 1 --steps 10
which --stats-from DIR --stats-out profiles/positive_layer_stats.txt then condenses (no GPU needed for that).

    python scripts/run_gpu_positive_layer.py [--out profiles/positive_layer_bench.json] [--rounds 6] [--steps 20] [--ncol 1048576]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

NLEV = 64
CHOICES = ('lowest', 'highest', 'deepest', 'most_cape')


def condense(src, out):
    """The library's kernels out of rocprofv3's *kernel_stats.csv under `src`, as lines of text."""
    files = sorted(glob.glob(os.path.join(src, '**', '*kernel_stats.csv'), recursive=True))
    assert files, 'no *kernel_stats.csv under ' + src
    lines = ['rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/run_gpu_positive_layer.py --rounds 1 --steps 10',
             '(a run of its own; 64 x 2^20 float64 columns, surface parcel, exact mode; 3 warm-up + pre-roll + 10 timed steps per side)', '',
             'Name, Calls, AverageNs, MinNs, MaxNs, Percentage']
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            if 'xp::' in row['Name']:
                lines.append(', '.join(str(row.get(k, '')) for k in ('Name', 'Calls', 'AverageNs', 'MinNs', 'MaxNs', 'Percentage')))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'positive_layer_bench.json'))
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--ncol', type=int, default=1 << 20)
    ap.add_argument('--stats-from', default=None)
    ap.add_argument('--stats-out', default=os.path.join('profiles', 'positive_layer_stats.txt'))
    a = ap.parse_args()
    if a.stats_from:
        return condense(a.stats_from, a.stats_out)
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from xarray_parcel_amd import _lib, numpy_api as xa, synth

    p, t, td = synth.columns_torch(NLEV, a.ncol, 'cuda', seed=20250718, dtype=torch.float64)
    top = torch.full((a.ncol,), 500.0, dtype=torch.float64, device='cuda')
    sides = {'envelope': lambda: xa.cape_cin_columns(p, t, td, moist='exact', want=('cape', 'cin')),
             'envelope_all': lambda: xa.cape_cin_columns(p, t, td, moist='exact'),
             'layers_one': lambda: xa.cape_cin_layers(p, t, td, [{'top': top}], moist='exact')}
    for ch in CHOICES:
        sides[ch] = (lambda ch: lambda: xa.cape_cin_columns(p, t, td, moist='exact', positive_layer=ch))(ch)
    order = list(sides)

    def step(side):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = sides[side]()
        e1.record()
        return e0, e1, r
    for side in order:                                               # warm-up: code objects, scratch pools
        for _ in range(3):
            step(side)
    torch.cuda.synchronize()
    t0 = time.perf_counter()                                         # pre-roll
    while time.perf_counter() - t0 < 0.6:
        for side in order:
            step(side)
        torch.cuda.synchronize()
    ms = {side: [] for side in order}
    n = len(order)
    for r in range(a.rounds):
        for side in order[r % n:] + order[:r % n]:
            ev = [step(side)[:2] for _ in range(a.steps)]
            torch.cuda.synchronize()
            ms[side].append([e0.elapsed_time(e1) for e0, e1 in ev])
    default = sides['envelope_all']()['cape']
    moved = {ch: int((sides[ch]()['cape'] != default).sum()) for ch in CHOICES}
    torch.cuda.synchronize()
    result = {'csrc_sha': _lib.csrc_sha(), 'nlev': NLEV, 'ncol': a.ncol, 'dtype': 'float64', 'moist': 'exact', 'parcel': 'surface',
              'rounds': a.rounds, 'steps_per_round': a.steps, 'what': 'step time (device events around the call), not kernel time',
              'device': torch.cuda.get_device_name(0), 'columns_whose_cape_leaves_the_default': moved}
    for side, rounds in ms.items():
        allsteps = np.concatenate(rounds)
        per_round = [float(np.median(x)) for x in rounds]
        result[side] = {'ms_per_step': round(float(np.median(allsteps)), 4), 'round_medians_ms': [round(x, 4) for x in per_round],
                        'spread_ms': round(max(per_round) - min(per_round), 4), 'timed_steps': int(allsteps.size)}
    for ch in CHOICES:
        result['ratio_%s_over_envelope_all' % ch] = round(result[ch]['ms_per_step'] / result['envelope_all']['ms_per_step'], 4)
        result['ratio_%s_over_envelope' % ch] = round(result[ch]['ms_per_step'] / result['envelope']['ms_per_step'], 4)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
