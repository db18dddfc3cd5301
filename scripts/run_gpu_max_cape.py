"""Step time of CAPE / CIN of the maximum-CAPE parcel (XP_PARCEL_MAX_CAPE, csrc/xp_max_cape.hpp) next to the two calls
it is to be read against.

bench.py measures the flagship and is not touched by this feature, so the new path is measured here:
  grid      64 levels x 2^18 float32 columns from synth.columns_torch, device-resident; moist='family'; depth 300 hPa;
  sides     max_cape:       cape_cin_columns(parcel='max_cape', want=('cape', 'cin'))  -- selection, re-base, surface pass;
            most_unstable:  the same call with parcel='most_unstable' (the theta-e rule: one ascent per column);
            inflow_open:    effective_inflow_layer with thresholds every candidate passes (cape_min = -1, cin_min = -1e9):
                            the same sweep -- one ascent per candidate of the window -- already in the tree;
  protocol  one process; warm-up of every side and at least 0.6 s of pre-roll; then ROUNDS rounds, each STEPS steps of each
            side (order rotating), every step between two device events; a side's figure is the median of all its steps,
            its spread the range of its per-round medians;
  output    ms per step of each side, the ratios max_cape / inflow_open and max_cape / most_unstable, the mean number of
            candidates per column, and how many columns depart above level 0.
These are STEP times.  The kernels' own times come from a run of this script under a kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/run_gpu_max_cape.py --rounds 1 --steps 10
which --stats-from DIR --stats-out profiles/max_cape_stats.txt then condenses (no GPU needed for that).

    python scripts/run_gpu_max_cape.py [--out profiles/max_cape_bench.json] [--rounds 6] [--steps 20] [--ncol 262144]
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
DEPTH = 300.0


def condense(src, out):
    """The library's kernels out of rocprofv3's *kernel_stats.csv under `src`, as lines of text."""
    files = sorted(glob.glob(os.path.join(src, '**', '*kernel_stats.csv'), recursive=True))
    assert files, 'no *kernel_stats.csv under ' + src
    lines = ['rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/run_gpu_max_cape.py --rounds 1 --steps 10',
             '(a run of its own; 64 x 2^18 float32 columns, family mode, depth 300 hPa; 3 warm-up + pre-roll + 10 timed steps per side)', '',
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
    ap.add_argument('--out', default=os.path.join('profiles', 'max_cape_bench.json'))
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--ncol', type=int, default=1 << 18)
    ap.add_argument('--stats-from', default=None)
    ap.add_argument('--stats-out', default=os.path.join('profiles', 'max_cape_stats.txt'))
    a = ap.parse_args()
    if a.stats_from:
        return condense(a.stats_from, a.stats_out)
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from xarray_parcel_amd import _lib, numpy_api as xa, synth

    p, t, td = synth.columns_torch(NLEV, a.ncol, 'cuda', seed=20250718, dtype=torch.float32)
    kw = dict(moist='family', want=('cape', 'cin'))
    sides = {'max_cape': lambda: xa.cape_cin_columns(p, t, td, parcel='max_cape', depth=DEPTH, **kw),
             'most_unstable': lambda: xa.cape_cin_columns(p, t, td, parcel='most_unstable', depth=DEPTH, **kw),
             'inflow_open': lambda: xa.effective_inflow_layer(p, t, td, cape_min=-1.0, cin_min=-1e9, search_depth=DEPTH, moist='family')}
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
    for r in range(a.rounds):
        for side in order[r % 3:] + order[:r % 3]:
            ev = [step(side)[:2] for _ in range(a.steps)]
            torch.cuda.synchronize()
            ms[side].append([e0.elapsed_time(e1) for e0, e1 in ev])
    idx = xa.max_cape_parcel(p, t, td, depth=DEPTH)['index']
    both = {k: sides[k]()['cape'] for k in ('max_cape', 'most_unstable')}
    inflow = sides['inflow_open']()
    torch.cuda.synchronize()
    result = {'csrc_sha': _lib.csrc_sha(), 'nlev': NLEV, 'ncol': a.ncol, 'dtype': 'float32', 'moist': 'family', 'depth_hpa': DEPTH,
              'rounds': a.rounds, 'steps_per_round': a.steps, 'what': 'step time (device events around the call), not kernel time',
              'device': torch.cuda.get_device_name(0),
              'candidates_per_column_mean': round(float((p >= p[0:1] - DEPTH).sum(dim=0).double().mean()), 3),
              'inflow_layer_spans_the_window': int((inflow['status'] & _lib.ST_LAYER_OPEN != 0).sum()),
              'columns_departing_above_level_0': int((idx > 0).sum()),
              'columns_with_larger_cape_than_most_unstable': int((both['max_cape'] > both['most_unstable'] + 1.0).sum())}
    for side, rounds in ms.items():
        allsteps = np.concatenate(rounds)
        per_round = [float(np.median(x)) for x in rounds]
        result[side] = {'ms_per_step': round(float(np.median(allsteps)), 4), 'round_medians_ms': [round(x, 4) for x in per_round],
                        'spread_ms': round(max(per_round) - min(per_round), 4), 'timed_steps': int(allsteps.size)}
    result['ratio_max_cape_over_inflow_open'] = round(result['max_cape']['ms_per_step'] / result['inflow_open']['ms_per_step'], 4)
    result['ratio_max_cape_over_most_unstable'] = round(result['max_cape']['ms_per_step'] / result['most_unstable']['ms_per_step'], 4)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
