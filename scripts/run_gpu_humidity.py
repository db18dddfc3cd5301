"""Step time of a CAPE / CIN call by what its moisture view holds: dewpoint, specific humidity, relative humidity, mixing ratio.

bench.py measures the flagship and is not touched by this feature, so the front pass of XP_HUM_RELATIVE / XP_HUM_MIXING_RATIO
(csrc/xp_humidity.hpp) is measured here, by bench.py's own protocol:
  grid      BASELINE config c2's: 64 levels x 1024 x 1024 columns from synth.columns_torch, device-resident, as float64 and as
            float32; relative humidity, mixing ratio and specific humidity derived from its dewpoints on the device in float64;
  sides     cape_cin_columns(parcel='surface', moist='family', want=('cape', 'cin')) with humidity='dewpoint', 'specific',
            'relative', 'mixing_ratio';
  protocol  one process; warm-up of every side and at least 0.6 s of pre-roll; then ROUNDS rounds, each STEPS steps of each
            side (order rotating), every step between two device events; a side's figure is the median of all its steps,
            its spread the range of its per-round medians;
  output    ms per step of each side, the ratios to the dewpoint call, the extra time of the two new kinds, and the bytes
            their front pass moves (two arrays read, one written).
These are STEP times: the extra time of a new kind holds the front kernel, its launch, the stream-ordered allocation of its
scratch array and whatever the lift gains or loses by reading a dense D, so it is not the divisor for a bandwidth.  The
kernel's own time -- and with front_pass_bytes its achieved bandwidth -- comes from a run of this script under a kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/run_gpu_humidity.py --rounds 1 --steps 10
which --stats-from DIR --stats-out profiles/humidity_stats.txt then condenses (no GPU needed for that).

    python scripts/run_gpu_humidity.py [--out profiles/humidity_bench.json] [--rounds 6] [--steps 20] [--ncol 1048576]
                                       [--kinds dewpoint,specific]    (with XPARCEL_LIB: another build of the library)
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
KINDS = ('dewpoint', 'specific', 'relative', 'mixing_ratio')
EPS = 0.6219569100577033


def condense(src, out):
    """The library's kernels out of rocprofv3's *kernel_stats.csv under `src`, as lines of text."""
    files = sorted(glob.glob(os.path.join(src, '**', '*kernel_stats.csv'), recursive=True))
    assert files, 'no *kernel_stats.csv under ' + src
    lines = ['rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/run_gpu_humidity.py --rounds 1 --steps 10',
             '(a run of its own; 64 x 2^20 columns, float64 then float32, family mode; 3 warm-up + pre-roll + 10 timed steps per side)', '',
             'Name, Calls, AverageNs, MinNs, MaxNs, Percentage']
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            if 'xp::' in row['Name']:
                lines.append(', '.join(str(row.get(k, '')) for k in ('Name', 'Calls', 'AverageNs', 'MinNs', 'MaxNs', 'Percentage')))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def moistures(torch, p, t, td, dtype):
    """dewpoint, specific humidity, relative humidity and mixing ratio of the grid in `dtype`, derived in float64 level by level."""
    es = lambda x: 6.112 * torch.exp(17.67 * (x - 273.15) / (x - 29.65))
    out = {k: torch.empty(p.shape, dtype=dtype, device=p.device) for k in KINDS}
    for k in range(p.shape[0]):
        e = es(td[k].double())
        est = es(t[k].double())
        w = EPS * e / (p[k].double() - e)
        wq = EPS * e / (p[k].double() - est)             # the w that XP_HUM_SPECIFIC's chain (MetPy 1.4.1: RH = w / w_s(p, T)) maps back to e
        out['dewpoint'][k] = td[k].to(dtype)
        out['relative'][k] = (e / est).to(dtype)
        out['mixing_ratio'][k] = w.to(dtype)
        out['specific'][k] = (wq / (1.0 + wq)).to(dtype)
    return out


def measure(torch, xa, p, t, m, rounds, steps, kinds):
    sides = {k: (lambda k=k: xa.cape_cin_columns(p, t, m[k], parcel='surface', moist='family', humidity=k, want=('cape', 'cin'))) for k in kinds}
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
    for r in range(rounds):
        k = r % len(order)
        for side in order[k:] + order[:k]:
            ev = [step(side)[:2] for _ in range(steps)]
            torch.cuda.synchronize()
            ms[side].append([e0.elapsed_time(e1) for e0, e1 in ev])
    res = {}
    for side, per in ms.items():
        allsteps = np.concatenate(per)
        med = [float(np.median(x)) for x in per]
        res[side] = {'ms_per_step': round(float(np.median(allsteps)), 4), 'round_medians_ms': [round(x, 4) for x in med],
                     'spread_ms': round(max(med) - min(med), 4), 'timed_steps': int(allsteps.size)}
    base = res['dewpoint']['ms_per_step']
    cape = {k: sides[k]()['cape'] for k in kinds}
    torch.cuda.synchronize()
    front_bytes = 3 * p.numel() * p.element_size()
    for k in kinds[1:]:
        res[k]['ratio_to_dewpoint'] = round(res[k]['ms_per_step'] / base, 4)
        res[k]['max_abs_cape_difference_to_dewpoint_J_per_kg'] = float((cape[k] - cape['dewpoint']).abs().max())
    for k in [k for k in kinds if k in ('relative', 'mixing_ratio')]:
        extra = res[k]['ms_per_step'] - base
        res[k]['extra_ms'] = round(extra, 4)
        res[k]['front_pass_bytes'] = front_bytes
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'humidity_bench.json'))
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--ncol', type=int, default=1 << 20)
    ap.add_argument('--kinds', default=','.join(KINDS), help="'dewpoint' first; a library of before the new kinds takes dewpoint,specific")
    ap.add_argument('--stats-from', default=None)
    ap.add_argument('--stats-out', default=os.path.join('profiles', 'humidity_stats.txt'))
    a = ap.parse_args()
    if a.stats_from:
        return condense(a.stats_from, a.stats_out)
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from xarray_parcel_amd import _lib, numpy_api as xa, synth

    kinds = tuple(a.kinds.split(','))
    assert kinds[0] == 'dewpoint' and all(k in KINDS for k in kinds)
    p, t, td = synth.columns_torch(NLEV, a.ncol, 'cuda', seed=20250718, dtype=torch.float64)
    result = {'csrc_sha': _lib.csrc_sha(), 'library': os.path.relpath(_lib.LIB_PATH), 'nlev': NLEV, 'ncol': a.ncol, 'moist': 'family', 'parcel': 'surface', 'rounds': a.rounds,
              'steps_per_round': a.steps, 'what': 'step time (device events around the call), not kernel time',
              'device': torch.cuda.get_device_name(0)}
    for name, dtype in (('float64', torch.float64), ('float32', torch.float32)):
        m = moistures(torch, p, t, td, dtype)
        result[name] = measure(torch, xa, p.to(dtype), t.to(dtype), m, a.rounds, a.steps, kinds)
        del m
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
