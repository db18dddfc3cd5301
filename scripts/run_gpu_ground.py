"""Step time of surface CAPE / CIN over the ground (XP_PARCEL_OVER_GROUND, csrc/xp_ground.hpp) against the ordinary call on
a grid that was re-based beforehand.

bench.py measures the flagship on model levels and is not touched by this feature, so the ground path is measured here:
  grid      the benchmark's own shape: 64 x 2^20 float64 columns from synth.columns_torch, device-resident;
  ground    every column is cut between two of its lowest levels: the number of levels below the ground, 0 ... 8, follows a
            smooth wave over the (y, x) grid ('smooth': runs of equal k0, as terrain gives) or a hash ('hashed': neighbouring
            columns unrelated); the surface values are those of the column at that pressure (linear in ln p);
  paths     flagged:   cape_cin_columns(p, T, Td, parcel='surface', moist='family', want=('cape', 'cin'), ground=(ps, Ts, Tds));
            prebuilt:  the same call without ground= on the (65, ncol) re-based arrays, built once with torch outside the timing;
  protocol  one process; warm-up of both sides and at least 0.6 s of pre-roll; then ROUNDS rounds, each STEPS steps of one
            side followed by STEPS steps of the other (order alternating), every step between two device events; a side's
            figure is the median of all its steps, its spread the range of its per-round medians;
  output    ms per step of both, their ratio, and a check that both give the same CAPE and CIN bit for bit.
These are STEP times (the call: staging of the arguments, the re-basing kernel, the family pass, the RK4 pass over the
flagged columns).  The re-basing kernel's own time comes from a run of this script under a kernel trace (--rounds 1).

    python scripts/run_gpu_ground.py [--out profiles/ground_bench.json] [--rounds 6] [--steps 30] [--ncol 1048576]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

NLEV = 64
MAX_DROPPED = 8


def ground(torch, synth, p, t, td, smooth, seed=7):
    """k0 (levels dropped, 0 ... MAX_DROPPED) and ps, Ts, Tds between levels k0 - 1 and k0 (k0 = 0: under level 0)."""
    ncol = p.shape[1]
    u = (synth.column_uniforms_smooth if smooth else synth.column_uniforms)(ncol, seed)
    k0 = torch.from_numpy(np.minimum((u[0] * (MAX_DROPPED + 1)).astype(np.int64), MAX_DROPPED)).cuda()
    f = torch.from_numpy(0.1 + 0.8 * u[1]).cuda()
    lo, hi = (k0 - 1).clamp(min=0)[None, :], k0[None, :]
    take = lambda a, k: torch.gather(a, 0, k)[0]
    x = torch.log(take(p, lo)) * (1 - f) + torch.log(take(p, hi)) * f
    ps = torch.where(k0 == 0, take(p, hi) + 5.0 * f, torch.exp(x))
    w = torch.where(k0 == 0, torch.zeros_like(f), f)
    ts = take(t, lo) * (1 - w) + take(t, hi) * w
    tds = take(td, lo) * (1 - w) + take(td, hi) * w
    return k0, ps, ts, tds


def prebuilt(torch, arrays, surface, k0):
    nlev, ncol = arrays[0].shape
    idx = k0[None, :] + torch.arange(nlev, device='cuda')[:, None]
    out = []
    for a, s in zip(arrays, surface):
        body = torch.where(idx < nlev, torch.gather(a, 0, idx.clamp(max=nlev - 1)), torch.full_like(a, float('nan')))
        out.append(torch.cat([s[None, :], body]).contiguous())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'ground_bench.json'))
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--ncol', type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from xarray_parcel_amd import _lib, numpy_api as xa, synth

    kw = dict(parcel='surface', moist='family', want=('cape', 'cin'))
    result = {'csrc_sha': _lib.csrc_sha(), 'nlev': NLEV, 'ncol': a.ncol, 'dtype': 'float64', 'rounds': a.rounds, 'steps_per_round': a.steps,
              'what': 'step time (device events around the call), not kernel time', 'device': torch.cuda.get_device_name(0), 'grids': {}}
    p, t, td = synth.columns_torch(NLEV, a.ncol, 'cuda', seed=20250718, dtype=torch.float64)
    for name, smooth in (('smooth', True), ('hashed', False)):
        k0, ps, ts, tds = ground(torch, synth, p, t, td, smooth)
        rp, rt, rtd = prebuilt(torch, (p, t, td), (ps, ts, tds), k0)
        sides = {'flagged': lambda: xa.cape_cin_columns(p, t, td, ground=(ps, ts, tds), **kw),
                 'prebuilt': lambda: xa.cape_cin_columns(rp, rt, rtd, **kw)}

        def step(side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = sides[side]()
            e1.record()
            return e0, e1, r
        outs = {}
        for side in sides:                                           # warm-up: code objects, scratch pools
            for _ in range(3):
                outs[side] = step(side)[2]
        torch.cuda.synchronize()
        same = all(bool(((outs['flagged'][k] == outs['prebuilt'][k]) | (outs['flagged'][k].isnan() & outs['prebuilt'][k].isnan())).all())
                   for k in ('cape', 'cin'))
        t0 = time.perf_counter()                                     # pre-roll
        while time.perf_counter() - t0 < 0.6:
            for side in sides:
                step(side)
            torch.cuda.synchronize()
        ms = {side: [] for side in sides}
        for r in range(a.rounds):
            for side in (('flagged', 'prebuilt') if r % 2 == 0 else ('prebuilt', 'flagged')):
                ev = [step(side)[:2] for _ in range(a.steps)]
                torch.cuda.synchronize()
                ms[side].append([e0.elapsed_time(e1) for e0, e1 in ev])
        rec = {'levels_dropped_mean': round(float(k0.double().mean()), 3), 'bit_identical_cape_cin': same,
               'columns_with_cape': int((outs['flagged']['cape'] > 0).sum())}
        for side, rounds in ms.items():
            allsteps = np.concatenate(rounds)
            per_round = [float(np.median(x)) for x in rounds]
            rec[side] = {'ms_per_step': round(float(np.median(allsteps)), 4), 'round_medians_ms': [round(x, 4) for x in per_round],
                         'spread_ms': round(max(per_round) - min(per_round), 4), 'timed_steps': int(allsteps.size)}
        rec['ratio_flagged_over_prebuilt'] = round(rec['flagged']['ms_per_step'] / rec['prebuilt']['ms_per_step'], 4)
        rec['extra_ms'] = round(rec['flagged']['ms_per_step'] - rec['prebuilt']['ms_per_step'], 4)
        result['grids'][name] = rec
        print(name, json.dumps(rec), flush=True)
        del rp, rt, rtd
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
