"""Step time of surface CAPE / CIN in family mode with compute='float64' against compute='float32' (csrc/xp_cape_f32.hpp).

bench.py measures the fp64 flagship and is not touched by this feature, so the fp32 walk is measured here:
  grid      c4's per-rank shape cut to one slab: 128 x 2^20 float32 columns from synth.columns_torch, hashed (neighbouring
            columns unrelated) and smooth=True (neighbouring columns alike, as model fields are);
  path      cape_cin_columns(parcel='surface', moist='family', want=('cape', 'cin')) on device tensors;
  protocol  one process; warm-up of both sides and at least 0.5 s of pre-roll; then ROUNDS rounds, each STEPS steps of
            one side followed by STEPS steps of the other, every step between two device events; a side's figure is the median
            of all its steps, its spread the range of its per-round medians;
  output    ms per step, columns/s, algorithmic bytes (1 544 B per column: 3 x 128 float32 levels + two float32 outputs)
            over time as a share of 8 TB/s, the ratio fp64 / fp32, and the doubt-column share of a 4 096-column strided
            sample by the CPU census of tests/compute32_cases.py.
These are STEP times (the call: staging of the arguments, the family pass, the RK4 pass over the flagged columns), not
kernel times.

    python scripts/run_gpu_compute32.py [--out profiles/compute32_bench.json] [--rounds 6] [--steps 40] [--ncol 1048576]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

NLEV = 128
BYTES_PER_COLUMN = 3 * NLEV * 4 + 2 * 4
HBM_BYTES_PER_S = 8.0e12


def doubt_share(p, t, td, sample=4096):
    """Share of a strided sample of columns with a doubt node, by the CPU census (the C oracle's profile)."""
    from oracle import c_oracle as co
    from tests import compute32_cases as cc
    step = max(1, p.shape[1] // sample)
    cols = [a[:, ::step][:, :sample].cpu().numpy() for a in (p, t, td)]
    prof = co.cape_cin_grid(*cols, parcel='surface', moist='rk4', want_profile=True)['profile']
    with np.errstate(invalid='ignore'):
        y = prof['virtual_temperature'] - prof['environment_virtual_temperature']
        return float((np.abs(y[1:]) < cc.guard()).any(axis=0).mean()), int(cols[0].shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'compute32_bench.json'))
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--ncol', type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from xarray_parcel_amd import _lib, numpy_api as xa, synth

    def step(p, t, td, compute):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = xa.cape_cin_columns(p, t, td, parcel='surface', moist='family', want=('cape', 'cin'), compute=compute)
        e1.record()
        return e0, e1, r

    result = {'csrc_sha': _lib.csrc_sha(), 'nlev': NLEV, 'ncol': a.ncol, 'dtype': 'float32', 'rounds': a.rounds,
              'steps_per_round': a.steps, 'bytes_per_column': BYTES_PER_COLUMN, 'what': 'step time (device events around the call), not kernel time',
              'device': torch.cuda.get_device_name(0), 'grids': {}}
    for grid, smooth in (('hashed', False), ('smooth', True)):
        p, t, td = synth.columns_torch(NLEV, a.ncol, 'cuda', seed=20250721, dtype=torch.float32, smooth=smooth)
        outs = {}
        for compute in ('float64', 'float32'):                       # warm-up: code objects, scratch pools
            for _ in range(3):
                outs[compute] = step(p, t, td, compute)[2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()                                     # pre-roll
        while time.perf_counter() - t0 < 0.6:
            for compute in ('float64', 'float32'):
                step(p, t, td, compute)
            torch.cuda.synchronize()
        ms = {'float64': [], 'float32': []}
        for r in range(a.rounds):
            for compute in (('float64', 'float32') if r % 2 == 0 else ('float32', 'float64')):
                ev = [step(p, t, td, compute)[:2] for _ in range(a.steps)]
                torch.cuda.synchronize()
                ms[compute].append([e0.elapsed_time(e1) for e0, e1 in ev])
        rec = {}
        for compute, rounds in ms.items():
            allsteps = np.concatenate(rounds)
            med = float(np.median(allsteps))
            per_round = [float(np.median(x)) for x in rounds]
            rec[compute] = {'ms_per_step': round(med, 4), 'round_medians_ms': [round(x, 4) for x in per_round],
                            'spread_ms': round(max(per_round) - min(per_round), 4), 'timed_steps': int(allsteps.size),
                            'columns_per_s': round(a.ncol / (med * 1e-3)),
                            'hbm_share': round(BYTES_PER_COLUMN * a.ncol / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
        rec['ratio_f64_over_f32'] = round(rec['float64']['ms_per_step'] / rec['float32']['ms_per_step'], 4)
        rec['gain_ms'] = round(rec['float64']['ms_per_step'] - rec['float32']['ms_per_step'], 4)
        # faster "by more than the measured spread of either" side
        rec['f32_faster_beyond_spread'] = bool(rec['gain_ms'] > max(rec['float64']['spread_ms'], rec['float32']['spread_ms']))
        c64, c32 = (np.asarray(outs[k]['cape'].cpu(), dtype=np.float64) for k in ('float64', 'float32'))
        rec['max_abs_dcape_f32_vs_f64'] = float(np.max(np.abs(c64 - c32)))
        rec['max_abs_dcin_f32_vs_f64'] = float(np.max(np.abs(np.asarray(outs['float64']['cin'].cpu(), dtype=np.float64) -
                                                             np.asarray(outs['float32']['cin'].cpu(), dtype=np.float64))))
        rec['doubt_column_share'], rec['doubt_sample_columns'] = doubt_share(p, t, td)
        result['grids'][grid] = rec
        print(grid, json.dumps(rec), flush=True)
        del p, t, td
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
