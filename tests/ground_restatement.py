"""The re-based column of XP_PARCEL_OVER_GROUND in NumPy, written from the rules of include/xparcel.h (not from the kernel):
isobaric levels cut at the ground, the surface fields as row 0."""
import numpy as np


def levels_below_ground(p, ps):
    """k0 per column: the first level index with p[k0] < ps, a plain comparison (a NaN pressure compares false); nlev where no
    level lies above the ground.  p: (nlev, ncol) or the nlev isobars; ps: (ncol,)."""
    p, ps = np.asarray(p), np.asarray(ps).reshape(-1)
    if p.ndim == 1:
        p = p[:, None]
    with np.errstate(invalid='ignore'):
        above = np.broadcast_to(p, (p.shape[0], ps.size)) < ps[None, :]
    return np.where(above.any(axis=0), above.argmax(axis=0), p.shape[0]).astype(np.int64)


def rebase(p, t, m, ps, ts, tds):
    """(nlev + 1, ncol) pressure, temperature and moisture of the re-based columns, in the dtype of `t`: row 0 = (ps, Ts, Tds),
    row 1 + j = level k0 + j, NaN above; a column whose ps, Ts or Tds is NaN is NaN throughout.  `m` is copied like `t`: for
    specific-humidity input it has to be the dewpoint grid of xp_dewpoint_from_specific_humidity already."""
    t, m = np.asarray(t), np.asarray(m)
    nlev, ncol = t.shape
    p = np.broadcast_to(np.asarray(p).reshape(nlev, -1), (nlev, ncol))
    ps, ts, tds = (np.asarray(x).reshape(ncol) for x in (ps, ts, tds))
    out = [np.full((nlev + 1, ncol), np.nan, dtype=t.dtype) for _ in range(3)]
    k0 = levels_below_ground(p, ps)
    for c in range(ncol):
        if np.isnan(ps[c]) or np.isnan(ts[c]) or np.isnan(tds[c]):
            continue
        n = nlev - k0[c]
        for o, src, sfc in zip(out, (p, t, m), (ps, ts, tds)):
            o[0, c] = sfc[c]
            o[1:1 + n, c] = src[k0[c]:, c]
    return tuple(out)
