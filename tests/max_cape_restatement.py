"""NumPy restatement of XP_PARCEL_MAX_CAPE as include/xparcel.h specifies it, built from the oracle: candidate k of a column
is lifted with oracle.c_oracle.cape_cin_grid(p[k:], t[k:], td[k:], parcel='surface'), nothing else.

Per column:
  1. a level is valid when p, T and Td are all non-NaN; p0 = the pressure of the lowest valid level; the candidates are the
     valid levels with p >= p0 - depth (plain comparison), in level order (candidates());
  2. CAPE_k = the CAPE of the surface parcel of the column cut off below k, for every candidate: no early stop;
  3. k* = the lowest candidate whose CAPE_k is the largest: walking upward the first candidate is taken and then replaced
     only when CAPE_k > best, so a NaN never wins and all-zero CAPEs leave the lowest valid level; no candidate: k* = 0
     (choose());
  4. the re-based column has nlev rows: row j = level k* + j, NaN behind the column's top (rebase()).
The grid function walks k = 0, 1, ... and hands the oracle, at every k, the columns that lift candidate k, the way
tests/effective_layer_restatement.py does."""
import numpy as np

from oracle import c_oracle


def candidates(p, t, td, depth=300.0):
    """(nlev, ncol) bool: the candidate levels of every column.  Compared in float64 on the inputs as they are."""
    p, t, td = (np.asarray(a, dtype=np.float64) for a in (p, t, td))
    ncol = p.shape[1]
    valid = ~(np.isnan(p) | np.isnan(t) | np.isnan(td))
    has = valid.any(axis=0)
    k0 = np.where(has, np.argmax(valid, axis=0), 0)                      # the lowest valid level
    p0 = np.where(has, p[k0, np.arange(ncol)], np.nan)
    with np.errstate(invalid='ignore'):
        return valid & (p >= (p0 - float(depth))[None, :])


def choose(cand, cape):
    """k* (ncol,) int32 from the candidate mask and the candidates' CAPEs, both (nlev, ncol)."""
    nlev, ncol = cand.shape
    kstar = np.zeros(ncol, dtype=np.int32)
    best = np.full(ncol, np.nan)
    have = np.zeros(ncol, dtype=bool)
    for k in range(nlev):
        with np.errstate(invalid='ignore'):
            take = cand[k] & (~have | (cape[k] > best))
        kstar[take] = k
        best[take] = cape[k, take]
        have |= cand[k]
    return kstar


def rebase(p, t, td, kstar):
    """The three arrays with every column moved down by its k*, NaN behind its top; shape and dtype kept."""
    nlev, ncol = np.shape(p)
    src = np.arange(nlev)[:, None] + np.asarray(kstar)[None, :]
    live = src < nlev
    src = np.minimum(src, nlev - 1)
    cols = np.arange(ncol)[None, :]
    return tuple(np.where(live, np.asarray(a)[src, cols], np.nan).astype(np.asarray(a).dtype) for a in (p, t, td))


def tie_class(cand, cape, rel=1e-6):
    """True for the columns whose best and second-best candidate CAPE lie within rel * max(1, best) of each other: which of
    the two wins hangs on the last digits.  A column whose best CAPE is exactly 0 is not in the class: with the sign-filtered
    sums a CAPE of 0 is an empty sum, exact in every implementation, and the rule gives such a column its lowest valid level."""
    c = np.where(cand, cape, np.nan)
    c = np.where(np.isnan(c), -np.inf, c)
    s = np.sort(c, axis=0)
    best = s[-1]
    second = s[-2] if s.shape[0] > 1 else np.full_like(best, -np.inf)
    with np.errstate(invalid='ignore'):
        return np.isfinite(best) & np.isfinite(second) & (best != 0.0) & (best - second <= rel * np.maximum(1.0, best))


def max_cape_grid(p, t, td, depth=300.0, moist='rk4', **opts):
    """(nlev, ncol) arrays -> dict: 'kstar' (ncol,) int32, 'candidates' (nlev, ncol) bool, 'candidate_cape' (nlev, ncol; NaN
    where the level is no candidate), 'tie' (ncol,) bool, and 'pressure' / 'temperature' / 'dewpoint', the re-based arrays."""
    cand = candidates(p, t, td, depth)
    p64, t64, td64 = (np.asarray(a, dtype=np.float64) for a in (p, t, td))
    cape = np.full(cand.shape, np.nan)
    for k in range(cand.shape[0]):
        act = np.nonzero(cand[k])[0]
        if act.size:
            cape[k, act] = c_oracle.cape_cin_grid(p64[k:, act], t64[k:, act], td64[k:, act], parcel='surface', moist=moist, **opts)['cape']
    kstar = choose(cand, cape)
    rp, rt, rtd = rebase(p, t, td, kstar)
    return {'kstar': kstar, 'candidates': cand, 'candidate_cape': cape, 'tie': tie_class(cand, cape),
            'pressure': rp, 'temperature': rt, 'dewpoint': rtd}
