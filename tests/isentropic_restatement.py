"""NumPy restatement of xp_isentropic_interpolation (include/xparcel.h has the rules), one column at a time.  The steps:
  1. valid levels: p and T non-NaN; the others are dropped (a NaN in an extra variable drops nothing);
  2. x = ln p and theta = T exp(kappa (ln 1000 - x)) of every valid level;
  3. per target theta*: the pairs of consecutive valid levels (k, k + 1) where (theta_k <= theta*) differs from
     (theta_k+1 <= theta*); the lowest of them (from_below) or the highest; none: NaN and XP_ST_NO_LAYER;
  4. T = a x + b on the pair; Newton on f(x) = theta* - (a x + b) exp(kappa (ln 1000 - x)) from the pair's midpoint in x,
     converged after the step with |x_new - x| <= eps, at most max_iters steps; otherwise NaN and XP_ST_NOT_CONVERGED;
  5. pressure = exp(x), temperature = theta* exp(-kappa (ln 1000 - x)), the extras linear in theta on the same pair."""
import numpy as np

ST_NO_LAYER, ST_NOT_CONVERGED = 16, 256
MAX_LEVELS = 64
KAPPA = 2.0 / 7.0
LN1000 = float(np.log(1000.0))
NAN = float('nan')


def theta_of(x, t):
    return t * np.exp(KAPPA * (LN1000 - x))


def newton(theta, x0, t0, x1, t1, max_iters=50, eps=1e-6):
    """Step 4 on the pair (x0, t0), (x1, t1), level k first: (x or NaN, steps taken, converged)."""
    a = (t1 - t0) / (x1 - x0)
    b = t1 - a * x1
    x = 0.5 * (x0 + x1)
    for it in range(1, max_iters + 1):
        e = np.exp(KAPPA * (LN1000 - x))
        t = a * x + b
        f = theta - e * t
        fp = e * (KAPPA * t - a)
        xn = x - f / fp
        conv = abs(xn - x) <= eps
        x = xn
        if conv:
            return float(x), it, True
    return NAN, max_iters, False


def column(p, t, levels, extras=(), from_below=True, max_iters=50, eps=1e-6):
    """One column.  Returns a dict: 'pressure', 'temperature' (nlevel), 'vars' (one array per extra), 'status', and for the
    census 'pairs' (per target the pairs (k, k + 1) of VALID-level positions holding a crossing), 'steps' (Newton steps
    per target, 0 where there is no pair), 'theta' (of the valid levels), 'pair' (the chosen pair's position or -1) and
    'vends' (per extra, per target: the two ends read)."""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    levels = np.asarray(levels, np.float64)
    ok = ~(np.isnan(p) | np.isnan(t))
    with np.errstate(all='ignore'):
        x = np.log(p[ok])
        tv = t[ok]
        th = theta_of(x, tv)
    ex = [np.asarray(v, np.float64)[ok] for v in extras]
    n = len(levels)
    out = {'pressure': np.full(n, NAN), 'temperature': np.full(n, NAN), 'vars': [np.full(n, NAN) for _ in ex], 'status': 0,
           'pairs': [], 'steps': np.zeros(n, int), 'theta': th, 'pair': np.full(n, -1), 'vends': [np.full((n, 2), NAN) for _ in ex]}
    for j, target in enumerate(levels):
        below = th <= target
        pairs = np.nonzero(below[:-1] != below[1:])[0] if th.size > 1 else np.zeros(0, int)
        out['pairs'].append(pairs)
        if pairs.size == 0:
            out['status'] |= ST_NO_LAYER
            continue
        k = int(pairs[0] if from_below else pairs[-1])
        out['pair'][j] = k
        with np.errstate(all='ignore'):
            xs, steps, conv = newton(target, x[k], tv[k], x[k + 1], tv[k + 1], max_iters, eps)
        out['steps'][j] = steps
        if not conv:
            out['status'] |= ST_NOT_CONVERGED
            continue
        out['pressure'][j] = np.exp(xs)
        out['temperature'][j] = target * np.exp(-KAPPA * (LN1000 - xs))
        for i, v in enumerate(ex):
            out['vars'][i][j] = v[k] + (v[k + 1] - v[k]) * (target - th[k]) / (th[k + 1] - th[k])
            out['vends'][i][j] = v[k], v[k + 1]
    return out


def grid(p, t, levels, extras=(), **kw):
    """column() over the columns of (nlev, ncol) arrays: 'pressure', 'temperature' (nlevel, ncol), 'vars' (a list of such),
    'status' (ncol) and 'columns', the per-column dicts."""
    ncol = p.shape[1]
    cols = [column(p[:, c], t[:, c], levels, [v[:, c] for v in extras], **kw) for c in range(ncol)]
    return {'pressure': np.stack([r['pressure'] for r in cols], 1), 'temperature': np.stack([r['temperature'] for r in cols], 1),
            'vars': [np.stack([r['vars'][i] for r in cols], 1) for i in range(len(extras))],
            'vscale': [np.stack([np.max(np.abs(r['vends'][i]), axis=1) for r in cols], 1) for i in range(len(extras))],
            'status': np.array([r['status'] for r in cols], np.int32), 'columns': cols}


def tie_column(col, levels, rel=1e-9):
    """Some target lies within rel * theta* of one of the column's level thetas: the bracket may differ by the last bit of exp."""
    th = col['theta']
    return bool(th.size) and any(np.any(np.abs(th - target) <= rel * target) for target in levels)
