"""XP_HUM_RELATIVE and XP_HUM_MIXING_RATIO restated in NumPy from the words of include/xparcel.h, on oracle/thermo.py's
saturation_vapor_pressure, vapor_pressure and dewpoint -- not from the kernel (csrc/xp_humidity.hpp):

    relative:      e = m * e_s(T)            m: relative humidity over liquid water as a fraction
    mixing ratio:  e = p * m / (eps + m)     m: kg/kg
    both:          D = 273.15 + 243.5 v / (17.67 - v), v = ln(e / 6.112), in double;
                   D is NaN unless m > 0 by plain comparison; IEEE arithmetic decides everything else;
                   D is stored in the views' dtype, rounded once.
"""
import numpy as np

from oracle import thermo as O

RELATIVE, MIXING_RATIO = 'relative', 'mixing_ratio'
KINDS = (RELATIVE, MIXING_RATIO)
ENUM = {'dewpoint': 0, 'specific': 1, RELATIVE: 2, MIXING_RATIO: 3}        # the header's XP_HUM_*


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def dewpoint64(kind, pressure, temperature, moisture):
    """D in float64, before it is stored.  pressure: on the grid, or the nlev isobars of an (nlev, ...) grid."""
    assert kind in KINDS
    m = _f64(moisture)
    with np.errstate(all='ignore'):
        if kind == RELATIVE:
            e = m * O.saturation_vapor_pressure(_f64(temperature))
        else:
            p = _f64(pressure)
            if p.ndim == 1 and m.ndim > 1:
                p = p.reshape((-1,) + (1,) * (m.ndim - 1))
            e = O.vapor_pressure(p, m)
        d = O.dewpoint(e)
        return np.where(m > 0, d, np.nan)


def dewpoint(kind, pressure, temperature, moisture, dtype=None):
    """D as the call stores it: rounded once to `dtype` (default: the moisture's)."""
    dtype = np.asarray(moisture).dtype if dtype is None else dtype
    return np.ascontiguousarray(dewpoint64(kind, pressure, temperature, moisture).astype(dtype))


def relative_humidity(temperature, dewpoint_):
    """The fraction with which dewpoint() gives `dewpoint_` back: e_s(Td) / e_s(T)."""
    with np.errstate(all='ignore'):
        return O.saturation_vapor_pressure(_f64(dewpoint_)) / O.saturation_vapor_pressure(_f64(temperature))


def mixing_ratio(pressure, dewpoint_):
    """The mixing ratio [kg/kg] with which dewpoint() gives `dewpoint_` back: eps e / (p - e), e = e_s(Td)."""
    with np.errstate(all='ignore'):
        return O.mixing_ratio(O.saturation_vapor_pressure(_f64(dewpoint_)), _f64(pressure))
