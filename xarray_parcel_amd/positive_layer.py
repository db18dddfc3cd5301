"""
CAPE / CIN of ONE positive layer on DataArrays.  A sounding with a capping inversion, elevated convection or a dry intrusion
has several separate positive areas; the reference's rule (lfc_el: the bottom LFC and the top EL) adds them all up, and
this module lets the caller say which one is meant (XP_OPT_LAYER_*, include/xparcel.h; numpy_api's positive_layer=): the
lowest layer, the highest, the deepest in ln p or the one with the most CAPE -- or, in MetPy's spelling, a which_lfc /
which_el pair.  The reference has no counterpart, so this lives next to the mirror (parcel_functions.py) rather than in
it, and is built from the mirror's plumbing, as max_cape.py and ground.py.
"""
from . import numpy_api as _api
from .parcel_functions import VERT, _Grid, _device, _moisture

_CAPE = 'J kg$^{-1}$'
_ATTRS = {
    'cape': {'long_name': 'Convective available potential energy of the chosen positive layer', 'units': _CAPE},
    'cin': {'long_name': 'Convective inhibition below the chosen positive layer', 'units': _CAPE},
    'lfc_pressure': {'long_name': 'Pressure of the bottom of the chosen positive layer (its LFC)', 'units': 'hPa'},
    'lfc_temperature': {'long_name': 'Parcel temperature at the bottom of the chosen positive layer', 'units': 'K'},
    'el_pressure': {'long_name': 'Pressure of the top of the chosen positive layer (its EL)', 'units': 'hPa'},
    'el_temperature': {'long_name': 'Parcel temperature at the top of the chosen positive layer', 'units': 'K'},
}
WANT = tuple(_ATTRS)


def cape_cin(pressure, temperature, dewpoint, parcel='surface', positive_layer=None, which_lfc=None, which_el=None,
             vert_dim=VERT, depth=None, ground=None, **kwargs):
    """CAPE, CIN, LFC and EL of one positive layer of the ascent of `parcel` ('surface', 'most_unstable', 'mixed_layer',
    'max_cape').  pressure [hPa], temperature, dewpoint [K] on the same dims with `vert_dim` among them.
    positive_layer: 'envelope' (the default: the reference's bottom LFC and top EL), 'lowest', 'highest', 'deepest' or
    'most_cape'; or MetPy's pair which_lfc= / which_el=: ('bottom', 'top'), ('bottom', 'bottom'), ('top', 'top'),
    ('wide', 'wide'), ('most_cape', 'most_cape') for the same five -- any other pair is a ValueError.
    ground=(surface_pressure, surface_temperature, surface_dewpoint): isobaric levels cut at the ground, as ground.py.
    Returns a Dataset of cape, cin, lfc_pressure, lfc_temperature, el_pressure, el_temperature per column.  kwargs: moist
    and the CAPE / CIN options of numpy_api.cape_cin_columns; among them humidity='relative' (`dewpoint` holds relative
    humidity as a fraction; percent is refused), 'mixing_ratio' or 'specific' [kg/kg]."""
    g = _Grid(temperature, vert_dim)
    if ground is not None:
        ground = tuple(g.values(x) for x in ground)
    res = _device(_api.cape_cin_columns, g.values(pressure), g.values(temperature), _moisture(g, dewpoint, kwargs),
                  parcel=parcel, depth=depth, ground=ground, want=WANT, positive_layer=positive_layer, which_lfc=which_lfc,
                  which_el=which_el, **kwargs)
    return g.dataset(res, attrs=_ATTRS.get)
