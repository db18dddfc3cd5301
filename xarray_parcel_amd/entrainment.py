"""
Entraining CAPE (Peters, Chavas, Su, Morrison and Coffer 2023) on DataArrays: the buoyancy-dilution potential NCAPE of every
column, the per-point formula, and the chain from the sounding grid to ECAPE, through libxparcel (numpy_api.ncape,
ecape_from_ncape, ecape).  The reference has no counterparts, so this lives next to the mirror (parcel_functions.py) rather
than in it, and is built from the mirror's plumbing, as kinematics.py and downdraft.py.
"""
from . import numpy_api as _api
from .parcel_functions import VERT, _Grid, _device

_CAPE = 'J kg$^{-1}$'
_WIND = 'm s$^{-1}$'
_ATTRS = {
    'ecape': {'long_name': 'Entraining convective available potential energy', 'units': _CAPE},
    'ecape_a': {'long_name': 'Entraining CAPE plus the kinetic energy of the storm-relative inflow', 'units': _CAPE},
    'psi': {'long_name': 'Entrainment parameter of entraining CAPE', 'units': '1'},
    'ncape': {'long_name': 'Buoyancy-dilution potential (NCAPE) between the LFC and the EL', 'units': _CAPE},
    'cape': {'long_name': 'Convective available potential energy', 'units': _CAPE},
    'cin': {'long_name': 'Convective inhibition', 'units': _CAPE},
    'lfc_height': {'long_name': 'Level of free convection height above the lowest level', 'units': 'm'},
    'el_height': {'long_name': 'Equilibrium level height above the lowest level', 'units': 'm'},
    'sr_u': {'long_name': 'Storm-relative 0-1 km pressure-weighted mean wind, u component', 'units': _WIND},
    'sr_v': {'long_name': 'Storm-relative 0-1 km pressure-weighted mean wind, v component', 'units': _WIND},
    'status': {'long_name': 'Status bits'},
}
_NCAPE = ('ncape', 'lfc_height', 'el_height', 'status')
_ECAPE = ('ecape', 'ecape_a', 'psi')
_CHAIN = _ECAPE + ('ncape', 'cape', 'cin', 'lfc_height', 'el_height', 'sr_u', 'sr_v', 'status')


def ncape(pressure, temperature, dewpoint, height, lfc_pressure, el_pressure, vert_dim=VERT):
    """NCAPE [J/kg] of every column between lfc_pressure and el_pressure [hPa; DataArrays on the horizontal dims, as the CAPE
    / CIN functions return them], from pressure [hPa], temperature, dewpoint [K] and height [m] on one vertical.  Returns a
    Dataset on the horizontal dims: ncape, lfc_height and el_height [m above the lowest valid level] and the status bits.
    A column without an LFC has ncape 0; one whose EL is not above its LFC is NaN."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.ncape, g.values(pressure), g.values(temperature), g.values(dewpoint), g.values(height),
                  g.per_col(lfc_pressure), g.per_col(el_pressure))
    return g.dataset(res, _NCAPE, _ATTRS.get)


def ecape_from_ncape(cape, ncape, el_height, sr_u, sr_v):
    """Entraining CAPE per point from cape, ncape [J/kg], el_height [m above the lowest valid level] and the storm-relative
    0-1 km mean wind sr_u, sr_v [m/s].  Returns a Dataset of ecape, ecape_a (with the inflow's kinetic energy) and psi."""
    g = _Grid(cape, None)
    res = _device(_api.ecape_from_ncape, *(g.values(x) for x in (cape, ncape, el_height, sr_u, sr_v)))
    return g.dataset(res, _ECAPE, _ATTRS.get)


def ecape(pressure, temperature, dewpoint, height, u, v, vert_dim=VERT, parcel='most_unstable', depth=None, storm='right',
          storm_u=None, storm_v=None, moist=None, **cape_cin_options):
    """Entraining CAPE of every column from the sounding grid: CAPE / CIN of `parcel`, NCAPE between its LFC and EL, the
    Bunkers storm motion (`storm`: 'right', 'left' or 'mean'; or storm_u / storm_v, scalars or DataArrays on the horizontal
    dims), the 0-1 km pressure-weighted mean wind relative to it, and the formula -- numpy_api.ecape has the chain.  Returns a
    Dataset on the horizontal dims: ecape, ecape_a, psi, ncape, cape, cin, lfc_height, el_height, sr_u, sr_v and status."""
    g = _Grid(pressure, vert_dim)
    res = _device(_api.ecape, *(g.values(x) for x in (pressure, temperature, dewpoint, height, u, v)), parcel=parcel,
                  depth=depth, storm=storm, storm_u=g.per_col(storm_u), storm_v=g.per_col(storm_v), moist=moist,
                  **cape_cin_options)
    return g.dataset(res, _CHAIN, _ATTRS.get)
