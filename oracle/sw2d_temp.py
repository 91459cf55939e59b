"""2-D shallow water + potential temperature + viscosity
(reference matsumo_temp.py, viscosity.py)."""
from .constants import Rd, Cp, G, mu_air
from .grid import ipj, imj, ijp, ijm
from .sw2d import (advection_of_velocity_u, advection_of_velocity_v,
                   geopotential_gradient_u, geopotential_gradient_v,
                   advection_of_geopotential)
from .terms import check, term

# named terms of matsumo_scheme (oracle/terms.py), each used in both Euler stages.  visc_u / visc_v are
# mu lap(u) / rho in the u / v equation; "visc_v_of_v" substitutes lap(v) in the v equation.
TERMS = ("adv_u", "pgf_u", "visc_u", "adv_v", "pgf_v", "visc_v", "adv_p", "adv_t")


def finite_laplacian_2d(q, dx):
    """viscosity.py:12-19 (add order as written)."""
    top = ijp(q) + ijm(q) + ipj(q) + imj(q) - 4 * q
    return top / (dx * dx)


def incompressible_viscosity_2d(u, mu, dx):
    """viscosity.py:22-25."""
    return mu * finite_laplacian_2d(u, dx)


def density_from(p, t):
    """matsumo_temp.py:13-19."""
    pressure_ratio = (100000.0 / p)
    temp = t / (pressure_ratio ** (Rd / Cp))
    return p / (Rd * temp)


def scaling(pa, t, dx):
    """matsumo_temp.py:28-30."""
    return pa * t * dx * dx


def unscaling(pb, tt, dx):
    """matsumo_temp.py:33-35."""
    return tt / (pb * dx * dx)


def geopotential_from(rho, p):
    """matsumo_temp.py:45-47."""
    return p / (G * rho)


def euler_stage(u, v, p, scaled_t, su, sv, sp, st, dx, dt, _terms=None):
    """One Euler stage of matsumo_temp.py:66-99: the tendencies of the state (su, sv, sp, st) applied to the
    base state (u, v, p) and to the base's scaled temperature.  Returns (u, v, p, t)."""
    T = _terms
    density = density_from(sp, st)
    geo = geopotential_from(density, sp)
    scaled_st = scaling(sp, st, dx)
    u_n = u - dt * (term(T, "adv_u", advection_of_velocity_u(su, sv, dx))
                    + term(T, "pgf_u", geopotential_gradient_u(geo, dx))
                    - term(T, "visc_u", incompressible_viscosity_2d(su, mu_air, dx) / density))
    v_n = v - dt * (term(T, "adv_v", advection_of_velocity_v(su, sv, dx))
                    + term(T, "pgf_v", geopotential_gradient_v(geo, dx))
                    - term(T, "visc_v", incompressible_viscosity_2d(su, mu_air, dx) / density,
                           visc_v_of_v=lambda: incompressible_viscosity_2d(sv, mu_air, dx) / density))
    p_n = p - dt * term(T, "adv_p", advection_of_geopotential(su, sv, sp, dx))
    tt = scaled_t - dt * term(T, "adv_t", advection_of_geopotential(su, sv, scaled_st, dx))
    return u_n, v_n, p_n, unscaling(p_n, tt, dx)


def predictor(u, v, p, t, dx, dt, _terms=None):
    """matsumo_temp.py:66-80: the predicted ("star") state (u*, v*, p*, t*)."""
    check(_terms, TERMS)
    return euler_stage(u, v, p, scaling(p, t, dx), u, v, p, t, dx, dt, _terms)


def matsumo_scheme(u, v, p, t, dx, dt, _terms=None):
    """matsumo_temp.py:66-99.  The v equation uses the viscosity of u
    (:75,:91) -- reproduced.  Takes and returns (u, v, p, t).  `_terms`: see
    oracle/terms.py (test instrumentation only)."""
    check(_terms, TERMS)
    scaled_t = scaling(p, t, dx)
    star = euler_stage(u, v, p, scaled_t, u, v, p, t, dx, dt, _terms)
    return euler_stage(u, v, p, scaled_t, *star, dx, dt, _terms)
