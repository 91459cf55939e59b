"""Ensembles of the 2-D drop-ins: the same call surface as matsuno_c_grid.py / matsumo_temp.py on
arrays with a leading member axis, (M, H, W).  The members share the grid, dx, the model, the tracer
scheme and dt; only the state differs.  One handle carries all M (gcm_config.members), and one launch
per step advances all of them -- M small grids fill the chip where one leaves most of it idle.

    u, v, p = ensemble.matsumo_scheme(u, v, p, dx, dt)              # u.shape == (M, H, W)
    u, v, p, t = ensemble.matsumo_temp_scheme(u, v, p, t, dx, dt)
    u, v, p, t, q = ensemble.matsumo_temp_scheme(u, v, p, t, dx, dt, q=q, tracer="van_leer")
    u, v, p = ensemble.run(u, v, p, dx, dt, steps, callback=cb, every=10)
    cn = ensemble.courant_numbers(p, u, dx, dt)                      # (M,)

Every function takes a keyword-only dtype="f64"; "f32" runs a float32 handle (the state rounded to
float32 on the way in, float64 arrays of float32 values back) that holds twice the members per byte.
"""
import numpy as np

from . import _lib
from .core import Core, as_f64, check_dtype
from .matsumo_temp import TRACERS
from .units import strip, scalar, attach

_cache = {}


def _core(model, shape, dx, **kw):
    key = (model, shape, dx, tuple(sorted(kw.items())))
    c = _cache.get(key)
    if c is None:
        if len(_cache) > 8:
            _cache.popitem()[1].close()
        c = _cache[key] = Core(model, shape[2], shape[1], dx=dx, members=shape[0], **kw)
    return c


def _in(c, a):
    """a (M, H, W) array as the handle's set_state takes it: one member's handle takes (H, W)"""
    return None if a is None else (a[0] if c.members == 1 else a)


def _out(c, a):
    """the handle's get_state array with the member axis, (M, H, W)"""
    return None if a is None else a.reshape((c.members, c.H, c.W))


def _members(named):
    """[(name, array or Quantity)] -> ([float64 (M, H, W) magnitudes], [units]); ValueError unless every
    array is 3-D with the first one's shape"""
    mags, units = [], []
    shape = None
    for name, x in named:
        m, un = strip(x)
        m = as_f64(m, shape, name)
        if shape is None:
            if m.ndim != 3 or min(m.shape) < 1:
                raise ValueError("%s must be 3-D [member, j, i], got shape %s" % (name, m.shape))
            shape = m.shape
        mags.append(m)
        units.append(un)
    return mags, units


def _tracer(q, tracer):
    if q is None:
        return _lib.TRACER_NONE
    if tracer not in TRACERS or TRACERS[tracer] == _lib.TRACER_NONE:
        raise ValueError("a tracer q needs tracer='upwind' or 'van_leer', got %r" % (tracer,))
    return TRACERS[tracer]


def matsumo_scheme(u, v, p, dx, dt, *, dtype="f64"):
    """matsuno_c_grid.matsumo_scheme on every member: one Matsuno step; takes and returns (u, v, p), each
    (M, H, W).  Inputs are not modified."""
    check_dtype(dtype)
    (um, vm, pm), (uu, vu, pu) = _members((("u", u), ("v", v), ("p", p)))
    c = _core(_lib.SW2D, um.shape, scalar(dx), dtype=dtype)
    c.set_state(p=_in(c, pm), u=_in(c, um), v=_in(c, vm))
    c.step(1, scalar(dt))
    pn, un, vn, _, _ = (_out(c, x) for x in c.get_state((_lib.P, _lib.U, _lib.V)))
    return attach(un, uu), attach(vn, vu), attach(pn, pu)


def matsumo_temp_scheme(u, v, p, t, dx, dt, q=None, tracer="van_leer", *, dtype="f64"):
    """matsumo_temp.matsumo_scheme on every member -> (u, v, p, t); with a tracer q (M, H, W) also
    advected by the time-n winds (matsumo_temp.matsumo_scheme_with_tracer) -> (u, v, p, t, q)."""
    check_dtype(dtype)
    named = [("u", u), ("v", v), ("p", p), ("t", t)] + ([("q", q)] if q is not None else [])
    mags, units = _members(named)
    tr = _tracer(q, tracer)
    c = _core(_lib.SW2D_TEMP, mags[0].shape, scalar(dx), tracer=tr, dtype=dtype)
    um, vm, pm, tm = mags[:4]
    c.set_state(p=_in(c, pm), u=_in(c, um), v=_in(c, vm), t=_in(c, tm), q=_in(c, mags[4]) if q is not None else None)
    c.step(1, scalar(dt))
    pn, un, vn, tn, qn = (_out(c, x) for x in c.get_state())
    out = [attach(un, units[0]), attach(vn, units[1]), attach(pn, units[2]), attach(tn, units[3])]
    if q is not None:
        out.append(attach(qn, units[4]))
    return tuple(out)


def run(u, v, p, dx, dt, steps, t=None, q=None, tracer="van_leer", callback=None, every=1, *, dtype="f64"):
    """Device-resident driver loop over all members (matsuno_c_grid.run with a member axis; with t,
    GCM_SW2D_TEMP, and with q its tracer): `steps` Matsuno steps, the state stays in HBM between them.
    callback(i, u, v, p[, t[, q]]) every `every` steps with (M, H, W) arrays.  The loop ends early once
    every member carries a NaN in u (a member that blows up does not stop the others).
    -> (u, v, p[, t[, q]])"""
    check_dtype(dtype)
    named = [("u", u), ("v", v), ("p", p)]
    if t is not None:
        named.append(("t", t))
    if q is not None:
        if t is None:
            raise ValueError("a tracer q needs the temperature model (t)")
        named.append(("q", q))
    mags, units = _members(named)
    tr = _tracer(q, tracer)
    M, H, W = mags[0].shape
    model = _lib.SW2D if t is None else _lib.SW2D_TEMP
    c = Core(model, W, H, dx=scalar(dx), tracer=tr, members=M, dtype=dtype)
    fields = (_lib.U, _lib.V, _lib.P, _lib.T, _lib.Q)[:len(named)]

    def state():
        got = c.get_state(fields)
        return tuple(attach(_out(c, got[f]), un) for f, un in zip(fields, units))

    try:
        c.set_state(**{k: _in(c, a) for (k, _), a in zip(named, mags)})
        done = 0
        while done < steps:
            n = min(every, steps - done) if callback else steps - done
            c.step(n, scalar(dt))
            done += n
            if callback:
                callback(done, *state())
            if c.diag_members(_lib.DIAG_ANY_NAN).all():
                break
        return state()
    finally:
        c.close()


def courant_numbers(p, u, dx, dt, *, dtype="f64"):
    """matsuno_c_grid.courant_number of every member, (M,): (max u + sqrt(mean p g)) dt / dx by device
    reductions (one launch and one synchronisation per reduction for all members)."""
    check_dtype(dtype)
    (pm, um), _ = _members((("p", p), ("u", u)))
    c = _core(_lib.SW2D, um.shape, scalar(dx), dtype=dtype)
    c.set_state(p=_in(c, pm), u=_in(c, um), v=_in(c, np.zeros_like(um)))
    return (c.diag_members(_lib.DIAG_MAX_U) + np.sqrt(c.diag_members(_lib.DIAG_MEAN_P) * 9.8)) * scalar(dt) / scalar(dx)
