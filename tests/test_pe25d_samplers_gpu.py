"""What the four sampled diagnostics of GCM_PE25D share -- the zonal-mean climatology, the pressure-level climatology, the
zonal wavenumber spectra and the pressure-level maps -- and no other test pins: the text gcm_last_error holds behind a
refused call, and the two counters of a registration (steps since it, samples in the sums).  One small fp64 handle per
case, the smallest shape tests/test_pe25d_spectra_gpu.py registers on; the numbers in the sums are the business of each
diagnostic's own test file."""
import ctypes as C

import numpy as np
import pytest

import gpu_setups as su
from gpu_setups import g  # noqa: F401  (the fixture)
import pe25d_inputs as inp

pytestmark = pytest.mark.gpu

SHAPE = (6, 10, 3)              # (H, W, L)
DT = 120.0
PLEV = np.array([70000.0, 40000.0])
MMAX = 3
# name in the entry points: the "what" of "no ... registered", the arguments of gcm_set_<name> behind `every`, the names
# of gcm_put_<name>'s sum arrays as its message spells them, and the query that needs a registration besides
SAMPLERS = {
    "climate": ("climatology", (), "m3 and m2 are", None),
    "plev_climate": ("pressure-level climatology", (PLEV.size, PLEV.ctypes.data_as(C.POINTER(C.c_double))), "s is",
                     "gcm_plev_climate_levels"),
    "spectra": ("spectra", (MMAX,), "s is", "gcm_spectra_mmax"),
    "plev_maps": ("pressure-level maps", (PLEV.size, PLEV.ctypes.data_as(C.POINTER(C.c_double))), "s and s2 are",
                  "gcm_plev_maps_levels"),
}
NAMES = tuple(SAMPLERS)         # in the order a step samples


def handle(g):
    geom = su.geom_of(*SHAPE)
    return su.single(g, geom, inp.state_of(geom))


def fn(g, pattern, name):
    return getattr(g._lib.lib, "gcm_" + pattern % name)


def register(g, c, name, every):
    """gcm_set_<name> through the C ABI -> its return code"""
    return fn(g, "set_%s", name)(c._h, every, *SAMPLERS[name][1])


def sums(c, name):
    """(n, the one or two sum arrays) as Core.<name>_sums returns them"""
    return getattr(c, name + "_sums")()


def put(g, c, name, arrays, n):
    dp = g._lib._dp
    return fn(g, "put_%s", name)(c._h, *[None if a is None else a.ctypes.data_as(dp) for a in arrays], n)


def last_error(g, c):
    return g._lib.lib.gcm_last_error(c._h).decode()


def assert_unchanged(c, name, was):
    now = sums(c, name)
    assert now[0] == was[0], (name, now[0], was[0])
    for a, b in zip(now[1:], was[1:]):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("name", NAMES)
def test_without_a_registration_every_call_says_which_one_is_missing(g, name):
    L_ = g._lib
    what, _, required, query = SAMPLERS[name]
    c = handle(g)
    nsums = 2 if " and " in required else 1
    calls = {"gcm_%s_sample" % name: lambda: fn(g, "%s_sample", name)(c._h),
             "gcm_%s_reset" % name: lambda: fn(g, "%s_reset", name)(c._h),
             "gcm_get_%s" % name: lambda: fn(g, "get_%s", name)(c._h, *([None] * nsums), None),
             "gcm_put_%s" % name: lambda: put(g, c, name, [None] * nsums, 0)}
    if query == "gcm_spectra_mmax":
        calls[query] = lambda: L_.lib.gcm_spectra_mmax(c._h)
    elif query:
        calls[query] = lambda: getattr(L_.lib, query)(c._h, None, 0)
    for entry, call in calls.items():
        assert call() == L_.ERR_STATE, entry
        assert last_error(g, c) == "%s: no %s registered (gcm_set_%s)" % (entry, what, name)
    # ... and again behind a registration that was taken back
    assert register(g, c, name, 2) == L_.OK and register(g, c, name, 0) == L_.OK
    for entry, call in calls.items():
        assert call() == L_.ERR_STATE, entry
        assert last_error(g, c) == "%s: no %s registered (gcm_set_%s)" % (entry, what, name)
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_refused_put_or_set_says_why_and_changes_nothing(g, name):
    L_ = g._lib
    required = SAMPLERS[name][2]
    c = handle(g)
    assert register(g, c, name, 1) == L_.OK
    c.step(2, DT)
    was = sums(c, name)
    arrays = list(was[1:])
    assert was[0] == 2 and arrays[0].any()
    message = "gcm_put_%s: %s required, nsamples must be >= 0" % (name, required)
    refused = [([None if k == gone else a for k, a in enumerate(arrays)], 1) for gone in range(len(arrays))] + [(arrays, -1)]
    for given, n in refused:
        assert put(g, c, name, given, n) == L_.ERR_ARG
        assert last_error(g, c) == message
        assert_unchanged(c, name, was)
    assert register(g, c, name, -1) == L_.ERR_ARG
    assert last_error(g, c) == "gcm_set_%s: every must be >= 0" % name
    assert getattr(c, name + "_every") == 1
    assert_unchanged(c, name, was)
    # the registration's step counter is untouched too: the next step samples
    c.step(1, DT)
    assert sums(c, name)[0] == 3
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_the_step_counter_and_the_sample_count(g, name):
    L_ = g._lib
    c = handle(g)
    assert register(g, c, name, 3) == L_.OK
    c.step(7, DT)
    assert sums(c, name)[0] == 2                      # steps 3 and 6
    # an explicit sample counts as a sample, not as a step: the next automatic one still falls on step 9
    assert fn(g, "%s_sample", name)(c._h) == L_.OK
    assert sums(c, name)[0] == 3
    c.step(1, DT)
    assert sums(c, name)[0] == 3                      # step 8
    c.step(1, DT)
    assert sums(c, name)[0] == 4                      # step 9
    c.step(1, DT)
    assert sums(c, name)[0] == 4                      # step 10
    # registering again restarts both counters: steps 11 and 12 of the handle are steps 1 and 2 of the registration
    assert register(g, c, name, 3) == L_.OK
    n, first = sums(c, name)[:2]
    assert n == 0 and not first.any()
    c.step(2, DT)
    assert sums(c, name)[0] == 0
    c.step(1, DT)
    assert sums(c, name)[0] == 1
    c.close()


def test_four_registrations_count_the_steps_each_on_its_own(g):
    c = handle(g)
    for every, name in enumerate(NAMES, start=1):
        assert register(g, c, name, every) == g._lib.OK
    c.step(12, DT)
    assert [sums(c, name)[0] for name in NAMES] == [12, 6, 4, 3]
    assert [getattr(c, name + "_every") for name in NAMES] == [1, 2, 3, 4]
    c.close()
