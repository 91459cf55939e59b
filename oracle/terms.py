"""Named term hooks of the oracle's time steps -- TEST INSTRUMENTATION ONLY.

A step function that takes `_terms` evaluates each of its named terms through `term()`.  `_terms` maps a
term name to a multiplier (0 drops the term, 1.01 scales it by 1 %) or to the name of a substitute the step
offers (e.g. "visc_v_of_v").  `_terms=None`, the default, leaves every expression as written, so the default
path stays bit-identical to the reference's arithmetic (tests/test_oracle_golden.py).  Each model lists its
names in TERMS; tests/test_term_visibility_cpu.py uses them to show that the GPU parity cases can see every
term.
"""


def check(terms, names):
    """refuse a name the step does not have (a typo would otherwise leave the step untouched)"""
    if terms:
        bad = set(terms) - set(names)
        if bad:
            raise KeyError("unknown term(s) %s; known: %s" % (sorted(bad), ", ".join(names)))


def term(terms, name, x, **subs):
    """the term `name` whose value as written is x: unchanged, times terms[name], or the substitute
    subs[terms[name]]() when that is a string"""
    if not terms or name not in terms:
        return x
    k = terms[name]
    if isinstance(k, str):
        return subs[k]()
    return x * k
