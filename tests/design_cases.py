"""The design cases of tests/golden/design.npz (make_golden_design.py holds the same table: callables cannot be stored), and the keys
of the golden arrays parsed back into (design name, n, [n_tries,] seed)."""
import re


def ppf_quadratic(u):
    return 2.0 * u * u - 1.0


DESIGN_ARGS = {
    "unit3": (3,),
    "box2": (2, (-1.0, 3.0)),
    "list3": ([(0.0, 1.0), (10.0, 20.0), (-5.0, -4.0)],),
    "ppf4": (4, ppf_quadratic),
    "mixed2": ([ppf_quadratic, (2.0, 2.5)],),
}
N_PARAMETERS = {"unit3": 3, "box2": 2, "list3": 3, "ppf4": 4, "mixed2": 2}


def oneshot_cases(g, tag):
    """[(key, name, n, seed)] of the seeded Monte-Carlo (tag "mc") or Latin-hypercube ("lhc") samples."""
    found = []
    for key in g.files:
        m = re.fullmatch(r"%s_([a-z0-9]+)_n(\d+)_seed(\d+)" % tag, key)
        if m:
            found.append((key, m.group(1), int(m.group(2)), int(m.group(3))))
    return sorted(found)


def maximin_cases(g):
    """[(key, name, n, n_tries, seed)] of the seeded maximin samples; g[key + "_mins"] holds the minimum distance of every try."""
    found = []
    for key in g.files:
        m = re.fullmatch(r"mm_([a-z0-9]+)_n(\d+)_t(\d+)_seed(\d+)", key)
        if m:
            found.append((key, m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return sorted(found)


MICE_CASES = ("c50", "c50s", "c400")
