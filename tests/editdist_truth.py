"""The truth the edit-distance tests hold the kernels to, in plain Python: the recursion on tuples
(cost, sub, del, ins) that Python compares lexicographically, the enumeration of every alignment
that pins it, the unit sequences of a path, the route formula of include/beer_hip.h restated, and
minimum-Bayes-risk selection in numpy's long double."""

import numpy as np

EINVAL = -100000
OPS, ROW_LDS, ROW_WS = 0x100, 0x1000, 0x2000
MAX_LEN, MAX_LEN_OPS = 1 << 30, (1 << 21) - 1
ROW_BYTES = 16 * 1024


# a step adds its vector to a cell (cost, sub, del, ins)
def _sub(c):
    return (c[0] + 1, c[1] + 1, c[2], c[3])


def _del(c):
    return (c[0] + 1, c[1], c[2] + 1, c[3])


def _ins(c):
    return (c[0] + 1, c[1], c[2], c[3] + 1)


def edit_ops(a, b):
    '''(cost, sub, del, ins) of turning `a` into `b`: the smallest tuple over all alignments.  A
    deletion consumes a symbol of `a` alone, an insertion a symbol of `b` alone.'''
    a, b = list(a), list(b)
    row = [(0, 0, 0, 0)]
    for _ in b:
        row.append(_ins(row[-1]))
    for x in a:
        new = [_del(row[0])]
        for j, y in enumerate(b, start=1):
            new.append(min(row[j - 1] if x == y else _sub(row[j - 1]), _del(row[j]),
                           _ins(new[j - 1])))
        row = new
    return row[-1]


def distance(a, b):
    return edit_ops(a, b)[0]


def enumerated(a, b):
    'The smallest (cost, sub, del, ins) over EVERY alignment of `a` and `b`, one by one.'
    a, b = list(a), list(b)
    best = [None]

    def walk(i, j, cell):
        if i == len(a) and j == len(b):
            if best[0] is None or cell < best[0]:
                best[0] = cell
            return
        if i < len(a) and j < len(b):
            walk(i + 1, j + 1, cell if a[i] == b[j] else _sub(cell))
        if i < len(a):
            walk(i + 1, j, _del(cell))
        if j < len(b):
            walk(i, j + 1, _ins(cell))

    walk(0, 0, (0, 0, 0, 0))
    return best[0]


def route_formula(max_short, max_long, want_ops):
    'beer_edit_distance_route as the header states it.'
    if max_short < 0 or max_long < max_short:
        return EINVAL
    if max_long > (MAX_LEN_OPS if want_ops else MAX_LEN):
        return EINVAL
    team = 8 if max_short <= 8 else (16 if max_short <= 16 else (32 if max_short <= 32 else 64))
    route = team | (OPS if want_ops else 0)
    if max_short > 64:
        route |= ROW_LDS if (max_long + 1) * (8 if want_ops else 4) <= ROW_BYTES else ROW_WS
    return route


def unit_sequence(path, unit_of_pdf):
    '''(units, per-frame units) of a pdf-id path, or the kernel's code: 0 units for an empty
    path, -1 for a path that begins with a negative symbol, -2 for a pdf outside the table or a
    first pdf that begins no unit.'''
    path = [int(p) for p in path]
    if not path:
        return [], []
    if path[0] < 0:
        return -1, -1
    if any(p < 0 or p >= len(unit_of_pdf) for p in path) or unit_of_pdf[path[0]] < 0:
        return -2, -2
    units, frames = [], []
    for t, p in enumerate(path):
        if t == 0 or (p != path[t - 1] and unit_of_pdf[p] >= 0):
            units.append(int(unit_of_pdf[p]))
        frames.append(units[-1])
    return units, frames


def mbr(seqs, weights):
    '''(risk, lowest) of hypotheses `seqs` (None: absent) under `weights` (unnormalised, any for
    an absent one): risk[i] = sum_j w_j d(i, j) / sum_j w_j in long double, inf for an absent
    hypothesis; `lowest` the smallest risk.'''
    n = len(seqs)
    w = np.asarray([0. if s is None else float(x) for s, x in zip(seqs, weights)],
                   dtype=np.longdouble)
    w = w / w.sum() if w.sum() > 0 else w
    risk = np.full(n, np.inf, dtype=np.longdouble)
    for i, a in enumerate(seqs):
        if a is None:
            continue
        risk[i] = sum(w[j] * distance(a, b) for j, b in enumerate(seqs) if b is not None)
    return risk, risk.min() if n else np.inf
