"""Host side of contact coupling over the models of an ensemble (``Context.models_coupling`` /
``EnsembleComplex.run_coupling``): which contacts form and break together, where the persistence tables say how often a
contact exists, the lifetimes how long it lasts and the similarity matrix which models resemble each other.

Inputs: F >= 2 resident models and the bags of a pass over them.  A *row* is a contact — a topology atom pair or a topology
residue pair —, *present* in a model when a participating record of it has one of the named planes (``similarity.planes``).
The *features* are the rows present in ``min_count`` ... ``max_count`` models, 1 <= min_count <= max_count <= F - 1, numbered
in ascending (a, b).  For two features u < v with n_u and n_v models and n11 models in common,

    d = F n11 - n_u n_v,      phi = d / sqrt(n_u (F - n_u) n_v (F - n_v)),

and the device keeps the pair when ``1024 d^2 >= q n_u (F - n_u) n_v (F - n_v)``: phi^2 >= q / 1024, a comparison of
integers (``phi2_q`` turns a threshold on \\|phi\\| into q).  Anti-correlated pairs are kept like correlated ones.

The result is two tables, dicts of NumPy columns (``tables.COUPLING_FEATURES`` / ``tables.COUPLING_PAIRS``):

    features    a, b int32 (atom or residue ids of the topology), count uint32 (n)      ascending (a, b)
    pairs       u, v uint32 (feature numbers, u < v), n11 uint32                        ascending (u, v)

The chunks of a streamed trajectory cannot be merged: the threshold is not additive over chunks.

Everything here is NumPy on the host: no GPU is needed to derive phi, group or export.
"""
import csv
import math
import os
from fractions import Fraction

import numpy as np

from . import tables

BY_RESIDUE = 1             # ARP_COUPLE_BY_RESIDUE
MAX_FEATURES = 65536       # ARP_COUPLE_MAX_FEATURES
Q_ONE = 1024               # phi^2 = 1
LEVELS = ('atom', 'residue')


def empty():
    """A result without features and pairs."""
    return tables.empty(tables.COUPLING_FEATURES), tables.empty(tables.COUPLING_PAIRS)


def _exact(x):
    """The number a float is written as — 0.05 is 1 / 20, not the binary fraction a little above it —, as a Fraction."""
    return Fraction(repr(float(x)))


def phi2_q(min_abs_phi):
    """``(q, effective)``: q = ceil(phi^2 * 1024) clipped to 1 ... 1024, the launch argument for "keep \\|phi\\| >=
    min_abs_phi", and the threshold on \\|phi\\| that q stands for, sqrt(q / 1024) — never below the one asked for unless that
    was above 1.  The square is taken exactly, of the decimal number the float is written as, so a threshold that is a multiple
    of 1 / 32 is met exactly."""
    x = float(min_abs_phi)
    if not 0.0 <= x < math.inf:
        raise ValueError('coupling.phi2_q: min_abs_phi must be a finite number, not negative')
    q = min(max(math.ceil(_exact(x) ** 2 * Q_ONE), 1), Q_ONE)
    return q, math.sqrt(q / Q_ONE)


def counts(occupancy_min, occupancy_max, n_models):
    """The band of model counts for a band of occupancies: ceil(min F) and floor(max F), each clipped to 1 ... F - 1."""
    F = int(n_models)
    if F < 2:
        raise ValueError('coupling.counts: coupling needs at least 2 models')
    lo, hi = math.ceil(_exact(occupancy_min) * F), math.floor(_exact(occupancy_max) * F)
    return min(max(lo, 1), F - 1), min(max(hi, 1), F - 1)


def _columns(features, pairs, n_models):
    F = int(n_models)
    n = features['count'].astype(np.int64)
    nu, nv, n11 = n[pairs['u'].astype(np.int64)], n[pairs['v'].astype(np.int64)], pairs['n11'].astype(np.int64)
    return F, nu, nv, n11


def covariance(features, pairs, n_models):
    """d = F n11 - n_u n_v of every pair, int64 [P]: its sign is the sign of phi."""
    F, nu, nv, n11 = _columns(features, pairs, n_models)
    return F * n11 - nu * nv


def phi(features, pairs, n_models):
    """The phi coefficient of every pair, float64 [P]: d / sqrt(n_u (F - n_u) n_v (F - n_v)) from the integers (the product
    stays below 2^44, exact in float64)."""
    F, nu, nv, n11 = _columns(features, pairs, n_models)
    return (F * n11 - nu * nv).astype(np.float64) / np.sqrt((nu * (F - nu) * nv * (F - nv)).astype(np.float64))


def jaccard(features, pairs):
    """n11 / (n_u + n_v - n11) of every pair, float64 [P] (a feature is present in at least one model: never 0 / 0)."""
    _, nu, nv, n11 = _columns(features, pairs, 0)
    return n11.astype(np.float64) / (nu + nv - n11).astype(np.float64)


def groups(features, pairs, positive_only=True, n_models=None):
    """The sets of contacts that switch together: the connected components of the graph whose nodes are the features and
    whose edges are the kept pairs — with ``positive_only`` the correlated ones (d > 0; ``n_models`` is needed for the sign).
    Returns a list of int64 arrays of feature numbers, each ascending, only components of two features or more, in the order
    of their smallest feature.  A host union-find."""
    K = len(features['a'])
    u, v = pairs['u'].astype(np.int64), pairs['v'].astype(np.int64)
    if positive_only:
        if n_models is None:
            raise ValueError('coupling.groups: positive_only needs n_models (the sign of a pair is that of F n11 - n_u n_v)')
        keep = covariance(features, pairs, n_models) > 0
        u, v = u[keep], v[keep]
    parent = np.arange(K, dtype=np.int64)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    for x, y in zip(u.tolist(), v.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)      # (the root is the smallest member)
    roots = np.array([find(x) for x in range(K)], np.int64)
    order = np.argsort(roots, kind='stable')
    out = []
    for members in np.split(order, np.nonzero(np.diff(roots[order]))[0] + 1) if K else []:
        if len(members) > 1:
            out.append(members.astype(np.int64))
    return out


def _labels(pc, level, component_types):
    from .core import export
    if level not in LEVELS:
        raise ValueError(f"coupling: level must be 'atom' or 'residue', not {level!r}")
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    return lab, (lab.atom_macro if level == 'atom' else lambda r: lab.res_macro[r])


def to_records(pc, features, pairs, n_models, level='atom', component_types=None):
    """The pairs as a list of dicts for JSON: 'bgn' / 'end' are the two contacts, each {'bgn', 'end', 'n_models'} with the
    labels the other tables use; the counts are plain ints, 'phi' and 'jaccard' floats."""
    lab, _ = _labels(pc, level, component_types)
    what = lab.atom_dict if level == 'atom' else (lambda r: lab.res_macro[r])
    ph, ja = phi(features, pairs, n_models), jaccard(features, pairs)

    def contact(k):
        return {'bgn': what(int(features['a'][k])), 'end': what(int(features['b'][k])), 'n_models': int(features['count'][k])}
    return [{'bgn': contact(int(pairs['u'][r])), 'end': contact(int(pairs['v'][r])), 'type': 'contact-coupling',
             'n_both': int(pairs['n11'][r]), 'phi': float(ph[r]), 'jaccard': float(ja[r])} for r in range(len(pairs['u']))]


CSV_HEADER = ['u_bgn', 'u_end', 'v_bgn', 'v_end', 'n_u', 'n_v', 'n11', 'phi']


def write_csv(path, features, pairs, pc, n_models, level='atom', component_types=None):
    """One row per kept pair: the two contacts by the labels the other CSV tables use ('A/508/O', or 'A/508' at residue
    level), n_u, n_v, n11 and phi (the shortest text that gives the float64 back)."""
    _, name = _labels(pc, level, component_types)
    ph = phi(features, pairs, n_models)
    a, b, n = features['a'], features['b'], features['count']
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r in range(len(pairs['u'])):
            u, v = int(pairs['u'][r]), int(pairs['v'][r])
            w.writerow([name(int(a[u])), name(int(b[u])), name(int(a[v])), name(int(b[v])), int(n[u]), int(n[v]), int(pairs['n11'][r]),
                        repr(float(ph[r]))])


def write_coupling(wd, sid, features, pairs, pc, n_models, level='atom', component_types=None):
    """'<id>.coupling' in ``wd``."""
    path = os.path.join(wd, sid + '.coupling')
    write_csv(path, features, pairs, pc, n_models, level, component_types)
    return path
