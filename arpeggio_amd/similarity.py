"""Host side of the interaction-fingerprint similarity between the models of an ensemble (``Context.models_similarity`` /
``EnsembleComplex.run_similarity``): which models share their contacts.

The device delivers ``inter``, uint32 [F, F]: ``inter[f, g]`` = features present in model f and in model g, a feature being
(row, plane) — a row a topology atom pair (or, at residue level, a topology residue pair), a plane one of the 15 SIFt bits
(``config.SIFT_NAMES``: "an atom-atom record with that bit") or one of the five record classes (``tables.CLASSES``: "a record
of that class").  ``inter[f, f]`` is the feature count of model f.  From it follow the Tanimoto similarity, a distance for
clustering and the medoid.  Everything here is NumPy on the host: no GPU, no native library.
"""
import csv
import os

import numpy as np

from . import contact_filter, tables
from .core import config

N_PLANES = tables.N_BITS + len(tables.CLASSES)      # ARP_SIM_PLANES
CLASS_PLANE = tables.N_BITS                         # plane of class m: CLASS_PLANE + m
ATOM_PLANES = (1 << (CLASS_PLANE + 1)) - 1          # the planes that exist at atom level: the SIFt bits and 'atom_atom'
MAX_MODELS = 4096                                   # ARP_SIM_MAX_MODELS
BY_RESIDUE = 1                                      # ARP_SIM_BY_RESIDUE


def planes(contacts=None, classes=()):
    """The ``planes`` mask: the SIFt planes of the contacts named in ``contacts`` (``config.SIFT_NAMES``; ``None`` means
    every contact but bare proximity, ``contact_filter.SPECIFIC``'s; an empty list none) and the class planes named in
    ``classes`` (``tables.CLASSES``: 'atom_atom', 'atom_plane', ...).  An unknown name raises ``ValueError``, and so does a
    mask without any plane."""
    if contacts is None:
        m = contact_filter.SPECIFIC[0]
    else:
        m = 0
        for nm in ([contacts] if isinstance(contacts, str) else list(contacts)):
            if nm not in config.SIFT_NAMES[:tables.N_BITS]:
                raise ValueError(f'similarity.planes: unknown contact name {nm!r} (known: {", ".join(config.SIFT_NAMES[:tables.N_BITS])})')
            m |= 1 << config.SIFT_NAMES.index(nm)
    for nm in ([classes] if isinstance(classes, str) else list(classes)):
        if nm not in tables.CLASSES:
            raise ValueError(f'similarity.planes: unknown class name {nm!r} (known: {", ".join(tables.CLASSES)})')
        m |= 1 << (CLASS_PLANE + tables.CLASSES.index(nm))
    if not m:
        raise ValueError('similarity.planes: no plane named (a mask of 0 makes no feature)')
    return m


def _square(inter):
    a = np.asarray(inter)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError('similarity: inter must be a square matrix [F, F]')
    return a.astype(np.int64)


def counts(inter):
    """The feature count of every model: the diagonal, int64 [F]."""
    return np.diagonal(_square(inter)).copy()


def tanimoto(inter):
    """float64 [F, F]: I / (n_f + n_g - I); 1.0 where both models have no feature, and on the diagonal."""
    a = _square(inter)
    n = np.diagonal(a)
    union = n[:, None] + n[None, :] - a
    t = np.ones(a.shape, np.float64)
    np.divide(a, union, out=t, where=union > 0)
    np.fill_diagonal(t, 1.0)
    return t


def distance(inter):
    """1 - tanimoto: float64 [F, F], 0 on the diagonal and between two models without features."""
    return 1.0 - tanimoto(inter)


def medoid(inter):
    """The model with the largest summed Tanimoto similarity to all models (0-based); the lowest index wins a tie."""
    a = _square(inter)
    if not len(a):
        raise ValueError('medoid: no model')
    return int(np.argmax(tanimoto(a).sum(axis=1)))


def to_records(inter, model_numbers=None):
    """One dict per pair f < g for JSON: the two models (0-based index, or ``model_numbers[f]``), 'shared', the two feature
    counts and 'tanimoto'; plain ints and floats."""
    a = _square(inter)
    t = tanimoto(a)
    name = (lambda f: f) if model_numbers is None else (lambda f: model_numbers[f])
    F = len(a)
    return [{'bgn': name(f), 'end': name(g), 'type': 'model-similarity', 'shared': int(a[f, g]), 'n_bgn': int(a[f, f]),
             'n_end': int(a[g, g]), 'tanimoto': float(t[f, g])} for f in range(F) for g in range(f + 1, F)]


CSV_HEADER = ['f', 'g', 'shared', 'n_f', 'n_g', 'tanimoto']


def write_csv(path, inter):
    """One line per pair f < g (0-based model indices): f, g, shared, n_f, n_g and the Tanimoto similarity as the shortest
    text that gives the float64 back (``repr``)."""
    a = _square(inter)
    t = tanimoto(a)
    F = len(a)
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for f in range(F):
            for g in range(f + 1, F):
                w.writerow([f, g, int(a[f, g]), int(a[f, f]), int(a[g, g]), repr(float(t[f, g]))])


def write_similarity(wd, sid, inter):
    """'<id>.modelsim' in ``wd``."""
    path = os.path.join(wd, sid + '.modelsim')
    write_csv(path, inter)
    return path
