"""Host side of the contact-persistence table (``Context.models_persistence`` / ``EnsembleComplex.run_persistence``).

A table is a dict of ten NumPy columns, one row per distinct topology pair (a, b), a < b, rows in ascending (a, b):

    a, b                 int32        topology atom ids
    n_models             uint16       models in which the pair has a record
    first, last          int32        lowest / highest 0-based model index with a record
    dist_min, dist_max   float32      over those models
    dist_sum             float64      the float32 distances added one by one in ascending model order (mean = dist_sum / n_models)
    bit_count            uint16 [15]  per SIFt bit (``config.SIFT_NAMES``): models whose record has it
    ctype_mask           uint8        OR of 1 << contact type over the models

Everything here is NumPy on the host: no GPU is needed to merge, normalise or export tables.
"""
import numpy as np

from . import tables

COLUMNS = tables.PERSIST.columns
N_BITS = tables.N_BITS


def empty():
    """A table without rows."""
    return tables.empty(tables.PERSIST)


def merge(t1, t2, model_offset):
    """The table of two chunks of one trajectory: ``t1`` over models [0, model_offset), ``t2`` over the models that follow
    (its 0-based model indices are shifted by ``model_offset``).  Counts are added, min / max combined, and
    ``dist_sum = t1.dist_sum + t2.dist_sum`` in that order — so a table accumulated chunk by chunk is defined to the bit by
    the chunking, and differs from the one-pass table of all the models at most in the rounding of ``dist_sum``.  Rows in
    (a, b) order.  ``OverflowError`` when a count would leave uint16."""
    return tables.merge(tables.PERSIST, t1, t2, model_offset, ('a', 'b'), {'n_models': 65535, 'bit_count': 65535},
                        'merge: a pair is counted in more than 65535 models (the table counts in uint16)')


def frequency(t, n_models):
    """Occupancy of every pair and of every SIFt bit over ``n_models`` models: ``{'contact': n_models / F [U],
    'bits': bit_count / F [U, 15]}`` as float64."""
    F = int(n_models)
    if F < 1:
        raise ValueError('frequency: n_models must be at least 1')
    return {'contact': t['n_models'].astype(np.float64) / F, 'bits': t['bit_count'].astype(np.float64) / F}


def to_records(t, pc, component_types=None):
    """The table as a list of dicts for JSON: 'bgn' / 'end' label the two atoms in the form ``get_contacts`` uses (export.py),
    the counts are plain ints, 'contact' maps each SIFt name that occurs to the number of models with it, and
    'interacting_entities' lists the contact types met."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    out = []
    for r in range(len(t['a'])):
        nm = int(t['n_models'][r])
        s = float(t['dist_sum'][r])
        out.append({'bgn': lab.atom_dict(int(t['a'][r])), 'end': lab.atom_dict(int(t['b'][r])), 'type': 'atom-atom',
                    'n_models': nm, 'first_model': int(t['first'][r]), 'last_model': int(t['last'][r]),
                    'distance_min': float(t['dist_min'][r]), 'distance_max': float(t['dist_max'][r]), 'distance_sum': s,
                    'distance_mean': s / nm if nm else None,
                    'contact': tables.sift_counts(t['bit_count'][r].tolist()),
                    'interacting_entities': tables.contact_types(int(t['ctype_mask'][r]))})
    return out
