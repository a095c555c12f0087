"""Host side of the residue contact-persistence table (``Context.models_residue_persistence`` /
``EnsembleComplex.run_residue_persistence``): a residue contact-frequency map over the models of an ensemble.

A table is a dict of twelve NumPy columns, one row per pair of topology residues with at least one record in any of the five
bags of at least one model, rows in ascending (res_a, res_b):

    res_a, res_b   int32        topology residue indices, res_a <= res_b (equal only through ring / amide records)
    n_models       uint16       models with at least one record of the pair, in any bag
    first, last    int32        lowest / highest 0-based model index among those
    n_contacts     uint32       atom-atom records of the pair over all models
    class_models   uint16 [5]   models with a record of class m (``CLASSES``: atom-atom, then the four ring / amide bags)
    bit_models     uint16 [15]  per SIFt bit (``config.SIFT_NAMES``): models in which an atom-atom record of the pair has it
    dist_min       float32      smallest atom-atom distance over all models (+inf when class_models[0] == 0)
    dist_max       float32      largest of the per-model smallest atom-atom distances (-inf when class_models[0] == 0)
    dist_sum       float64      the per-model smallest distances added one by one in ascending model order
                                (mean closest approach = dist_sum / class_models[0])
    ctype_mask     uint8        OR of 1 << contact type over the atom-atom records

Everything here is NumPy on the host: no GPU is needed to merge, normalise or export tables.
"""
import csv
import os

import numpy as np

from . import tables
from .core import config
from .residue_pairs import _residue_dict

COLUMNS = tables.RESPERSIST.columns
N_BITS = tables.N_BITS
CLASSES = tables.CLASSES


def empty():
    """A table without rows."""
    return tables.empty(tables.RESPERSIST)


def merge(t1, t2, model_offset):
    """The table of two chunks of one trajectory: ``t1`` over models [0, model_offset), ``t2`` over the models that follow
    (its 0-based model indices are shifted by ``model_offset``).  Counts are added, min / max / OR combined, and
    ``dist_sum = t1.dist_sum + t2.dist_sum`` in that order, as ``persistence.merge`` defines it — so a table accumulated
    chunk by chunk is defined to the bit by the chunking, and differs from the one-pass table of all the models at most in
    the rounding of ``dist_sum``.  Rows in (res_a, res_b) order.  ``OverflowError`` when a count would leave its type."""
    return tables.merge(tables.RESPERSIST, t1, t2, model_offset, ('res_a', 'res_b'),
                        {'n_models': 65535, 'n_contacts': 0xFFFFFFFF, 'class_models': 65535, 'bit_models': 65535},
                        'merge: {k} leaves its type (a pair counted in more than 65535 models, or 2^32 records)')


def frequency(t, n_models):
    """Occupancy of every residue pair over ``n_models`` models: ``{'contact': n_models / F [U], 'classes': class_models / F
    [U, 5], 'bits': bit_models / F [U, 15]}`` as float64."""
    F = int(n_models)
    if F < 1:
        raise ValueError('frequency: n_models must be at least 1')
    return {'contact': t['n_models'].astype(np.float64) / F, 'classes': t['class_models'].astype(np.float64) / F,
            'bits': t['bit_models'].astype(np.float64) / F}


def to_records(t, pc, component_types=None):
    """The table as a list of dicts for JSON: 'bgn' / 'end' label the two residues as ``residue_pairs.to_records`` does, the
    counts are plain ints, 'contact' maps each SIFt name that occurs to the number of models with it, 'classes' each record
    class that occurs to its number of models, 'interacting_entities' lists the contact types met, and the distances are
    None for a pair without atom-atom records."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    out = []
    for r in range(len(t['res_a'])):
        cl = t['class_models'][r].tolist()
        s = float(t['dist_sum'][r])
        aa = cl[0]
        out.append({'bgn': _residue_dict(lab, int(t['res_a'][r])), 'end': _residue_dict(lab, int(t['res_b'][r])),
                    'type': 'residue-residue', 'n_models': int(t['n_models'][r]), 'first_model': int(t['first'][r]),
                    'last_model': int(t['last'][r]), 'n_contacts': int(t['n_contacts'][r]),
                    'distance_min': float(t['dist_min'][r]) if aa else None, 'distance_max': float(t['dist_max'][r]) if aa else None,
                    'distance_sum': s if aa else None, 'distance_mean': s / aa if aa else None,
                    'contact': tables.sift_counts(t['bit_models'][r].tolist()),
                    'classes': {CLASSES[k]: cl[k] for k in range(len(CLASSES)) if cl[k]},
                    'interacting_entities': tables.contact_types(int(t['ctype_mask'][r]))})
    return out


CSV_HEADER = ['residue_bgn', 'residue_end', 'n_models', 'first_model', 'last_model', 'n_contacts', 'distance_min', 'distance_max',
              'distance_sum'] + ['models_' + c for c in CLASSES] + list(config.SIFT_NAMES) + ['interacting_entities']


def write_csv(path, t, pc, component_types=None):
    """One row per residue pair: the residues in the form the other CSV tables use ('A/508/'), the model counts and range, the
    atom-atom records, the three distances (empty without an atom-atom record), the five class counts, the fifteen SIFt
    counts and the contact types met, joined with '|'."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r in range(len(t['res_a'])):
            aa = int(t['class_models'][r][0])
            dist = [str(t['dist_min'][r]), str(t['dist_max'][r]), repr(float(t['dist_sum'][r]))] if aa else ['', '', '']
            w.writerow([lab.res_macro[int(t['res_a'][r])], lab.res_macro[int(t['res_b'][r])], int(t['n_models'][r]), int(t['first'][r]),
                        int(t['last'][r]), int(t['n_contacts'][r])] + dist + t['class_models'][r].tolist() + t['bit_models'][r].tolist() +
                       ['|'.join(tables.contact_types(int(t['ctype_mask'][r])))])


def write_residue_persistence(wd, sid, t, pc, component_types=None):
    """'<id>.respersist' in ``wd``."""
    path = os.path.join(wd, sid + '.respersist')
    write_csv(path, t, pc, component_types)
    return path
