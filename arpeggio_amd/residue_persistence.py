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

from .core import config
from .residue_pairs import PLANE_BAGS, _residue_dict

COLUMNS = (('res_a', np.int32), ('res_b', np.int32), ('n_models', np.uint16), ('first', np.int32), ('last', np.int32),
           ('n_contacts', np.uint32), ('class_models', np.uint16), ('bit_models', np.uint16), ('dist_min', np.float32),
           ('dist_max', np.float32), ('dist_sum', np.float64), ('ctype_mask', np.uint8))
N_BITS = 15
CLASSES = ('atom_atom',) + PLANE_BAGS
_WIDTH = {'class_models': len(CLASSES), 'bit_models': N_BITS}
_U16_MAX = 65535
_U32_MAX = 0xFFFFFFFF


def empty():
    """A table without rows."""
    return {k: np.zeros((0, _WIDTH[k]) if k in _WIDTH else 0, dt) for k, dt in COLUMNS}


def merge(t1, t2, model_offset):
    """The table of two chunks of one trajectory: ``t1`` over models [0, model_offset), ``t2`` over the models that follow
    (its 0-based model indices are shifted by ``model_offset``).  Counts are added, min / max / OR combined, and
    ``dist_sum = t1.dist_sum + t2.dist_sum`` in that order, as ``persistence.merge`` defines it — so a table accumulated
    chunk by chunk is defined to the bit by the chunking, and differs from the one-pass table of all the models at most in
    the rounding of ``dist_sum``.  Rows in (res_a, res_b) order.  ``OverflowError`` when a count would leave its type."""
    model_offset = int(model_offset)
    if model_offset < 0:
        raise ValueError('merge: model_offset must not be negative')
    a = np.concatenate([t1['res_a'], t2['res_a']]).astype(np.int64)
    b = np.concatenate([t1['res_b'], t2['res_b']]).astype(np.int64)
    n1 = len(t1['res_a'])
    stride = int(b.max()) + 1 if len(b) else 1
    key, inv = np.unique(a * stride + b, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(key)
    r1, r2 = inv[:n1], inv[n1:]      # (a table's pairs are distinct: each of r1, r2 hits a row at most once)
    out = {'res_a': (key // stride).astype(np.int32), 'res_b': (key % stride).astype(np.int32)}
    for k, width, top in (('n_models', None, _U16_MAX), ('n_contacts', None, _U32_MAX), ('class_models', len(CLASSES), _U16_MAX),
                          ('bit_models', N_BITS, _U16_MAX)):
        acc = np.zeros(U if width is None else (U, width), np.int64)
        acc[r1] += t1[k]
        acc[r2] += t2[k]
        if acc.size and acc.max() > top:
            raise OverflowError(f'merge: {k} leaves its type (a pair counted in more than 65535 models, or 2^32 records)')
        out[k] = acc.astype(dict(COLUMNS)[k])
    first, last = np.zeros(U, np.int32), np.zeros(U, np.int32)
    first[r2] = t2['first'] + model_offset      # (every model of t2 comes after every model of t1 ...)
    first[r1] = t1['first']                     # ... so t1's first wins where both have the pair,
    last[r1] = t1['last']
    last[r2] = t2['last'] + model_offset        # and t2's last
    out['first'], out['last'] = first, last
    # (a pair without atom-atom records on one side brings +inf / -inf / 0.0 there: the identities of min / max / +)
    dmin, dmax = np.full(U, np.inf, np.float32), np.full(U, -np.inf, np.float32)
    dmin[r1], dmax[r1] = t1['dist_min'], t1['dist_max']
    dmin[r2] = np.minimum(dmin[r2], t2['dist_min'])
    dmax[r2] = np.maximum(dmax[r2], t2['dist_max'])
    out['dist_min'], out['dist_max'] = dmin, dmax
    s1, s2 = np.zeros(U, np.float64), np.zeros(U, np.float64)
    s1[r1] = t1['dist_sum']
    s2[r2] = t2['dist_sum']
    out['dist_sum'] = s1 + s2
    ct = np.zeros(U, np.uint8)
    ct[r1] |= t1['ctype_mask']
    ct[r2] |= t2['ctype_mask']
    out['ctype_mask'] = ct
    return {k: out[k] for k, _ in COLUMNS}


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
    names, ctn = config.SIFT_NAMES, config.CONTACT_TYPE_NAMES
    out = []
    for r in range(len(t['res_a'])):
        bm = t['bit_models'][r].tolist()
        cl = t['class_models'][r].tolist()
        cm = int(t['ctype_mask'][r])
        s = float(t['dist_sum'][r])
        aa = cl[0]
        out.append({'bgn': _residue_dict(lab, int(t['res_a'][r])), 'end': _residue_dict(lab, int(t['res_b'][r])),
                    'type': 'residue-residue', 'n_models': int(t['n_models'][r]), 'first_model': int(t['first'][r]),
                    'last_model': int(t['last'][r]), 'n_contacts': int(t['n_contacts'][r]),
                    'distance_min': float(t['dist_min'][r]) if aa else None, 'distance_max': float(t['dist_max'][r]) if aa else None,
                    'distance_sum': s if aa else None, 'distance_mean': s / aa if aa else None,
                    'contact': {names[k]: bm[k] for k in range(N_BITS) if bm[k]},
                    'classes': {CLASSES[k]: cl[k] for k in range(len(CLASSES)) if cl[k]},
                    'interacting_entities': [ctn[k] for k in range(len(ctn)) if (cm >> k) & 1]})
    return out


CSV_HEADER = ['residue_bgn', 'residue_end', 'n_models', 'first_model', 'last_model', 'n_contacts', 'distance_min', 'distance_max',
              'distance_sum'] + ['models_' + c for c in CLASSES] + list(config.SIFT_NAMES) + ['interacting_entities']


def write_csv(path, t, pc, component_types=None):
    """One row per residue pair: the residues in the form the other CSV tables use ('A/508/'), the model counts and range, the
    atom-atom records, the three distances (empty without an atom-atom record), the five class counts, the fifteen SIFt
    counts and the contact types met, joined with '|'."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    ctn = config.CONTACT_TYPE_NAMES
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r in range(len(t['res_a'])):
            aa = int(t['class_models'][r][0])
            cm = int(t['ctype_mask'][r])
            dist = [str(t['dist_min'][r]), str(t['dist_max'][r]), repr(float(t['dist_sum'][r]))] if aa else ['', '', '']
            w.writerow([lab.res_macro[int(t['res_a'][r])], lab.res_macro[int(t['res_b'][r])], int(t['n_models'][r]), int(t['first'][r]),
                        int(t['last'][r]), int(t['n_contacts'][r])] + dist + t['class_models'][r].tolist() + t['bit_models'][r].tolist() +
                       ['|'.join(ctn[k] for k in range(len(ctn)) if (cm >> k) & 1)])


def write_residue_persistence(wd, sid, t, pc, component_types=None):
    """'<id>.respersist' in ``wd``."""
    path = os.path.join(wd, sid + '.respersist')
    write_csv(path, t, pc, component_types)
    return path
