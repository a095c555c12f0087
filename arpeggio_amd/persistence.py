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

from .core import config

COLUMNS = (('a', np.int32), ('b', np.int32), ('n_models', np.uint16), ('first', np.int32), ('last', np.int32),
           ('dist_min', np.float32), ('dist_max', np.float32), ('dist_sum', np.float64), ('bit_count', np.uint16),
           ('ctype_mask', np.uint8))
N_BITS = 15
_U16_MAX = 65535


def empty():
    """A table without rows."""
    return {k: np.zeros((0, N_BITS) if k == 'bit_count' else 0, dt) for k, dt in COLUMNS}


def merge(t1, t2, model_offset):
    """The table of two chunks of one trajectory: ``t1`` over models [0, model_offset), ``t2`` over the models that follow
    (its 0-based model indices are shifted by ``model_offset``).  Counts are added, min / max combined, and
    ``dist_sum = t1.dist_sum + t2.dist_sum`` in that order — so a table accumulated chunk by chunk is defined to the bit by
    the chunking, and differs from the one-pass table of all the models at most in the rounding of ``dist_sum``.  Rows in
    (a, b) order.  ``OverflowError`` when a count would leave uint16."""
    model_offset = int(model_offset)
    if model_offset < 0:
        raise ValueError('merge: model_offset must not be negative')
    a = np.concatenate([t1['a'], t2['a']]).astype(np.int64)
    b = np.concatenate([t1['b'], t2['b']]).astype(np.int64)
    n1 = len(t1['a'])
    stride = int(b.max()) + 1 if len(b) else 1
    key, inv = np.unique(a * stride + b, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(key)
    r1, r2 = inv[:n1], inv[n1:]      # (a table's pairs are distinct: each of r1, r2 hits a row at most once)
    in1 = np.zeros(U, bool)
    in1[r1] = True
    out = {'a': (key // stride).astype(np.int32), 'b': (key % stride).astype(np.int32)}
    nm = np.zeros(U, np.int64)
    nm[r1] += t1['n_models']
    nm[r2] += t2['n_models']
    bits = np.zeros((U, N_BITS), np.int64)
    bits[r1] += t1['bit_count']
    bits[r2] += t2['bit_count']
    if (len(nm) and nm.max() > _U16_MAX) or (bits.size and bits.max() > _U16_MAX):
        raise OverflowError('merge: a pair is counted in more than 65535 models (the table counts in uint16)')
    out['n_models'] = nm.astype(np.uint16)
    first, last = np.zeros(U, np.int32), np.zeros(U, np.int32)
    first[r2] = t2['first'] + model_offset      # (every model of t2 comes after every model of t1 ...)
    first[r1] = t1['first']                     # ... so t1's first wins where both have the pair,
    last[r1] = t1['last']
    last[r2] = t2['last'] + model_offset        # and t2's last
    out['first'], out['last'] = first, last
    dmin, dmax = np.zeros(U, np.float32), np.zeros(U, np.float32)
    dmin[r1], dmax[r1] = t1['dist_min'], t1['dist_max']
    only2 = ~in1[r2]
    dmin[r2[only2]], dmax[r2[only2]] = t2['dist_min'][only2], t2['dist_max'][only2]
    both = ~only2
    dmin[r2[both]] = np.minimum(dmin[r2[both]], t2['dist_min'][both])
    dmax[r2[both]] = np.maximum(dmax[r2[both]], t2['dist_max'][both])
    out['dist_min'], out['dist_max'] = dmin, dmax
    s1, s2 = np.zeros(U, np.float64), np.zeros(U, np.float64)
    s1[r1] = t1['dist_sum']
    s2[r2] = t2['dist_sum']
    out['dist_sum'] = s1 + s2        # (a pair of one table alone: x + 0.0, which is x — a sum of distances is never -0.0)
    out['bit_count'] = bits.astype(np.uint16)
    ct = np.zeros(U, np.uint8)
    ct[r1] |= t1['ctype_mask']
    ct[r2] |= t2['ctype_mask']
    out['ctype_mask'] = ct
    return {k: out[k] for k, _ in COLUMNS}


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
    names, ctn = config.SIFT_NAMES, config.CONTACT_TYPE_NAMES
    out = []
    for r in range(len(t['a'])):
        nm = int(t['n_models'][r])
        bc = t['bit_count'][r].tolist()
        cm = int(t['ctype_mask'][r])
        s = float(t['dist_sum'][r])
        out.append({'bgn': lab.atom_dict(int(t['a'][r])), 'end': lab.atom_dict(int(t['b'][r])), 'type': 'atom-atom',
                    'n_models': nm, 'first_model': int(t['first'][r]), 'last_model': int(t['last'][r]),
                    'distance_min': float(t['dist_min'][r]), 'distance_max': float(t['dist_max'][r]), 'distance_sum': s,
                    'distance_mean': s / nm if nm else None,
                    'contact': {names[k]: bc[k] for k in range(N_BITS) if bc[k]},
                    'interacting_entities': [ctn[k] for k in range(len(ctn)) if (cm >> k) & 1]})
    return out
