"""Host side of the water-bridge persistence table (``Context.models_water_bridge_persistence`` /
``EnsembleComplex.run_water_bridge_persistence``): the occupancy of water bridges over the models of an ensemble.

A table is a dict of fourteen NumPy columns, one row per pair of topology atoms (``tables.BRIDGEPERSIST_ATOM``: ``a < b``) or of
topology residues (``tables.BRIDGEPERSIST_RESIDUE``: ``res_a <= res_b``) that share a water in at least one model, rows
ascending by the pair.  Leg "a" of a bridge row is its own leg a at atom level; at residue level it is the leg whose partner
lies in ``res_a`` (the row's own leg a when the residues are equal).  A row's path is ``dist_a + dist_b``, added in float32.

    a, b / res_a, res_b         int32        topology ids
    n_models                    uint16       models with at least one bridge row of the pair
    first, last                 int32        lowest / highest 0-based model index among those
    n_waters                    uint32       sum over the models of the distinct waters bridging the pair in that model
    n_bridges                   uint32       bridge rows of the pair over all models (atom level: equals n_waters)
    dist_min                    float32      smallest path over all rows
    dist_max                    float32      largest of the per-model smallest paths
    dist_sum                    float64      the per-model smallest paths added one by one in ascending model order
                                             (mean tightest bridge = dist_sum / n_models)
    bit_models_a, bit_models_b  uint16 [15]  per SIFt bit (``config.SIFT_NAMES``): models in which a row's leg a (b) has it
    ctype_mask_a, ctype_mask_b  uint8        OR of 1 << contact type of leg a (b) over all rows

Everything here is NumPy on the host: no GPU is needed to fold, merge, normalise or export tables.  ``fold`` makes the table
from a bridge table — the twin of the device's reduction, and the fallback where the bridge table is on the host anyway.
"""
import csv
import os

import numpy as np

from . import tables
from .core import config

N_BITS = tables.N_BITS
BY_RESIDUE = 1 << 1                  # ARP_WBP_BY_RESIDUE
LEVELS = {'atom': tables.BRIDGEPERSIST_ATOM, 'residue': tables.BRIDGEPERSIST_RESIDUE}
COLUMNS = {level: spec.columns for level, spec in LEVELS.items()}
_SW = config.CONTACT_TYPE_NAMES.index('SELECTION_WATER')
_NW = config.CONTACT_TYPE_NAMES.index('NON_SELECTION_WATER')


def level_of(t):
    """'atom' or 'residue': by the names of a table's first two columns."""
    return 'residue' if 'res_a' in t else 'atom'


def _spec(level):
    if level not in LEVELS:
        raise ValueError(f"bridge_persistence: level must be 'atom' or 'residue', not {level!r}")
    return LEVELS[level]


def empty(level='atom'):
    """A table without rows."""
    return tables.empty(_spec(level))


def fold(bridge_table, n_atoms_per_model, res_id_topology=None):
    """The table of a bridge table over resident models (``Context.water_bridges`` with models resident: resident atom ids,
    every model ``n_atoms_per_model`` atoms): at atom level, or — with ``res_id_topology``, the residue of every topology
    atom — at residue level."""
    n = int(n_atoms_per_model)
    if n <= 0:
        raise ValueError('fold: n_atoms_per_model must be positive')
    spec = tables.BRIDGEPERSIST_ATOM if res_id_topology is None else tables.BRIDGEPERSIST_RESIDUE
    ka, kb = spec.columns[0][0], spec.columns[1][0]
    w = np.asarray(bridge_table['water']).astype(np.int64)
    if not len(w):
        return tables.empty(spec)
    f = w // n
    a, b = np.asarray(bridge_table['a']).astype(np.int64) - f * n, np.asarray(bridge_table['b']).astype(np.int64) - f * n
    if res_id_topology is None:
        lo, hi, swap = a, b, np.zeros(len(w), bool)
    else:
        res = np.asarray(res_id_topology).astype(np.int64)
        ra, rb = res[a], res[b]
        lo, hi, swap = np.minimum(ra, rb), np.maximum(ra, rb), ra > rb
    path = (np.asarray(bridge_table['dist_a'], np.float32) + np.asarray(bridge_table['dist_b'], np.float32)).astype(np.float32)
    leg = {}
    for k in ('sift', 'ctype'):
        xa, xb = np.asarray(bridge_table[k + '_a']).astype(np.int64), np.asarray(bridge_table[k + '_b']).astype(np.int64)
        leg[k] = (np.where(swap, xb, xa), np.where(swap, xa, xb))
    stride = int(hi.max()) + 1
    key, inv = np.unique(lo * stride + hi, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(key)
    F = int(f.max()) + 1
    # the (pair, model) groups in ascending (pair, model); per group the smallest path and the OR of either leg's SIFt
    gkey, g = np.unique(inv * F + f, return_inverse=True)
    g = g.reshape(-1)
    ginv, gf = gkey // F, gkey % F
    gmin = np.full(len(gkey), np.inf, np.float32)
    np.minimum.at(gmin, g, path)
    out = tables.alloc(spec, U, np.zeros)
    out[ka], out[kb] = (key // stride).astype(np.int32), (key % stride).astype(np.int32)
    out['n_models'] = np.bincount(ginv, minlength=U).astype(np.uint16)
    first, last = np.full(U, F, np.int64), np.full(U, -1, np.int64)
    np.minimum.at(first, ginv, gf)
    np.maximum.at(last, ginv, gf)
    out['first'], out['last'] = first.astype(np.int32), last.astype(np.int32)
    waters = np.unique(np.stack([inv, w], axis=1), axis=0)          # (a resident water id names its model)
    out['n_waters'] = np.bincount(waters[:, 0], minlength=U).astype(np.uint32)
    out['n_bridges'] = np.bincount(inv, minlength=U).astype(np.uint32)
    dmin, dmax = np.full(U, np.inf, np.float32), np.full(U, -np.inf, np.float32)
    np.minimum.at(dmin, inv, path)
    np.maximum.at(dmax, ginv, gmin)
    out['dist_min'], out['dist_max'] = dmin, dmax
    dsum = np.zeros(U, np.float64)
    np.add.at(dsum, ginv, gmin.astype(np.float64))                   # (unbuffered, in the groups' order: ascending model per pair)
    out['dist_sum'] = dsum
    for side, q in (('a', 0), ('b', 1)):
        gs = np.zeros(len(gkey), np.int64)
        np.bitwise_or.at(gs, g, leg['sift'][q])
        for k in range(N_BITS):
            out['bit_models_' + side][:, k] = np.bincount(ginv, weights=(gs >> k) & 1, minlength=U).astype(np.uint16)
        m = np.zeros(U, np.int64)
        np.bitwise_or.at(m, inv, 1 << leg['ctype'][q])
        out['ctype_mask_' + side] = m.astype(np.uint8)
    return out


def merge(t1, t2, model_offset):
    """The table of two chunks of one trajectory: ``t1`` over models [0, model_offset), ``t2`` over the models that follow
    (its 0-based model indices are shifted by ``model_offset``).  Counts are added, min / max / OR combined, and
    ``dist_sum = t1.dist_sum + t2.dist_sum`` in that order, as ``persistence.merge`` defines it — so a table accumulated
    chunk by chunk is defined to the bit by the chunking, and differs from the one-pass table of all the models at most in
    the rounding of ``dist_sum``.  Both tables must be of one level.  ``OverflowError`` when a count would leave its type."""
    level = level_of(t1)
    if level_of(t2) != level:
        raise ValueError('merge: an atom-level and a residue-level table do not merge')
    spec = LEVELS[level]
    return tables.merge(spec, t1, t2, model_offset, (spec.columns[0][0], spec.columns[1][0]),
                        {'n_models': 65535, 'n_waters': 0xFFFFFFFF, 'n_bridges': 0xFFFFFFFF, 'bit_models_a': 65535, 'bit_models_b': 65535},
                        'merge: {k} leaves its type (a pair bridged in more than 65535 models, or 2^32 bridges)',
                        ors=('ctype_mask_a', 'ctype_mask_b'))


def frequency(t, n_models):
    """Occupancy of every pair over ``n_models`` models: ``{'bridge': n_models / F [U], 'bits_a': bit_models_a / F [U, 15],
    'bits_b': bit_models_b / F [U, 15]}`` as float64."""
    F = int(n_models)
    if F < 1:
        raise ValueError('frequency: n_models must be at least 1')
    return {'bridge': t['n_models'].astype(np.float64) / F, 'bits_a': t['bit_models_a'].astype(np.float64) / F,
            'bits_b': t['bit_models_b'].astype(np.float64) / F}


def ligand_rows(t):
    """The rows that bridge the selection to the rest through a water: one leg mask has SELECTION_WATER, the other
    NON_SELECTION_WATER."""
    ma, mb = np.asarray(t['ctype_mask_a']).astype(np.int64), np.asarray(t['ctype_mask_b']).astype(np.int64)
    sw, nw = 1 << _SW, 1 << _NW
    m = (((ma & sw) != 0) & ((mb & nw) != 0)) | (((ma & nw) != 0) & ((mb & sw) != 0))
    return {k: np.asarray(t[k])[m] for k, _ in COLUMNS[level_of(t)]}


def to_records(t, pc, component_types=None):
    """The table as a list of dicts for JSON: 'bgn' / 'end' label the two atoms as ``water_bridges.to_records`` does, or the
    two residues as ``residue_pairs.to_records`` does, each with 'contact' (SIFt name -> models in which the leg has it) and
    'interacting_entities' (the contact types the leg met); the counts are plain ints."""
    from .core import export
    from .residue_pairs import _residue_dict
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    level = level_of(t)
    ka, kb = COLUMNS[level][0][0], COLUMNS[level][1][0]
    label = (lambda x: lab.atom_dict(x)) if level == 'atom' else (lambda x: _residue_dict(lab, x))
    out = []
    for r in range(len(t[ka])):
        ends = {}
        for side, k, q in (('bgn', ka, 'a'), ('end', kb, 'b')):
            ends[side] = dict(label(int(t[k][r])), contact=tables.sift_counts(t['bit_models_' + q][r].tolist()),
                              interacting_entities=tables.contact_types(int(t['ctype_mask_' + q][r])))
        nm, s = int(t['n_models'][r]), float(t['dist_sum'][r])
        out.append({'bgn': ends['bgn'], 'end': ends['end'], 'type': 'water-bridge-persistence', 'level': level, 'n_models': nm,
                    'first_model': int(t['first'][r]), 'last_model': int(t['last'][r]), 'n_waters': int(t['n_waters'][r]),
                    'n_bridges': int(t['n_bridges'][r]), 'distance_min': float(t['dist_min'][r]),
                    'distance_max': float(t['dist_max'][r]), 'distance_sum': s, 'distance_mean': s / nm})
    return out


def csv_header(level):
    """The header of ``write_csv`` at a level."""
    _spec(level)
    return ([level + '_bgn', level + '_end', 'n_models', 'first_model', 'last_model', 'n_waters', 'n_bridges', 'distance_min',
             'distance_max', 'distance_sum'] + [n + '_bgn' for n in config.SIFT_NAMES[:N_BITS]] +
            [n + '_end' for n in config.SIFT_NAMES[:N_BITS]] + ['interacting_entities_bgn', 'interacting_entities_end'])


def write_csv(path, t, pc, component_types=None):
    """One row per pair: the atoms ('A/508/O') or residues ('A/508/') in the form the other CSV tables use, the model count
    and range, the waters and bridges, the three distances (the shortest text that gives the value back), the fifteen SIFt
    model counts of either leg and the contact types either leg met, joined with '|'."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    level = level_of(t)
    ka, kb = COLUMNS[level][0][0], COLUMNS[level][1][0]
    label = (lambda x: lab.atom_macro(x)) if level == 'atom' else (lambda x: lab.res_macro[x])
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(csv_header(level))
        for r in range(len(t[ka])):
            w.writerow([label(int(t[ka][r])), label(int(t[kb][r])), int(t['n_models'][r]), int(t['first'][r]), int(t['last'][r]),
                        int(t['n_waters'][r]), int(t['n_bridges'][r]), str(t['dist_min'][r]), str(t['dist_max'][r]),
                        repr(float(t['dist_sum'][r]))] + t['bit_models_a'][r].tolist() + t['bit_models_b'][r].tolist() +
                       ['|'.join(tables.contact_types(int(t['ctype_mask_a'][r]))), '|'.join(tables.contact_types(int(t['ctype_mask_b'][r])))])


def write_bridge_persistence(wd, sid, t, pc, component_types=None):
    """'<id>.bridgepersist' in ``wd``."""
    path = os.path.join(wd, sid + '.bridgepersist')
    write_csv(path, t, pc, component_types)
    return path
