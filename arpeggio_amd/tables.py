"""What the device-reduced tables share on the host: contact persistence (``persistence``), the residue-pair table
(``residue_pairs``), residue persistence (``residue_persistence``), the water bridges (``water_bridges``), water-bridge
persistence (``bridge_persistence``), contact lifetimes (``lifetimes``), the interaction networks (``networks``) and the two
tables of contact coupling (``coupling``).

A table is a dict of NumPy columns with one row per pair (``NETWORKS``: per component).  A ``Spec`` names the columns in the order of the C fetch's
arguments (include/arpeggio_hip.h) with their types, and the width of those that hold several values a row.  Everything here
is NumPy on the host.
"""
from typing import NamedTuple

import numpy as np

from .core import config

N_BITS = 15       # SIFt bits with a count of their own (ARP_*_BITS): config.SIFT_NAMES[:15]


class Bag(NamedTuple):
    """One ring / amide bag: its columns in the order of the C fetches' arguments (PLANE_TABLES in csrc/arp_bag_table.h says the same)."""
    ids: tuple          # the two int32 id columns, each (name, what it indexes: 'atom' | 'ring' | 'amide')
    vals: tuple         # the value columns
    vdt: type           # ... and their dtype
    bytes: tuple        # the uint8 columns
    order: tuple        # the id columns of the canonical order, major key first


BAGS = {
    'atom_plane': Bag((('atom', 'atom'), ('ring', 'ring')), ('dist', 'theta'), np.float64, ('mask', 'ctype'), ('ring', 'atom')),
    'plane_plane': Bag((('bgn', 'ring'), ('end', 'ring')), ('dist', 'dihedral', 'theta_bgn', 'theta_end'), np.float64,
                       ('type1', 'type2', 'ctype'), ('bgn', 'end')),
    'group_group': Bag((('bgn', 'amide'), ('end', 'amide')), ('dist', 'dihedral', 'theta'), np.float32, ('ctype',), ('bgn', 'end')),
    'group_plane': Bag((('amide', 'amide'), ('ring', 'ring')), ('dist', 'dihedral', 'theta'), np.float64, ('ctype',), ('amide', 'ring')),
}
PLANE_BAGS = tuple(BAGS)
PACKED_ORDER = ('plane_plane', 'atom_plane', 'group_group', 'group_plane')      # get_contacts: arp_fetch_packed's counts[1..4] and b
CLASSES = ('atom_atom',) + PLANE_BAGS


def bag_columns(name):
    """Every column of bag ``name`` as (name, dtype, slot), in fetch order.  slot: its place among the twelve offsets a bag has in
    a packed fetch — ids 0 and 1, 8-byte values from 2, 4-byte values from 6, bytes from 9."""
    b = BAGS[name]
    v0 = 2 if np.dtype(b.vdt).itemsize == 8 else 6
    return [(c, np.int32, q) for q, (c, _) in enumerate(b.ids)] + [(c, b.vdt, v0 + q) for q, c in enumerate(b.vals)] + \
           [(c, np.uint8, 9 + q) for q, c in enumerate(b.bytes)]


def bag_buffers(name, cap, make=np.empty):
    """The columns of bag ``name`` for ``cap`` records, each made by ``make(cap, dtype)``."""
    return [make(cap, dt) for _, dt, _ in bag_columns(name)]


class Spec(NamedTuple):
    columns: tuple      # ((name, dtype), ...)
    width: dict         # name -> values per row, for the columns that are [U, width]


PERSIST = Spec((('a', np.int32), ('b', np.int32), ('n_models', np.uint16), ('first', np.int32), ('last', np.int32),
                ('dist_min', np.float32), ('dist_max', np.float32), ('dist_sum', np.float64), ('bit_count', np.uint16),
                ('ctype_mask', np.uint8)), {'bit_count': N_BITS})
RESPAIR = Spec((('res_a', np.int32), ('res_b', np.int32), ('n_contacts', np.uint32), ('dist_min', np.float32),
                ('bit_count', np.uint32), ('ctype_mask', np.uint8), ('plane_count', np.uint32)),
               {'bit_count': N_BITS, 'plane_count': len(PLANE_BAGS)})
RESPERSIST = Spec((('res_a', np.int32), ('res_b', np.int32), ('n_models', np.uint16), ('first', np.int32), ('last', np.int32),
                   ('n_contacts', np.uint32), ('class_models', np.uint16), ('bit_models', np.uint16), ('dist_min', np.float32),
                   ('dist_max', np.float32), ('dist_sum', np.float64), ('ctype_mask', np.uint8)),
                  {'class_models': len(CLASSES), 'bit_models': N_BITS})
BRIDGES = Spec((('water', np.int32), ('a', np.int32), ('b', np.int32), ('dist_a', np.float32), ('dist_b', np.float32),
                ('sift_a', np.uint16), ('sift_b', np.uint16), ('ctype_a', np.uint8), ('ctype_b', np.uint8)), {})


def _bridgepersist(ka, kb):
    return Spec(((ka, np.int32), (kb, np.int32), ('n_models', np.uint16), ('first', np.int32), ('last', np.int32),
                 ('n_waters', np.uint32), ('n_bridges', np.uint32), ('dist_min', np.float32), ('dist_max', np.float32),
                 ('dist_sum', np.float64), ('bit_models_a', np.uint16), ('bit_models_b', np.uint16), ('ctype_mask_a', np.uint8),
                 ('ctype_mask_b', np.uint8)), {'bit_models_a': N_BITS, 'bit_models_b': N_BITS})


LIFETIMES = Spec((('a', np.int32), ('b', np.int32), ('n_models', np.uint16), ('first', np.int32), ('last', np.int32),
                  ('n_intervals', np.uint16), ('longest', np.uint16), ('longest_start', np.int32), ('head', np.uint16),
                  ('tail', np.uint16), ('span_sum', np.uint32)), {})
NETWORKS = Spec((('root', np.int32), ('n_nodes', np.int32), ('n_edges', np.int32), ('sift_or', np.uint16), ('ctype_or', np.uint8)), {})
COUPLING_FEATURES = Spec((('a', np.int32), ('b', np.int32), ('count', np.uint32)), {})
COUPLING_PAIRS = Spec((('u', np.uint32), ('v', np.uint32), ('n11', np.uint32)), {})
BRIDGEPERSIST_ATOM = _bridgepersist('a', 'b')
BRIDGEPERSIST_RESIDUE = _bridgepersist('res_a', 'res_b')


def alloc(spec, U, make=np.empty):
    """The columns of ``spec`` for ``U`` rows, each made by ``make(shape, dtype)``."""
    return {k: make((U, spec.width[k]) if k in spec.width else U, dt) for k, dt in spec.columns}


def empty(spec):
    """A table without rows."""
    return alloc(spec, 0, np.zeros)


def merge(spec, t1, t2, model_offset, keys, additive, overflow, mins=('dist_min',), maxs=('dist_max',), ors=('ctype_mask',)):
    """The table of two chunks of one trajectory: ``t1`` over models [0, model_offset), ``t2`` over the models that follow.
    Rows are joined on the two ``keys`` columns and come back in their order.  ``additive`` maps each count column to the
    largest value its type holds (``OverflowError(overflow.format(k=column))`` beyond it); ``mins`` / ``maxs`` / ``ors`` name
    the columns combined by min / max / OR; 'first' / 'last' are model indices (those of ``t2`` shifted by ``model_offset``);
    and ``dist_sum = t1.dist_sum + t2.dist_sum`` in that order.  A row that one side lacks brings +inf / -inf / 0 / 0.0 there:
    the identities of min / max / OR / +."""
    model_offset = int(model_offset)
    if model_offset < 0:
        raise ValueError('merge: model_offset must not be negative')
    ka, kb = keys
    a = np.concatenate([t1[ka], t2[ka]]).astype(np.int64)
    b = np.concatenate([t1[kb], t2[kb]]).astype(np.int64)
    n1 = len(t1[ka])
    stride = int(b.max()) + 1 if len(b) else 1
    key, inv = np.unique(a * stride + b, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(key)
    r1, r2 = inv[:n1], inv[n1:]      # (a table's pairs are distinct: each of r1, r2 hits a row at most once)
    out = alloc(spec, U, np.zeros)
    out[ka], out[kb] = (key // stride).astype(np.int32), (key % stride).astype(np.int32)
    for k, top in additive.items():
        acc = np.zeros(out[k].shape, np.int64)
        acc[r1] += t1[k]
        acc[r2] += t2[k]
        if acc.size and acc.max() > top:
            raise OverflowError(overflow.format(k=k))
        out[k] = acc.astype(out[k].dtype)
    out['first'][r2] = t2['first'] + model_offset      # (every model of t2 comes after every model of t1 ...)
    out['first'][r1] = t1['first']                     # ... so t1's first wins where both have the pair,
    out['last'][r1] = t1['last']
    out['last'][r2] = t2['last'] + model_offset        # and t2's last
    for names, identity, fold in ((mins, np.inf, np.minimum), (maxs, -np.inf, np.maximum), (ors, 0, np.bitwise_or)):
        for k in names:
            out[k][:] = identity
            out[k][r1] = t1[k]
            out[k][r2] = fold(out[k][r2], t2[k])
    s1, s2 = np.zeros(U, np.float64), np.zeros(U, np.float64)
    s1[r1] = t1['dist_sum']
    s2[r2] = t2['dist_sum']
    out['dist_sum'] = s1 + s2        # (a pair of one table alone: x + 0.0, which is x — a sum of distances is never -0.0)
    return out


def sift_counts(counts):
    """{SIFt name: count} for the counts of a row that are not zero."""
    return {config.SIFT_NAMES[k]: counts[k] for k in range(N_BITS) if counts[k]}


def contact_types(mask):
    """The names of the contact types in a ``ctype_mask``."""
    ctn = config.CONTACT_TYPE_NAMES
    return [ctn[k] for k in range(len(ctn)) if (mask >> k) & 1]
