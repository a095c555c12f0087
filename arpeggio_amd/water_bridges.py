"""Host side of the water-mediated contacts (``Context.water_bridges`` / ``InteractionComplex.water_bridges`` /
``EnsembleComplex.run_water_bridges``): which two atoms share a water.

A LEG is an atom-atom record (i, j) with exactly one water atom (``config.F_WATER``) and ``(sift & sift_any) != 0``; the water
is ``w``, the other atom the partner.  Water-water records and records without a water are no legs: first-order bridges only.
A table is a dict of nine NumPy columns, one row per water ``w`` and unordered pair ``a < b`` of its partners — dropped when
``res_id[a] == res_id[b]`` unless ``same_residue`` is asked for —, rows in ascending (water, a, b):

    water, a, b        int32    atom ids
    dist_a, dist_b     float32  the distances of the records (w, a) and (w, b)
    sift_a, sift_b     uint16   the whole SIFt of each leg, not masked
    ctype_a, ctype_b   uint8    each leg's interacting-entities code (``config.CONTACT_TYPE_NAMES``)

A ligand-water-protein bridge is a row with one SELECTION_WATER leg and one NON_SELECTION_WATER leg (``ligand_bridges``).
There is no angle criterion at the water and no second-order (water-water-) bridge.  Persistence of bridges over the models of
an ensemble is ``arpeggio_amd.bridge_persistence`` (reduced on the device: ``Context.models_water_bridge_persistence``).

Everything here is NumPy on the host: no GPU, no native library.  ``join`` makes the table from a fetched atom-atom bag — the
only route before the device made it, and the fallback where the whole bag is on the host anyway.
"""
import csv
import os

import numpy as np

from . import tables
from .core import config

COLUMNS = tables.BRIDGES.columns
SIFT_ALL = (1 << len(config.SIFT_NAMES)) - 1
SAME_RESIDUE = 1                     # ARP_WB_SAME_RESIDUE
DEFAULT_CONTACTS = ('hbond', 'polar')
_SW = config.CONTACT_TYPE_NAMES.index('SELECTION_WATER')
_NW = config.CONTACT_TYPE_NAMES.index('NON_SELECTION_WATER')


def empty():
    """A table without rows."""
    return {k: np.zeros(0, dt) for k, dt in COLUMNS}


def mask(contacts=DEFAULT_CONTACTS):
    """``sift_any`` for the contacts named in ``contacts`` (``config.SIFT_NAMES``); ``None`` means all; an unknown name or
    an empty list raises ``ValueError``."""
    known = config.SIFT_NAMES
    if contacts is None:
        return SIFT_ALL
    names = [contacts] if isinstance(contacts, str) else list(contacts)
    if not names:
        raise ValueError('water_bridges.mask: an empty list of contact names makes no record a leg (None means all)')
    m = 0
    for nm in names:
        if nm not in known:
            raise ValueError(f'water_bridges.mask: unknown contact name {nm!r} (known: {", ".join(known)})')
        m |= 1 << known.index(nm)
    return m


def _check_mask(sift_any):
    sift_any = int(sift_any)
    if sift_any == 0 or sift_any & ~SIFT_ALL:
        raise ValueError('water_bridges: sift_any must name at least one of the 15 SIFt bits and nothing else')
    return sift_any


def join(bag, flags_per_atom, res_id, sift_any, same_residue=False):
    """The table of an atom-atom bag (a dict with the columns i, j, dist, sift, ctype, in any order of records),
    ``flags_per_atom`` (``pc.flags``) and ``res_id`` of its atoms."""
    sift_any = _check_mask(sift_any)
    i, j = np.asarray(bag['i']).astype(np.int64), np.asarray(bag['j']).astype(np.int64)
    water = (np.asarray(flags_per_atom).astype(np.int64) & config.F_WATER) != 0
    res = np.asarray(res_id)
    wi, wj = water[i], water[j]
    leg = np.nonzero((wi != wj) & ((np.asarray(bag['sift']).astype(np.int64) & sift_any) != 0))[0]
    if not len(leg):
        return empty()
    w = np.where(wi[leg], i[leg], j[leg])
    p = np.where(wi[leg], j[leg], i[leg])
    order = np.lexsort((p, w))
    leg, w, p = leg[order], w[order], p[order]
    # runs of one water; every pair of positions x < y inside a run
    start = np.nonzero(np.r_[True, w[1:] != w[:-1]])[0]
    m = np.diff(np.r_[start, len(w)])
    first = np.repeat(start, m)                      # per leg: where its run begins
    after = first + np.repeat(m, m) - 1 - np.arange(len(w))      # per leg: the legs of its run behind it
    x = np.repeat(np.arange(len(w)), after)
    y = np.arange(len(x)) - np.repeat(np.cumsum(after) - after, after) + x + 1
    if not same_residue:
        keep = res[p[x]] != res[p[y]]
        x, y = x[keep], y[keep]
    la, lb = leg[x], leg[y]
    dist, sift, ctype = np.asarray(bag['dist']), np.asarray(bag['sift']), np.asarray(bag['ctype'])
    return {'water': w[x].astype(np.int32), 'a': p[x].astype(np.int32), 'b': p[y].astype(np.int32),
            'dist_a': dist[la].astype(np.float32), 'dist_b': dist[lb].astype(np.float32),
            'sift_a': sift[la].astype(np.uint16), 'sift_b': sift[lb].astype(np.uint16),
            'ctype_a': ctype[la].astype(np.uint8), 'ctype_b': ctype[lb].astype(np.uint8)}


def split_structures(table, atom_offsets):
    """The table of several structures resident at once, cut into one table per structure: ``atom_offsets`` = the first atom
    id of every structure and, last, the resident atom count (a batch: ``off['atom']`` of ``batch.concat_complexes``).  A
    water only meets atoms of its own structure and the rows ascend by water, so structure s is the contiguous range of rows
    with water in [atom_offsets[s], atom_offsets[s + 1]) — a binary search, not a sort.  Ids come back structure-local."""
    off = np.asarray(atom_offsets, np.int64)
    if off.ndim != 1 or len(off) < 1 or np.any(np.diff(off) < 0):
        raise ValueError('split_structures: atom_offsets must be ascending, one entry per structure and the total last')
    bounds = np.searchsorted(table['water'], off, side='left')
    out = []
    for s in range(len(off) - 1):
        lo, hi = int(bounds[s]), int(bounds[s + 1])
        t = {k: table[k][lo:hi] for k, _ in COLUMNS}
        if hi > lo and (int(t['b'].max()) >= off[s + 1] or int(t['a'].min()) < off[s]):
            raise ValueError(f'split_structures: a row of structure {s} reaches into another one (atom_offsets do not fit the table)')
        for k in ('water', 'a', 'b'):
            t[k] = (t[k] - off[s]).astype(np.int32)
        out.append(t)
    return out


def split_models(table, n_atoms_per_model):
    """The table of the resident models of one topology, cut into one table per model with topology atom ids: every model
    holds ``n_atoms_per_model`` atoms; the number of models is what the rows reach."""
    n = int(n_atoms_per_model)
    if n <= 0:
        raise ValueError('split_models: n_atoms_per_model must be positive')
    top = int(table['water'].max()) if len(table['water']) else -1
    F = top // n + 1 if top >= 0 else 0
    return split_structures(table, np.arange(F + 1, dtype=np.int64) * n)


def ligand_bridges(table):
    """The rows that bridge the selection to the rest through a water: one leg SELECTION_WATER, the other
    NON_SELECTION_WATER."""
    ca, cb = np.asarray(table['ctype_a']), np.asarray(table['ctype_b'])
    m = ((ca == _SW) & (cb == _NW)) | ((ca == _NW) & (cb == _SW))
    return {k: np.asarray(table[k])[m] for k, _ in COLUMNS}


BY_RESIDUE_COLUMNS = (('res_a', np.int32), ('res_b', np.int32), ('n_waters', np.uint32), ('n_bridges', np.uint32), ('dist_min', np.float32))


def by_residue(table, res_id):
    """The table folded by the residues of a and b: one row per unordered residue pair res_a <= res_b, ascending, with the
    distinct bridging waters, the bridges and the smallest ``dist_a + dist_b`` (added in float32)."""
    res = np.asarray(res_id).astype(np.int64)
    ra, rb = res[np.asarray(table['a'], np.int64)], res[np.asarray(table['b'], np.int64)]
    lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
    stride = int(hi.max()) + 1 if len(hi) else 1
    key, inv = np.unique(lo * stride + hi, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(key)
    path = (np.asarray(table['dist_a'], np.float32) + np.asarray(table['dist_b'], np.float32)).astype(np.float32)
    dmin = np.full(U, np.inf, np.float32)
    np.minimum.at(dmin, inv, path)
    pairs = np.unique(np.stack([inv, np.asarray(table['water'], np.int64)], axis=1), axis=0) if U else np.zeros((0, 2), np.int64)
    return {'res_a': (key // stride).astype(np.int32), 'res_b': (key % stride).astype(np.int32),
            'n_waters': np.bincount(pairs[:, 0], minlength=U).astype(np.uint32),
            'n_bridges': np.bincount(inv, minlength=U).astype(np.uint32), 'dist_min': dmin}


def _names(bits, known):
    return [known[k] for k in range(len(known)) if (int(bits) >> k) & 1]


def to_records(table, pc, component_types=None):
    """The table as a list of dicts for JSON: 'water', 'bgn' and 'end' label the three atoms with the keys ``get_contacts``
    uses for an atom (export.py); each leg brings its distance, its contacts by name and its interacting entities."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    ctn = config.CONTACT_TYPE_NAMES
    out = []
    for r in range(len(table['water'])):
        legs = {}
        for side, atom in (('bgn', 'a'), ('end', 'b')):
            legs[side] = dict(lab.atom_dict(int(table[atom][r])), distance=float(table['dist_' + atom][r]),
                              contact=_names(table['sift_' + atom][r], config.SIFT_NAMES),
                              interacting_entities=ctn[int(table['ctype_' + atom][r])])
        out.append({'water': lab.atom_dict(int(table['water'][r])), 'bgn': legs['bgn'], 'end': legs['end'], 'type': 'water-bridge'})
    return out


CSV_HEADER = ['water', 'atom_bgn', 'atom_end', 'distance_bgn', 'distance_end', 'contacts_bgn', 'contacts_end',
              'interacting_entities_bgn', 'interacting_entities_end']


def write_csv(path, table, pc, component_types=None):
    """One row per bridge: the three atoms in the form the other CSV tables use ('A/508/O'), the two distances (the shortest
    text that gives the float32 back), each leg's contacts by name joined with '|', and each leg's interacting entities."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    ctn = config.CONTACT_TYPE_NAMES
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r in range(len(table['water'])):
            w.writerow([lab.atom_macro(int(table['water'][r])), lab.atom_macro(int(table['a'][r])), lab.atom_macro(int(table['b'][r])),
                        str(table['dist_a'][r]), str(table['dist_b'][r]),
                        '|'.join(_names(table['sift_a'][r], config.SIFT_NAMES)), '|'.join(_names(table['sift_b'][r], config.SIFT_NAMES)),
                        ctn[int(table['ctype_a'][r])], ctn[int(table['ctype_b'][r])]])


def write_water_bridges(wd, sid, table, pc, component_types=None):
    """'<id>.waterbridges' in ``wd``."""
    path = os.path.join(wd, sid + '.waterbridges')
    write_csv(path, table, pc, component_types)
    return path
