"""Host side of the interaction networks (``Context.networks`` / ``InteractionComplex.networks`` /
``EnsembleComplex.run_networks``): the connected components of the contact graph.

Which atoms form one hydrogen-bond network, waters included?  How large is the hydrophobic cluster the ligand sits in?  Is
this salt bridge isolated, or part of an ionic cluster?

Inputs

- the atom-atom bag of the last pass, with whatever is resident: one structure, a batch, or models;
- ``sift_any``: 15 bits, not 0;
- ``ctype_mask``: not 0, in the bit order of ``contact_filter.masks``;
- ``flags``: ``ARP_NET_BY_RESIDUE`` or 0 (here: ``res_id`` given or not).

Nodes

- atom level: the N = n resident atoms;
- residue level: the N = ``nres`` resident residues; a record's nodes are ``res_id[i]``, ``res_id[j]``;
- the ring and amide bags take no part at either level.

Edges

- a record takes part when ``(sift & sift_any) != 0`` and bit ``ctype`` of ``ctype_mask`` is set (the rule of
  ``arpeggio_amd.lifetimes`` and ``contact_filter.keep``);
- a participating record is an edge between its two nodes;
- a record with a negative node is left out;
- a record whose two nodes are equal counts as an edge of that node and joins nothing (a pass cannot produce one — I:729:
  no record joins two atoms of one residue — but this function and the kernel define it the same way).

Results

1. ``label``, int32 [N]: the smallest node id of the node's component, or -1 for a node with no participating record;
2. the component table, one row per component in ascending ``root``, columns in the order of the fetch's arguments
   (``tables.NETWORKS``):

       root      int32   the component's smallest node id
       n_nodes   int32
       n_edges   int32   participating records, multi-edges counted
       sift_or   uint16  OR of the whole ``sift`` of the component's participating records
       ctype_or  uint8   OR of ``1 << ctype``

Everything is an integer, a minimum, a count or an OR: the order of the records cannot show, and the device result
(csrc/arp_networks.h, a lock-free union-find) equals ``components`` exactly.  No record joins two structures of a batch or
two models, so components never cross them (``split_structures`` / ``split_models``).

Everything here is NumPy on the host: no GPU, no native library.  ``components`` makes the result from a fetched atom-atom
bag — the only route before the device made it, and the fallback where the whole bag is on the host anyway.
"""
import csv
import os

import numpy as np

from . import contact_filter, tables
from .core import config

COLUMNS = tables.NETWORKS.columns
SIFT_ALL, CTYPE_ALL = contact_filter.SIFT_ALL, contact_filter.CTYPE_ALL
BY_RESIDUE = 1                       # ARP_NET_BY_RESIDUE


def empty():
    """A table without rows."""
    return tables.empty(tables.NETWORKS)


def check_masks(sift_any, ctype_mask):
    """The two masks as ints; ``ValueError`` for a mask of 0 or with bits beyond its own (the launch's refusals)."""
    sift_any, ctype_mask = int(sift_any), int(ctype_mask)
    if sift_any & ~SIFT_ALL or ctype_mask & ~CTYPE_ALL:
        raise ValueError('networks: a mask has bits beyond the 15 SIFt bits / the 7 contact types')
    if sift_any == 0 or ctype_mask == 0:
        raise ValueError('networks: a mask of 0 lets no record take part')
    return sift_any, ctype_mask


def components(bag, n_nodes, sift_any=SIFT_ALL, ctype_mask=CTYPE_ALL, res_id=None):
    """``(label, table)`` of an atom-atom bag (a dict with the columns i, j, sift, ctype, in any order of records) over
    ``n_nodes`` nodes: atoms, or — ``res_id`` given, the residue of every atom — residues.  The contract of the module's
    head, in NumPy: rounds of hooking roots under smaller roots and pointer jumping, until no edge joins two roots."""
    sift_any, ctype_mask = check_masks(sift_any, ctype_mask)
    N = int(n_nodes)
    if N < 0:
        raise ValueError('networks.components: n_nodes must not be negative')
    sift = np.asarray(bag['sift']).astype(np.int64)
    ctype = np.asarray(bag['ctype']).astype(np.int64)
    a, b = np.asarray(bag['i']).astype(np.int64), np.asarray(bag['j']).astype(np.int64)
    if res_id is not None:
        res = np.asarray(res_id).astype(np.int64)
        a, b = res[a], res[b]
    part = contact_filter.keep(sift, ctype, sift_any, ctype_mask) & (a >= 0) & (b >= 0)
    a, b, sift, ctype = a[part], b[part], sift[part], ctype[part]
    if len(a) and max(int(a.max()), int(b.max())) >= N:
        raise ValueError('networks.components: a record names a node beyond n_nodes')
    touched = np.zeros(N, bool)
    touched[a] = True
    touched[b] = True
    # lab[v] <= v is v's root whenever a round begins (lab[lab] == lab).  A round hooks every root that an edge joins to a
    # smaller root under the smallest such root, then jumps pointers until every node sees its root again; the edges whose
    # ends have met leave.  The root of a component ends as its smallest node.
    lab = np.arange(N, dtype=np.int64)
    ea, eb = a, b
    while len(ea):
        ra, rb = lab[ea], lab[eb]
        open_ = ra != rb
        ea, eb, ra, rb = ea[open_], eb[open_], ra[open_], rb[open_]
        np.minimum.at(lab, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    label = np.where(touched, lab, -1).astype(np.int32)
    roots = np.nonzero(label == np.arange(N))[0]
    row = np.full(N, -1, np.int64)
    row[roots] = np.arange(len(roots))
    er = row[lab[a]]                    # the row of every participating record
    sift_or, ctype_or = np.zeros(len(roots), np.int64), np.zeros(len(roots), np.int64)
    np.bitwise_or.at(sift_or, er, sift)
    np.bitwise_or.at(ctype_or, er, 1 << ctype)
    table = {'root': roots.astype(np.int32),
             'n_nodes': np.bincount(row[label[touched]], minlength=len(roots)).astype(np.int32),
             'n_edges': np.bincount(er, minlength=len(roots)).astype(np.int32),
             'sift_or': sift_or.astype(np.uint16), 'ctype_or': ctype_or.astype(np.uint8)}
    return label, table


def members(label, root):
    """The node ids of the component with the smallest node ``root``, ascending (none when ``root`` is no root)."""
    return np.nonzero(np.asarray(label) == int(root))[0].astype(np.int32)


def of_atoms(label, atoms):
    """The roots of the components that a selection of nodes touches, ascending and distinct — the ligand's networks, for
    example.  Nodes without a participating record bring none."""
    got = np.asarray(label)[np.asarray(atoms, np.int64)]
    return np.unique(got[got >= 0]).astype(np.int32)


def split_structures(label, table, offsets):
    """The result of several structures resident at once, cut into one ``(label, table)`` per structure: ``offsets`` = the
    first node id of every structure and, last, the resident node count (a batch: ``off['atom']`` or ``off['residue']`` of
    ``batch.concat_complexes``).  No component spans two structures and the rows ascend by root, so structure s is a contiguous
    range of rows.  Ids come back structure-local; a label of -1 stays -1."""
    off = np.asarray(offsets, np.int64)
    label = np.asarray(label)
    if off.ndim != 1 or len(off) < 1 or np.any(np.diff(off) < 0) or (len(off) and off[-1] != len(label)):
        raise ValueError('split_structures: offsets must be ascending, one entry per structure and the node count last')
    bounds = np.searchsorted(table['root'], off, side='left')
    out = []
    for s in range(len(off) - 1):
        lab = label[off[s]:off[s + 1]]
        if len(lab) and (int(lab.max()) >= off[s + 1] or np.any((lab >= 0) & (lab < off[s]))):
            raise ValueError(f'split_structures: a component of structure {s} reaches into another one (offsets do not fit the labels)')
        t = {k: np.asarray(table[k])[int(bounds[s]):int(bounds[s + 1])] for k, _ in COLUMNS}
        t['root'] = (t['root'] - off[s]).astype(np.int32)
        out.append((np.where(lab >= 0, lab - off[s], -1).astype(np.int32), t))
    return out


def split_models(label, table, n_per_model):
    """The result over the resident models of one topology, cut into one ``(label, table)`` per model with topology ids:
    every model holds ``n_per_model`` nodes (atoms, or residues at residue level)."""
    n = int(n_per_model)
    if n <= 0 or len(label) % n:
        raise ValueError('split_models: n_per_model must be positive and divide the number of labels')
    return split_structures(label, table, np.arange(len(label) // n + 1, dtype=np.int64) * n)


def largest(table):
    """The row index of the component with the most nodes (the smallest root on a tie); -1 for a table without rows."""
    return int(np.argmax(table['n_nodes'])) if len(table['n_nodes']) else -1


def _names(bits, known):
    return [known[k] for k in range(len(known)) if (int(bits) >> k) & 1]


def _residue_dict(lab, r):
    n, s, c, ic = lab.res_json[r]
    return {'label_comp_id': n, 'auth_seq_id': s, 'auth_asym_id': c, 'pdbx_PDB_ins_code': ic, 'label_comp_type': lab.res_comp_type[r]}


def to_records(label, table, pc, level='atom', component_types=None):
    """The components as a list of dicts for JSON: 'members' labels every node with the keys ``get_contacts`` uses for an atom
    or a residue (export.py), 'root' is the first of them, the counts are plain ints, 'contact' lists the SIFt names met
    and 'interacting_entities' the contact types met."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    one = _level(level, lab.atom_dict, lambda r: _residue_dict(lab, r))
    out = []
    for r in range(len(table['root'])):
        m = [one(int(v)) for v in members(label, table['root'][r])]
        out.append({'root': m[0], 'members': m, 'type': 'network', 'level': level, 'n_nodes': int(table['n_nodes'][r]),
                    'n_edges': int(table['n_edges'][r]), 'contact': _names(table['sift_or'][r], config.SIFT_NAMES),
                    'interacting_entities': tables.contact_types(int(table['ctype_or'][r]))})
    return out


def _level(level, atom, residue):
    if level not in ('atom', 'residue'):
        raise ValueError("networks: level must be 'atom' or 'residue'")
    return atom if level == 'atom' else residue


CSV_HEADER = ['root', 'n_nodes', 'n_edges', 'contacts', 'interacting_entities', 'members']


def write_csv(path, label, table, pc, level='atom', component_types=None):
    """One row per component: its root in the form the other CSV tables use ('A/508/O', or 'A/508/' at residue level), its
    nodes and edges, the contacts met by name and the interacting entities met, each joined with '|', and its members in that
    form, ascending by id, joined with '|'."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    one = _level(level, lab.atom_macro, lambda r: lab.res_macro[r])
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r in range(len(table['root'])):
            w.writerow([one(int(table['root'][r])), int(table['n_nodes'][r]), int(table['n_edges'][r]),
                        '|'.join(_names(table['sift_or'][r], config.SIFT_NAMES)),
                        '|'.join(tables.contact_types(int(table['ctype_or'][r]))),
                        '|'.join(one(int(v)) for v in members(label, table['root'][r]))])


def write_networks(wd, sid, label, table, pc, level='atom', component_types=None):
    """'<id>.networks' in ``wd``."""
    path = os.path.join(wd, sid + '.networks')
    write_csv(path, label, table, pc, level, component_types)
    return path
