"""Ligand poses on a resident receptor: host side of ``Context.poses_contacts`` (arp_poses_contacts_*, csrc/arp_poses.h).

Docking and virtual screening keep the receptor fixed and move the ligand thousands of times; what is wanted of each placement
is its protein - ligand interaction fingerprint.  The uploaded selection names the MOVABLE SET — the ligand's atoms, hydrogen
atoms included if the structure has them as atoms —; a pose is new coordinates for those atoms and for the hydrogen rows of
those atoms, and the device answers with every pose's ligand - receptor atom-atom records, exactly those of a pass over the
structure with the pose scattered in.

A result (``table``) is a dict:

    i, j, dist, sift, ctype   the records' columns, in ascending (pose, i, j); i < j are packed atom ids
    pose_off   uint64 [P + 1]  the records of pose p are [pose_off[p], pose_off[p + 1])
    summary    uint32 [P, 16]  per pose: records with SIFt bit k (config.SIFT_NAMES) in slot k, all its records in slot 15
    movable    int32 [S]       the movable set

Everything here is NumPy on the host; nothing imports the native library.
"""
import csv
import os

import numpy as np

from .core import config

N_BITS = 15
SUMMARY = 16
COLUMNS = ('i', 'j', 'dist', 'sift', 'ctype')
DTYPES = dict(i=np.int32, j=np.int32, dist=np.float32, sift=np.uint16, ctype=np.uint8)


def _mask(pc, sel):
    """``sel`` as a boolean mask over the atoms: a bool / uint8 array of n entries is a mask, any other integer array lists ids."""
    a = np.asarray(sel)
    n = pc.n_atoms
    if a.dtype == np.bool_ or a.dtype == np.uint8:
        if a.shape != (n,):
            raise ValueError('poses: a selection mask needs one entry per atom')
        return a.astype(bool)
    m = np.zeros(n, bool)
    m[a.astype(np.int64)] = True
    return m


def movable(pc, sel):
    """The movable set of selection ``sel`` (mask or atom ids): ``(atoms, h_rows)`` — the selected packed atom ids, ascending
    (the order of a pose's ``xyz``), and the rows of ``pc.h_xyz`` whose parent atom is selected, ascending (the order of a
    pose's ``h_xyz``)."""
    m = _mask(pc, sel)
    atoms = np.nonzero(m)[0].astype(np.int64)
    owner = np.repeat(np.arange(pc.n_atoms), np.diff(np.asarray(pc.h_off, np.int64)))
    return atoms, np.nonzero(m[owner])[0].astype(np.int64)


def as_models(pc, sel, xyz, h_xyz):
    """The poses as whole models of ``pc``'s topology: ``(X float32 [P, n, 3], H float64 [P, nh, 3])`` with the pose's
    coordinates scattered into the resident ones.  The bridge to the ensemble route (``EnsembleComplex``,
    ``Context.set_models``), which evaluates every pose as a model of its own."""
    atoms, rows = movable(pc, sel)
    x = np.asarray(xyz, np.float32)
    h = np.zeros((len(x), 0, 3)) if h_xyz is None else np.asarray(h_xyz, np.float64)
    if x.ndim != 3 or x.shape[1:] != (len(atoms), 3) or h.shape != (len(x), len(rows), 3):
        raise ValueError(f'as_models: xyz must be [P, {len(atoms)}, 3] and h_xyz [P, {len(rows)}, 3]')
    X = np.repeat(np.asarray(pc.xyz, np.float32)[None], len(x), axis=0)
    H = np.repeat(np.asarray(pc.h_xyz, np.float64).reshape(-1, 3)[None], len(x), axis=0)
    X[:, atoms] = x
    H[:, rows] = h
    return X, H


def n_poses(table):
    return len(table['pose_off']) - 1


def pose_of(table):
    """The pose of every record (int64 [k])."""
    return np.repeat(np.arange(n_poses(table)), np.diff(np.asarray(table['pose_off']).astype(np.int64)))


def empty(n=0, movable_atoms=()):
    """A result of ``n`` poses without records."""
    t = {k: np.zeros(0, DTYPES[k]) for k in COLUMNS}
    t['pose_off'] = np.zeros(n + 1, np.uint64)
    t['summary'] = np.zeros((n, SUMMARY), np.uint32)
    t['movable'] = np.asarray(movable_atoms, np.int32)
    return t


def summarise(sift):
    """The summary row of one pose's records: per SIFt bit, then the total (what the device writes)."""
    s = np.asarray(sift, np.uint16)
    return np.array([int(((s >> k) & 1).sum()) for k in range(N_BITS)] + [len(s)], np.uint32)


def split(table):
    """One result per pose (a list of P dicts of the five columns)."""
    off = np.asarray(table['pose_off']).astype(np.int64)
    return [{k: np.asarray(table[k])[off[p]:off[p + 1]] for k in COLUMNS} for p in range(len(off) - 1)]


def concat(chunks):
    """The results of consecutive chunks of poses as one: the poses of a chunk follow those of the chunks before it."""
    chunks = list(chunks)
    if not chunks:
        return empty()
    out = {k: np.concatenate([np.asarray(c[k]) for c in chunks]) for k in COLUMNS}
    base, offs = 0, [np.zeros(1, np.uint64)]
    for c in chunks:
        o = np.asarray(c['pose_off']).astype(np.uint64)
        offs.append(o[1:] + np.uint64(base))
        base += int(o[-1])
    out['pose_off'] = np.concatenate(offs)
    out['summary'] = np.concatenate([np.asarray(c['summary'], np.uint32).reshape(-1, SUMMARY) for c in chunks])
    mv = [np.asarray(c['movable']) for c in chunks if 'movable' in c]
    if mv:
        if any(not np.array_equal(mv[0], m) for m in mv[1:]):
            raise ValueError('concat: the chunks have different movable sets')
        out['movable'] = mv[0]
    return out


def partners(table):
    """Per record ``(ligand atom, receptor atom)``: which of i / j is in the movable set."""
    mv = np.asarray(table['movable'])
    i, j = np.asarray(table['i']), np.asarray(table['j'])
    i_moves = np.isin(i, mv)
    return np.where(i_moves, i, j), np.where(i_moves, j, i)


def fingerprints(table, pc, level='residue'):
    """The interaction fingerprint of every pose: ``(bits bool [P, R, 15], ids int [R])`` — ``bits[p, r, k]``: pose p has a
    record with SIFt bit k (``config.SIFT_NAMES``) to receptor residue ``ids[r]`` (``level='atom'``: receptor atom); ``ids``
    are the receptor residues (atoms) that occur in any pose, ascending."""
    if level not in ('residue', 'atom'):
        raise ValueError("fingerprints: level must be 'residue' or 'atom'")
    _, rec = partners(table)
    node = np.asarray(pc.res_id)[rec] if level == 'residue' else rec
    ids, col = np.unique(node, return_inverse=True)
    P = n_poses(table)
    bits = np.zeros((P, len(ids), N_BITS), bool)
    pose = pose_of(table)
    s = np.asarray(table['sift'], np.uint16)
    for k in range(N_BITS):
        on = ((s >> k) & 1).astype(bool)
        bits[pose[on], col[on], k] = True
    return bits, ids


def to_records(table, pc, component_types=None):
    """The records as the list of dicts ``get_contacts`` returns for atom-atom contacts (export.py), each with its 'pose'."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    ct = config.CONTACT_TYPE_NAMES
    pose = pose_of(table).tolist()
    return [{'pose': p, 'bgn': lab.atom_dict(i), 'end': lab.atom_dict(j), 'type': 'atom-atom', 'distance': d,
             'contact': [n for k, n in enumerate(config.SIFT_NAMES) if (s >> k) & 1], 'interacting_entities': ct[c]}
            for p, i, j, d, s, c in zip(pose, np.asarray(table['i']).tolist(), np.asarray(table['j']).tolist(), export.rounded(table['dist']),
                                        np.asarray(table['sift']).tolist(), np.asarray(table['ctype']).tolist())]


CSV_HEADER = ['pose', 'atom_bgn', 'atom_end', 'distance', 'contacts', 'interacting_entities']


def write_csv(path, table, pc, component_types=None):
    """One row per record: pose, the two atoms in the form the other CSV tables use ('A/508/O'), the distance rounded as
    ``get_contacts`` rounds it, the contacts by name joined with '|', the interacting entities."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    ct = config.CONTACT_TYPE_NAMES
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for p, i, j, d, s, c in zip(pose_of(table).tolist(), np.asarray(table['i']).tolist(), np.asarray(table['j']).tolist(),
                                    export.rounded(table['dist']), np.asarray(table['sift']).tolist(), np.asarray(table['ctype']).tolist()):
            w.writerow([p, lab.atom_macro(i), lab.atom_macro(j), d, '|'.join(n for k, n in enumerate(config.SIFT_NAMES) if (s >> k) & 1), ct[c]])


def write_poses(wd, sid, table, pc, component_types=None):
    """'<id>.poses' in ``wd``."""
    path = os.path.join(wd, sid + '.poses')
    write_csv(path, table, pc, component_types)
    return path


def reference_rows(bag, sel_mask):
    """Of an atom-atom bag (a pass over one pose as a whole structure or model) the rows with exactly one selected atom, in
    (i, j) order: what a pose's records must equal."""
    m = np.asarray(sel_mask).astype(bool)
    i, j = np.asarray(bag['i']), np.asarray(bag['j'])
    keep = m[i] != m[j]
    order = np.lexsort((j[keep], i[keep]))
    return {k: np.asarray(bag[k])[keep][order] for k in COLUMNS}
