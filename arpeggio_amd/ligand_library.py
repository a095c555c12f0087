"""A ligand library on a resident receptor: host side of ``Context.library_contacts`` (arp_library_*, csrc/arp_library.h).

``poses`` moves ONE ligand that is part of the resident structure.  A screen is the other case: many different molecules, each
with a few poses, against one receptor.  The receptor is resident alone; the ligands' per-atom facts are a table beside it
(``pack``), and one launch walks every (ligand, pose).

A ligand is a ``PackedComplex`` of ONE residue that is no polypeptide residue and has no sequence neighbours (peptide ligands
and covalent ligands are out of scope); only its atoms, hydrogens and single-bond neighbours are read, its rings and amides are
not (the plane tables of a library are out of scope).

A library (``pack``) is a dict:

    atom_off   int32 [L + 1]    CSR over the ligands: library atoms atom_off[l] ... atom_off[l + 1] - 1 are ligand l's
    type_mask, flags  uint16 [TA];  vdw, cov  float64 [TA]
    h_off      int32 [TA + 1]   the hydrogen rows of every library atom, CSR over all of them
    sb_nbr     int32 [TA]       the index WITHIN ITS LIGAND of the single-bond heavy neighbour, -1: none
    ligands    the packs it was made from (labels for ``to_records`` / ``write_csv``)

A result (``table``) is a dict:

    i, a, dist, sift, ctype   the records' columns in ascending (global pose, i, a): i the receptor's packed id, a the ligand
                              atom's index within its ligand
    pose_off   uint64 [T + 1]   the records of global pose t
    summary    uint32 [T, 16]   per pose: records with SIFt bit k in slot k, all its records in slot 15
    ligand_pose_off  int64 [L + 1]   the global poses of ligand l are [ligand_pose_off[l], ligand_pose_off[l + 1])

Everything here is NumPy on the host; nothing imports the native library.
"""
import copy
import csv
import os

import numpy as np

from .core import config
from .core.packed import PackedComplex
from .poses import N_BITS, SUMMARY, join_poses, n_poses, pose_of, summarise      # (a library result is read as a poses result is)

MAX_LIGANDS = 1 << 16
MAX_ATOMS = 256
MAX_WEIGHT = 1 << 24
INT64_MIN = -(1 << 63)
COLUMNS = ('i', 'a', 'dist', 'sift', 'ctype')
DTYPES = dict(i=np.int32, a=np.int32, dist=np.float32, sift=np.uint16, ctype=np.uint8)
ARRAYS = ('atom_off', 'type_mask', 'flags', 'vdw', 'cov', 'h_off', 'sb_nbr')


def validate(lib):
    """What arp_set_ligand_library refuses, in its order and with its causes, checked on the host (ValueError)."""
    off = np.asarray(lib['atom_off'], np.int64)
    if off.ndim != 1 or not 1 <= len(off) - 1 <= MAX_LIGANDS:
        raise ValueError('ligand library: 1 ... MAX_LIGANDS ligands')
    if off[0] != 0:
        raise ValueError('ligand library: atom_off must start at 0')
    S = np.diff(off)
    if (S < 1).any() or (S > MAX_ATOMS).any():
        raise ValueError('ligand library: atom_off: a ligand must hold 1 ... MAX_ATOMS atoms')
    TA = int(off[-1])
    for k in ('type_mask', 'flags', 'vdw', 'cov', 'sb_nbr'):
        if np.asarray(lib[k]).shape != (TA,):
            raise ValueError(f'ligand library: {k} must hold one entry per library atom')
    h = np.asarray(lib['h_off'], np.int64)
    if h.shape != (TA + 1,):
        raise ValueError('ligand library: h_off must hold one entry per library atom and the total')
    if h[0] != 0:
        raise ValueError('ligand library: h_off must start at 0')
    if (np.diff(h) < 0).any():
        raise ValueError('ligand library: h_off must not decrease')
    vdw, cov = np.asarray(lib['vdw'], np.float64), np.asarray(lib['cov'], np.float64)
    if not (np.isfinite(vdw).all() and np.isfinite(cov).all() and (vdw >= 0).all() and (cov >= 0).all()):
        raise ValueError('ligand library: radii must be finite and not negative')
    nbr = np.asarray(lib['sb_nbr'], np.int64)
    own = np.arange(TA) - np.repeat(off[:-1], S)
    if ((nbr < -1) | (nbr >= np.repeat(S, S)) | (nbr == own)).any():
        raise ValueError('ligand library: sb_nbr must be -1 or the index of another atom of the same ligand')
    return lib


def pack(ligands):
    """The library arrays of ``ligands`` (PackedComplex each).  Refused (ValueError, the cause named): no ligand or too many; a
    pack with more than one residue; a polypeptide residue or one with sequence neighbours; a ligand with no atom or more than
    ``MAX_ATOMS``; and what ``validate`` refuses."""
    ligands = list(ligands)
    if not 1 <= len(ligands) <= MAX_LIGANDS:
        raise ValueError('ligand library: 1 ... MAX_LIGANDS ligands')
    for l, pc in enumerate(ligands):
        if pc.n_residues != 1:
            raise ValueError(f'ligand library: ligand {l} is not one residue (a ligand is one residue of a chain of its own)')
        if int(pc.res_flags[0]) & (config.R_POLYPEPTIDE | config.R_HAS_SEQ) or int(pc.res_prev[0]) >= 0 or int(pc.res_next[0]) >= 0:
            raise ValueError(f'ligand library: ligand {l} is a polypeptide residue or has sequence neighbours (peptide ligands are out of scope)')
        if not 1 <= pc.n_atoms <= MAX_ATOMS:
            raise ValueError(f'ligand library: atom_off: a ligand must hold 1 ... MAX_ATOMS atoms (ligand {l} has {pc.n_atoms})')
    atom_off = np.concatenate([[0], np.cumsum([pc.n_atoms for pc in ligands])]).astype(np.int32)
    hcnt = np.concatenate([np.diff(np.asarray(pc.h_off, np.int64)) for pc in ligands])
    lib = dict(atom_off=atom_off,
               type_mask=np.concatenate([pc.type_mask for pc in ligands]).astype(np.uint16),
               flags=np.concatenate([pc.flags for pc in ligands]).astype(np.uint16),
               vdw=np.concatenate([pc.vdw for pc in ligands]).astype(np.float64),
               cov=np.concatenate([pc.cov for pc in ligands]).astype(np.float64),
               h_off=np.concatenate([[0], np.cumsum(hcnt)]).astype(np.int32),
               sb_nbr=np.concatenate([pc.sb_nbr for pc in ligands]).astype(np.int32),
               ligands=ligands)
    return validate(lib)


def n_ligands(lib):
    return len(lib['atom_off']) - 1


def sizes(lib):
    """``(S int64 [L], SH int64 [L])``: atoms and hydrogen rows of every ligand."""
    off, h = np.asarray(lib['atom_off'], np.int64), np.asarray(lib['h_off'], np.int64)
    return np.diff(off), h[off[1:]] - h[off[:-1]]


def from_residue(pc, r):
    """Residue ``r`` of ``pc`` cut out as a ligand: its atoms in packed order with their hydrogens, bonds and single-bond
    neighbours re-indexed, its labels, no rings and no amides.  Refused when the residue has a bond to another residue."""
    idx = np.nonzero(np.asarray(pc.res_id) == r)[0].astype(np.int64)
    if len(idx) == 0:
        raise ValueError(f'from_residue: residue {r} has no atom')
    pos = np.full(pc.n_atoms, -1, np.int64)
    pos[idx] = np.arange(len(idx))
    bonds = [np.asarray(pc.bond_idx[pc.bond_off[i]:pc.bond_off[i + 1]], np.int64) for i in idx]
    if any((pos[b] < 0).any() for b in bonds):
        raise ValueError(f'from_residue: residue {r} is bonded to another residue (covalent ligands are out of scope)')
    nbr = np.asarray(pc.sb_nbr, np.int64)[idx]
    if ((nbr >= 0) & (pos[np.maximum(nbr, 0)] < 0)).any():
        raise ValueError(f'from_residue: residue {r} has a single-bond neighbour in another residue')
    hrows = [np.arange(pc.h_off[i], pc.h_off[i + 1]) for i in idx]
    pc.ensure_labels()
    rn = pc.res_name[r]
    return PackedComplex(
        xyz=pc.xyz[idx], vdw=pc.vdw[idx], cov=pc.cov[idx], type_mask=pc.type_mask[idx], flags=pc.flags[idx], res_id=np.zeros(len(idx), np.int32),
        res_flags=pc.res_flags[r:r + 1], res_prev=[-1], res_next=[-1],
        bond_off=np.concatenate([[0], np.cumsum([len(b) for b in bonds])]), bond_idx=pos[np.concatenate(bonds)] if bonds else [],
        h_off=np.concatenate([[0], np.cumsum([len(h) for h in hrows])]), h_xyz=np.asarray(pc.h_xyz).reshape(-1, 3)[np.concatenate(hrows).astype(np.int64)],
        sb_nbr=np.where(nbr >= 0, pos[np.maximum(nbr, 0)], -1),
        ring_center=np.zeros((0, 3)), ring_normal=np.zeros((0, 3)), ring_res=np.zeros(0, np.int32),
        atom_name=[pc.atom_name[i] for i in idx], element=[pc.element[i] for i in idx], serial=np.asarray(pc.serial)[idx],
        res_name=[rn], res_seq=[int(pc.res_seq[r])], res_icode=[pc.res_icode[r]], res_chain=[pc.res_chain[r]],
        component_types={rn: pc.component_types.get(rn, 'B')}, id=f'{pc.id}:{rn}{int(pc.res_seq[r])}')


def complex_of(receptor, ligand, xyz=None, h_xyz=None):
    """The complex of the contract: ``receptor`` with ``ligand`` appended after its last atom as one more residue
    (``batch.concat_complexes([receptor, ligand])[0]``, to be uploaded as ONE structure), with the pose ``xyz`` float32 [S, 3] /
    ``h_xyz`` float64 [SH, 3] in place of the ligand's own coordinates when given.  The ligand's atoms are the ids
    ``receptor.n_atoms + a``."""
    from .batch import concat_complexes
    lig = ligand
    if xyz is not None or h_xyz is not None:
        lig = copy.copy(ligand)
        if xyz is not None:
            x = np.ascontiguousarray(xyz, np.float32)
            if x.shape != (ligand.n_atoms, 3):
                raise ValueError(f'complex_of: xyz must be [{ligand.n_atoms}, 3]')
            lig.xyz = x
        if h_xyz is not None:
            h = np.ascontiguousarray(h_xyz, np.float64).reshape(-1, 3)
            if h.shape != (len(ligand.h_xyz), 3):
                raise ValueError(f'complex_of: h_xyz must be [{len(ligand.h_xyz)}, 3]')
            lig.h_xyz = h
    both = concat_complexes([receptor, lig])[0]
    both.id = f'{receptor.id}+{ligand.id}'
    return both


def flatten_poses(lib, poses):
    """``poses``: per ligand ``(xyz [P_l, S_l, 3], h_xyz [P_l, SH_l, 3] or None)``, or None for a ligand without poses.  Returns
    ``(pose_off int64 [L + 1], xyz float32 flat, h_xyz float64 flat)``, ligand-major then pose-major: what a launch takes."""
    S, SH = sizes(lib)
    poses = list(poses)
    if len(poses) != len(S):
        raise ValueError(f'flatten_poses: one entry per ligand of the library ({len(S)}), not {len(poses)}')
    xs, hs, P = [], [], []
    for l, item in enumerate(poses):
        x, h = (None, None) if item is None else item
        x = np.zeros((0, S[l], 3), np.float32) if x is None else np.ascontiguousarray(x, np.float32)
        if x.ndim != 3 or x.shape[1:] != (S[l], 3):
            raise ValueError(f'flatten_poses: xyz of ligand {l} must be [P, {S[l]}, 3]')
        h = np.zeros((len(x), SH[l] if len(x) == 0 else 0, 3)) if h is None else np.ascontiguousarray(h, np.float64)
        if h.shape != (len(x), SH[l], 3):
            raise ValueError(f'flatten_poses: h_xyz of ligand {l} must be [{len(x)}, {SH[l]}, 3]')
        xs.append(x.reshape(-1))
        hs.append(h.reshape(-1))
        P.append(len(x))
    return np.concatenate([[0], np.cumsum(P)]).astype(np.int64), np.concatenate(xs).astype(np.float32), np.concatenate(hs).astype(np.float64)


def ligand_of(table):
    """The ligand of every global pose (int64 [T])."""
    lo = np.asarray(table['ligand_pose_off'], np.int64)
    return np.repeat(np.arange(len(lo) - 1), np.diff(lo))


def empty(n_lig, ligand_pose_off=None):
    lo = np.zeros(n_lig + 1, np.int64) if ligand_pose_off is None else np.asarray(ligand_pose_off, np.int64)
    t = {k: np.zeros(0, DTYPES[k]) for k in COLUMNS}
    t['pose_off'] = np.zeros(int(lo[-1]) + 1, np.uint64)
    t['summary'] = np.zeros((int(lo[-1]), SUMMARY), np.uint32)
    t['ligand_pose_off'] = lo
    return t


def from_rows(rows):
    """``rows``: per ligand a list of per-pose dicts of the five columns; the table the device must return for them."""
    flat = [r for lig in rows for r in lig]
    t = {k: (np.concatenate([np.asarray(r[k]) for r in flat]) if flat else np.zeros(0)).astype(DTYPES[k]) for k in COLUMNS}
    t['pose_off'] = np.concatenate([[0], np.cumsum([len(r['i']) for r in flat])]).astype(np.uint64)
    t['summary'] = np.stack([summarise(r['sift']) for r in flat]) if flat else np.zeros((0, SUMMARY), np.uint32)
    t['ligand_pose_off'] = np.concatenate([[0], np.cumsum([len(lig) for lig in rows])]).astype(np.int64)
    return t


def split(table):
    """Per ligand, per pose: a list of L lists of dicts of the five columns."""
    off = np.asarray(table['pose_off']).astype(np.int64)
    lo = np.asarray(table['ligand_pose_off'], np.int64)
    return [[{k: np.asarray(table[k])[off[t]:off[t + 1]] for k in COLUMNS} for t in range(lo[l], lo[l + 1])] for l in range(len(lo) - 1)]


def chunk_plan(pose_off, chunk):
    """Consecutive ranges of at most ``chunk`` global poses as launches of their own: a list of ``(pose_off_c int64 [L + 1],
    first global pose, last + 1)``.  A ligand's poses may be cut between two launches."""
    off = np.asarray(pose_off, np.int64)
    T, step = int(off[-1]), max(int(chunk), 1)
    return [(np.clip(off, a, min(a + step, T)) - a, a, min(a + step, T)) for a in range(0, T, step)]


def chunk_poses(lib, pose_off, xyz, h_xyz, chunk):
    """``chunk_plan`` with every launch's coordinates: yields ``(pose_off_c, first global pose, last + 1, xyz_c, h_xyz_c)``, the
    flat arrays of ``flatten_poses`` cut to the global poses of the range — of every ligand its poses inside it."""
    off = np.asarray(pose_off, np.int64)
    x, h = np.asarray(xyz).reshape(-1), np.asarray(h_xyz).reshape(-1)
    S, SH = sizes(lib)
    x_at = np.concatenate([[0], np.cumsum(np.diff(off) * S * 3)])
    h_at = np.concatenate([[0], np.cumsum(np.diff(off) * SH * 3)])
    for off_c, a, b in chunk_plan(off, chunk):
        first = np.clip(off, a, b) - off                       # (how many of the ligand's poses come before the range)
        xs = [x[x_at[l] + first[l] * S[l] * 3:x_at[l] + (first[l] + off_c[l + 1] - off_c[l]) * S[l] * 3] for l in range(len(S))]
        hs = [h[h_at[l] + first[l] * SH[l] * 3:h_at[l] + (first[l] + off_c[l + 1] - off_c[l]) * SH[l] * 3] for l in range(len(S))]
        yield off_c, a, b, np.concatenate(xs), np.concatenate(hs)


def concat(chunks):
    """The results of launches over consecutive ranges of the global poses (``chunk_plan``) as one result."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError('concat: no launch given')
    L = len(chunks[0]['ligand_pose_off'])
    if any(len(c['ligand_pose_off']) != L for c in chunks):
        raise ValueError('concat: the launches are over libraries of different sizes')
    out = {k: np.concatenate([np.asarray(c[k]) for c in chunks]).astype(DTYPES[k]) for k in COLUMNS}
    out['pose_off'], out['summary'] = join_poses(chunks)
    P = np.sum([np.diff(np.asarray(c['ligand_pose_off'], np.int64)) for c in chunks], axis=0)
    out['ligand_pose_off'] = np.concatenate([[0], np.cumsum(P)]).astype(np.int64)
    # consecutive ranges of a ligand-major pose sequence: ligand ids never decrease along the joined poses
    lig = np.concatenate([ligand_of(c) for c in chunks])
    if (np.diff(lig) < 0).any():
        raise ValueError('concat: the launches are not consecutive ranges of one ligand-major pose sequence')
    return out


def best(table, weights):
    """Host mirror of arp_library_best: per ligand ``n_poses`` int64, ``best_pose`` int32 (the global pose of the highest
    score = sum of weights[s] summary[t][s] in int64, ties to the lower id; -1 without poses) and ``score`` int64 (INT64_MIN
    there)."""
    w = np.asarray(weights, np.int64).reshape(-1)
    if w.shape != (SUMMARY,) or (np.abs(w) > MAX_WEIGHT).any():
        raise ValueError('best: weights must be 16 integers with |w| <= MAX_WEIGHT')
    score = (np.asarray(table['summary'], np.uint32).reshape(-1, SUMMARY).astype(np.int64) * w[None, :]).sum(axis=1)
    lo = np.asarray(table['ligand_pose_off'], np.int64)
    L = len(lo) - 1
    out = dict(n_poses=np.diff(lo).astype(np.int64), best_pose=np.full(L, -1, np.int32), score=np.full(L, INT64_MIN, np.int64))
    for l in range(L):
        if lo[l + 1] > lo[l]:
            k = int(np.argmax(score[lo[l]:lo[l + 1]]))      # (the first of equal scores)
            out['best_pose'][l], out['score'][l] = lo[l] + k, score[lo[l] + k]
    return out


def _rows(table, receptor, ligands, component_types):
    from .core import export
    rec = export.Labels(receptor, receptor.component_types if component_types is None else component_types)
    labs = {}
    lig = ligand_of(table)
    lo = np.asarray(table['ligand_pose_off'], np.int64)
    for t, i, a, d, s, c in zip(pose_of(table).tolist(), np.asarray(table['i']).tolist(), np.asarray(table['a']).tolist(),
                                export.rounded(table['dist']), np.asarray(table['sift']).tolist(), np.asarray(table['ctype']).tolist()):
        l = int(lig[t])
        if l not in labs:
            labs[l] = export.Labels(ligands[l], ligands[l].ensure_labels().component_types)
        yield l, t - int(lo[l]), rec, i, labs[l], a, d, [n for k, n in enumerate(config.SIFT_NAMES) if (s >> k) & 1], config.CONTACT_TYPE_NAMES[c]


def to_records(table, receptor, ligands, component_types=None):
    """The records as the dicts ``get_contacts`` returns for atom-atom contacts (export.py), each with its 'ligand' and 'pose'
    (the pose within the ligand).  bgn is the receptor atom; the ligand atom is labelled from the ligand's own pack."""
    return [{'ligand': l, 'pose': p, 'bgn': rec.atom_dict(i), 'end': lab.atom_dict(a), 'type': 'atom-atom', 'distance': d, 'contact': names,
             'interacting_entities': ct} for l, p, rec, i, lab, a, d, names, ct in _rows(table, receptor, ligands, component_types)]


CSV_HEADER = ['ligand', 'pose', 'atom_bgn', 'atom_end', 'distance', 'contacts', 'interacting_entities']


def write_csv(path, table, receptor, ligands, component_types=None):
    """One row per record: ligand, pose within the ligand, the two atoms ('A/508/O'), the distance rounded as ``get_contacts``
    rounds it, the contacts by name joined with '|', the interacting entities."""
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for l, p, rec, i, lab, a, d, names, ct in _rows(table, receptor, ligands, component_types):
            w.writerow([l, p, rec.atom_macro(i), lab.atom_macro(a), d, '|'.join(names), ct])


def write_library(wd, sid, table, receptor, ligands, component_types=None):
    """'<id>.library' in ``wd``."""
    path = os.path.join(wd, sid + '.library')
    write_csv(path, table, receptor, ligands, component_types)
    return path


def reference_rows(bag, n_receptor):
    """Of an atom-atom bag of a pass over the complex (``complex_of``) the rows with one receptor and one ligand atom as the
    library's columns (a = j - n), in (i, a) order: what a pose's records must equal."""
    i, j = np.asarray(bag['i']), np.asarray(bag['j'])
    keep = (i < n_receptor) != (j < n_receptor)
    order = np.lexsort((j[keep], i[keep]))
    out = {k: np.asarray(bag[k])[keep][order] for k in ('i', 'dist', 'sift', 'ctype')}
    out['a'] = (j[keep][order] - n_receptor).astype(np.int32)
    return {k: np.asarray(out[k]).astype(DTYPES[k]) for k in COLUMNS}
