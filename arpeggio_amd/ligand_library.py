"""A ligand library on a resident receptor: host side of ``Context.library_contacts`` (arp_library_*, csrc/arp_library.h).

``poses`` moves ONE ligand that is part of the resident structure.  A screen is the other case: many different molecules, each
with a few poses, against one receptor.  The receptor is resident alone; the ligands' per-atom facts are a table beside it
(``pack``), and one launch walks every (ligand, pose).

A ligand is a ``PackedComplex`` of ONE residue that is no polypeptide residue and has no sequence neighbours (peptide ligands
and covalent ligands are out of scope).  ``library_contacts`` reads its atoms, hydrogens and single-bond neighbours;
``library_planes`` reads the atoms of its rings and amides as well (``ring_atoms`` in ring-path order, ``amide_atoms``), never
their geometry: that is made per pose.

A library (``pack``) is a dict:

    atom_off   int32 [L + 1]    CSR over the ligands: library atoms atom_off[l] ... atom_off[l + 1] - 1 are ligand l's
    type_mask, flags  uint16 [TA];  vdw, cov  float64 [TA]
    h_off      int32 [TA + 1]   the hydrogen rows of every library atom, CSR over all of them
    sb_nbr     int32 [TA]       the index WITHIN ITS LIGAND of the single-bond heavy neighbour, -1: none
    ligands    the packs it was made from (labels for ``to_records`` / ``write_csv``)

and the plane table of ``Context.set_ligand_library_planes`` (indices WITHIN THE LIGAND; empty ranges for a ligand without):

    ring_off       int32 [L + 1]    CSR over the ligands: rings ring_off[l] ... ring_off[l + 1] - 1 are ligand l's, TR in all
    ring_atom_off  int32 [TR + 1];  ring_atom_idx  int32, every ring in ring-path order
    amide_off      int32 [L + 1];   amide_atoms    int32 [TM, 4]: N, C, O, C-alpha (the fourth is not read, may be -1)

A planes result (``Context.library_planes``) is a dict with one sub-table per ring / amide bag — the columns ``Context.fetch_bag``
gives that bag plus ``pose_off`` uint64 [T + 1] —, ``summary`` uint32 [T, 16] (``poses.PLANE_SUMMARY_SLOTS``) and
``ligand_pose_off``.  Its ids are those of the complex (``complex_of``): ligand atom n + a, ring n_rings + q, amide n_amides + g.

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
from . import poses as _poses
from .poses import N_BITS, SUMMARY, join_poses, n_poses, pose_of, summarise      # (a library result is read as a poses result is)

MAX_LIGANDS = 1 << 16
MAX_ATOMS = 256
MAX_WEIGHT = 1 << 24
INT64_MIN = -(1 << 63)
COLUMNS = ('i', 'a', 'dist', 'sift', 'ctype')
DTYPES = dict(i=np.int32, a=np.int32, dist=np.float32, sift=np.uint16, ctype=np.uint8)
ARRAYS = ('atom_off', 'type_mask', 'flags', 'vdw', 'cov', 'h_off', 'sb_nbr')
PLANE_ARRAYS = ('ring_off', 'ring_atom_off', 'ring_atom_idx', 'amide_off', 'amide_atoms')
PLANES_MAX_RINGS = 32            # ARP_LIBRARY_PLANES_MAX_RINGS: rings of one ligand
PLANES_MAX_AMIDES = 32           # ARP_LIBRARY_PLANES_MAX_AMIDES


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


def validate_planes(lib):
    """What arp_set_ligand_library_planes refuses, in its order and with its causes, checked on the host (ValueError)."""
    L = len(np.asarray(lib['atom_off'])) - 1
    for k in PLANE_ARRAYS:
        if lib.get(k) is None:
            raise ValueError(f'library planes: an array is missing ({k})')
    ro, rao, ao = (np.asarray(lib[k], np.int64) for k in ('ring_off', 'ring_atom_off', 'amide_off'))
    for k, off, n in (('ring_off', ro, L), ('ring_atom_off', rao, int(ro[-1]) if ro.shape == (L + 1,) and (np.diff(ro) >= 0).all() else None),
                      ('amide_off', ao, L)):
        if n is None or off.shape != (n + 1,) or off[0] != 0 or (np.diff(off) < 0).any():
            raise ValueError(f'library planes: {k} must start at 0 and never decrease (one entry per ' + ('ring' if k == 'ring_atom_off' else 'ligand') + ', and the total)')
    idx, am = np.asarray(lib['ring_atom_idx'], np.int64), np.asarray(lib['amide_atoms'], np.int64).reshape(-1, 4)
    if idx.shape != (int(rao[-1]),) or len(am) != int(ao[-1]):
        raise ValueError('library planes: ring_atom_idx must hold ring_atom_off[-1] entries and amide_atoms amide_off[-1] rows of 4')
    if (np.diff(ro) > PLANES_MAX_RINGS).any():
        raise ValueError('library planes: a ligand has more than PLANES_MAX_RINGS rings')
    if (np.diff(ao) > PLANES_MAX_AMIDES).any():
        raise ValueError('library planes: a ligand has more than PLANES_MAX_AMIDES amides')
    if (np.diff(rao) < 3).any():
        raise ValueError('library planes: a ring needs at least three atoms')
    S = np.diff(np.asarray(lib['atom_off'], np.int64))
    s_idx = np.repeat(np.repeat(S, np.diff(ro)), np.diff(rao))
    if ((idx < 0) | (idx >= s_idx)).any():
        raise ValueError('library planes: ring atom index outside its own ligand')
    s_am = np.repeat(S, np.diff(ao))[:, None]
    if len(am) and ((am[:, :3] < 0) | (am[:, :3] >= s_am)).any():
        raise ValueError('library planes: amide atom index outside its own ligand')
    return lib


def _plane_atoms(pc):
    """``(ring paths, amide rows [A, 4])`` of a ligand pack: the rings it names atoms for, the amides whose N, C and O it names."""
    rings = [np.asarray(a, np.int32).reshape(-1) for a in (pc.ring_atoms or [])]
    am = np.asarray(pc.amide_atoms, np.int32).reshape(-1, 4)
    return rings, am[(am[:, :3] >= 0).all(axis=1)]


def pack(ligands):
    """The library arrays of ``ligands`` (PackedComplex each), with the plane table made from the packs' ``ring_atoms`` and
    ``amide_atoms`` (a pack without them gives empty ranges).  Refused (ValueError, the cause named): no ligand or too many; a
    pack with more than one residue; a polypeptide residue or one with sequence neighbours; a ligand with no atom or more than
    ``MAX_ATOMS``; and what ``validate`` and ``validate_planes`` refuse."""
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
    planes = [_plane_atoms(pc) for pc in ligands]
    rings = [a for r, _ in planes for a in r]
    lib.update(ring_off=np.concatenate([[0], np.cumsum([len(r) for r, _ in planes])]).astype(np.int32),
               ring_atom_off=np.concatenate([[0], np.cumsum([len(a) for a in rings])]).astype(np.int32),
               ring_atom_idx=(np.concatenate(rings) if rings else np.zeros(0)).astype(np.int32),
               amide_off=np.concatenate([[0], np.cumsum([len(a) for _, a in planes])]).astype(np.int32),
               amide_atoms=np.concatenate([a for _, a in planes]).astype(np.int32).reshape(-1, 4))
    return validate_planes(validate(lib))


def n_ligands(lib):
    return len(lib['atom_off']) - 1


def sizes(lib):
    """``(S int64 [L], SH int64 [L])``: atoms and hydrogen rows of every ligand."""
    off, h = np.asarray(lib['atom_off'], np.int64), np.asarray(lib['h_off'], np.int64)
    return np.diff(off), h[off[1:]] - h[off[:-1]]


def host_plane_geometry(xyz, ring_atoms, amide_atoms):
    """Ring centres and unit normals (float64) and amide centres and normals (float32) of ``xyz`` in NumPy, by the formulas of
    the geometry kernels: what a ligand pack carries so that it is a consistent pack.  No result depends on these values — the
    device makes a pose's geometry itself."""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    rc, rn = np.zeros((len(ring_atoms), 3)), np.zeros((len(ring_atoms), 3))
    for k, a in enumerate(ring_atoms):
        p = x[np.asarray(a, np.int64)]
        rc[k] = p.mean(axis=0)
        v = np.cross(p - rc[k], np.roll(p, -1, axis=0) - rc[k]).sum(axis=0) / len(p)
        rn[k] = v / np.linalg.norm(v) if np.linalg.norm(v) >= 2e-6 else v
    am = np.asarray(amide_atoms, np.int64).reshape(-1, 4)
    N, Cc, O = x[am[:, 0]], x[am[:, 1]], x[am[:, 2]]
    m = (Cc + O + N) / 3.0
    v = np.cross(Cc - m, O - m)
    l = np.linalg.norm(v, axis=1, keepdims=True)
    return rc, rn, ((Cc + N) / 2.0).astype(np.float32), np.where(l > 0, v / np.where(l > 0, l, 1.0), v).astype(np.float32)


def from_residue(pc, r, planes=False):
    """Residue ``r`` of ``pc`` cut out as a ligand: its atoms in packed order with their hydrogens, bonds and single-bond
    neighbours re-indexed, its labels.  Refused when the residue has a bond to another residue.  ``planes``: keep the residue's
    rings and amides (``ring_atoms`` / ``amide_atoms`` re-indexed, their geometry taken over); refused when a ring or an amide
    (its N, C or O) shares atoms with another residue.  Without it: no rings and no amides."""
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
    ring_kw = dict(ring_center=np.zeros((0, 3)), ring_normal=np.zeros((0, 3)), ring_res=np.zeros(0, np.int32))
    if planes:
        if pc.n_rings and len(pc.ring_atoms) != pc.n_rings:
            raise ValueError('from_residue: planes=True needs the atoms of every ring (ring_atoms)')
        inside = [pos[np.asarray(a, np.int64)] >= 0 for a in pc.ring_atoms]
        if any(m.any() and not m.all() for m in inside):
            raise ValueError(f'from_residue: a ring of residue {r} shares atoms with another residue')
        keep = [k for k, m in enumerate(inside) if m.all()]
        am = np.asarray(pc.amide_atoms, np.int64).reshape(-1, 4)
        known = (am[:, :3] >= 0).all(axis=1) if len(am) else np.zeros(0, bool)
        ins = (pos[np.maximum(am[:, :3], 0)] >= 0) & known[:, None] if len(am) else np.zeros((0, 3), bool)
        if (ins.any(axis=1) & ~ins.all(axis=1)).any():
            raise ValueError(f'from_residue: an amide of residue {r} shares atoms with another residue')
        ka = np.nonzero(ins.all(axis=1))[0]
        ring_kw = dict(ring_center=pc.ring_center[keep], ring_normal=pc.ring_normal[keep], ring_res=np.zeros(len(keep), np.int32),
                       ring_atoms=[pos[np.asarray(pc.ring_atoms[k], np.int64)].astype(np.int32) for k in keep],
                       amide_center=pc.amide_center[ka], amide_normal=pc.amide_normal[ka], amide_res=np.zeros(len(ka), np.int32),
                       amide_atoms=np.where(am[ka] >= 0, pos[np.maximum(am[ka], 0)], -1).astype(np.int32).reshape(-1, 4))
    return PackedComplex(
        xyz=pc.xyz[idx], vdw=pc.vdw[idx], cov=pc.cov[idx], type_mask=pc.type_mask[idx], flags=pc.flags[idx], res_id=np.zeros(len(idx), np.int32),
        res_flags=pc.res_flags[r:r + 1], res_prev=[-1], res_next=[-1],
        bond_off=np.concatenate([[0], np.cumsum([len(b) for b in bonds])]), bond_idx=pos[np.concatenate(bonds)] if bonds else [],
        h_off=np.concatenate([[0], np.cumsum([len(h) for h in hrows])]), h_xyz=np.asarray(pc.h_xyz).reshape(-1, 3)[np.concatenate(hrows).astype(np.int64)],
        sb_nbr=np.where(nbr >= 0, pos[np.maximum(nbr, 0)], -1), **ring_kw,
        atom_name=[pc.atom_name[i] for i in idx], element=[pc.element[i] for i in idx], serial=np.asarray(pc.serial)[idx],
        res_name=[rn], res_seq=[int(pc.res_seq[r])], res_icode=[pc.res_icode[r]], res_chain=[pc.res_chain[r]],
        component_types={rn: pc.component_types.get(rn, 'B')}, id=f'{pc.id}:{rn}{int(pc.res_seq[r])}')


def complex_of(receptor, ligand, xyz=None, h_xyz=None):
    """The complex of the contract: ``receptor`` with ``ligand`` appended after its last atom as one more residue
    (``batch.concat_complexes([receptor, ligand])[0]``, to be uploaded as ONE structure), with the pose ``xyz`` float32 [S, 3] /
    ``h_xyz`` float64 [SH, 3] in place of the ligand's own coordinates when given.  The ligand's atoms are the ids
    ``receptor.n_atoms + a``.  The ligand's ``ring_atoms`` and ``amide_atoms`` are carried into the complex, shifted by
    ``receptor.n_atoms`` and appended after the receptor's: ring ``receptor.n_rings + q``, amide ``receptor.n_amides + g``.  The
    ligand's ring and amide GEOMETRY is carried as the pack has it (for its home coordinates): whoever evaluates the complex
    makes the planes of the pose (``initialize()``, the device).  Refused (ValueError) when the receptor or the ligand names
    the atoms of some of its rings only.  The complex also carries the LABELS of both packs, the receptor's first — atom
    names, elements, serials, residue names, numbers, insertion codes and chains (``ensure_labels`` gives either pack its
    defaults first) — and the union of their ``component_types``; where both name a component, the receptor's type holds."""
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
    n = receptor.n_atoms
    if receptor.ring_atoms or ligand.ring_atoms:
        if len(receptor.ring_atoms) != receptor.n_rings or len(ligand.ring_atoms) != ligand.n_rings:
            raise ValueError('complex_of: ring_atoms must name the atoms of every ring of the receptor and of the ligand, or of none')
        both.ring_atoms = [np.asarray(a, np.int32) for a in receptor.ring_atoms] + [np.asarray(a, np.int32) + n for a in ligand.ring_atoms]
    la = np.asarray(ligand.amide_atoms, np.int32).reshape(-1, 4)
    both.amide_atoms = np.concatenate([np.asarray(receptor.amide_atoms, np.int32).reshape(-1, 4), np.where(la >= 0, la + n, la)]).astype(np.int32)
    # the labels of both (the writers of the planes tables name entities of the complex)
    receptor.ensure_labels()
    ligand.ensure_labels()
    for k in ('atom_name', 'element', 'res_name', 'res_icode', 'res_chain'):
        setattr(both, k, list(getattr(receptor, k)) + list(getattr(ligand, k)))
    both.serial = np.concatenate([np.asarray(receptor.serial), np.asarray(ligand.serial)]).astype(np.int32)
    both.res_seq = np.concatenate([np.asarray(receptor.res_seq), np.asarray(ligand.res_seq)]).astype(np.int32)
    both.component_types = {**ligand.component_types, **receptor.component_types}
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


# ---------------------------------------------------------------------------------------------------------------------
# Ring and amide contacts of the library's poses: host side of ``Context.library_planes`` (arp_library_planes_*,
# csrc/arp_library_planes.h).  The tables are laid out as those of ``Context.poses_planes``: the helpers of ``poses`` serve.
# ---------------------------------------------------------------------------------------------------------------------
PLANE_TABLES = _poses.PLANE_TABLES
plane_columns = _poses.plane_columns


def affected_rings(receptor, xyz_pose):
    """The RECEPTOR rings one pose affects, ascending ids: a ligand atom lies within 3.0 A (inclusive, float64 sum of squares)
    of the ring's resident centre at its pose coordinate ``xyz_pose`` [S, 3].  (A library ligand has no resident coordinate: the
    "or at home" clause of ``poses.affected`` does not exist here.  The ligand's own rings are always affected.)"""
    if receptor.n_rings == 0:
        return np.zeros(0, np.int64)
    x = np.asarray(xyz_pose, np.float32).reshape(-1, 3).astype(np.float64)
    ctr = np.asarray(receptor.ring_center, np.float64).reshape(-1, 3)
    return np.nonzero((_poses._kd2(ctr, x) <= 9.0).any(axis=1))[0].astype(np.int64)


def plane_reference_rows(bags, receptor, ligand, xyz_pose):
    """Of the four ring / amide bags of a pass over the complex of one pose (``complex_of``, the ligand selected): the rows that
    involve an affected entity — a ligand atom, ring or amide, or a receptor ring of ``affected_rings`` —, each bag in its
    canonical order: what the pose's records must equal.  ``receptor`` carries the resident ring centres."""
    n, nr, na = receptor.n_atoms, receptor.n_rings, receptor.n_amides
    m = np.zeros(n + ligand.n_atoms, bool)
    m[n:] = True
    rg = np.zeros(nr + ligand.n_rings, bool)
    rg[nr:] = True
    rg[affected_rings(receptor, xyz_pose)] = True
    am = np.zeros(na + ligand.n_amides, bool)
    am[na:] = True
    keep = {'atom_plane': lambda b: m[b['atom']] | rg[b['ring']], 'plane_plane': lambda b: rg[b['bgn']] | rg[b['end']],
            'group_group': lambda b: am[b['bgn']] | am[b['end']], 'group_plane': lambda b: am[b['amide']] | rg[b['ring']]}
    out = {}
    for name in PLANE_TABLES:
        b = {c: np.asarray(bags[name][c]) for c, _ in plane_columns(name)}
        first, second = _poses.PLANE_ORDER[name]
        k = keep[name](b) if len(b[first]) else np.zeros(0, bool)
        order = np.lexsort((b[second][k], b[first][k]))
        out[name] = {c: b[c][k][order].astype(dt) for c, dt in plane_columns(name)}
    return out


def planes_from_rows(rows, summary=None):
    """``rows``: per ligand a list of per-pose ``plane_reference_rows`` results; the table the device must return for them
    (summary slots 12 - 14 from ``summary`` when given, else 0)."""
    flat = [r for lig in rows for r in lig]
    t = _poses.planes_from_rows(flat, (), summary)
    del t['movable']
    t['ligand_pose_off'] = np.concatenate([[0], np.cumsum([len(lig) for lig in rows])]).astype(np.int64)
    return t


def empty_planes(n_lig, ligand_pose_off=None):
    lo = np.zeros(n_lig + 1, np.int64) if ligand_pose_off is None else np.asarray(ligand_pose_off, np.int64)
    t = _poses.empty_planes(int(lo[-1]))
    del t['movable']
    t['ligand_pose_off'] = lo
    return t


def split_planes(table):
    """Per ligand, per pose: a list of L lists of dicts of four bags."""
    per = _poses.split_planes(table)
    lo = np.asarray(table['ligand_pose_off'], np.int64)
    return [per[lo[l]:lo[l + 1]] for l in range(len(lo) - 1)]


def concat_planes(chunks):
    """The planes results of launches over consecutive ranges of the global poses (``chunk_plan``) as one result."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError('concat_planes: no launch given')
    L = len(chunks[0]['ligand_pose_off'])
    if any(len(c['ligand_pose_off']) != L for c in chunks):
        raise ValueError('concat_planes: the launches are over libraries of different sizes')
    out = _poses.concat_planes([{k: v for k, v in c.items() if k != 'ligand_pose_off'} for c in chunks])
    out.pop('movable', None)
    P = np.sum([np.diff(np.asarray(c['ligand_pose_off'], np.int64)) for c in chunks], axis=0)
    out['ligand_pose_off'] = np.concatenate([[0], np.cumsum(P)]).astype(np.int64)
    if (np.diff(np.concatenate([ligand_of(c) for c in chunks])) < 0).any():
        raise ValueError('concat_planes: the launches are not consecutive ranges of one ligand-major pose sequence')
    return out


CLASS_PLANE = _poses.CLASS_PLANE      # the first class plane of a fingerprint (pose_fingerprints.CLASS_PLANE_NAMES)


def ligand_side(receptor, kind, ids):
    """Which entities of a planes result are the ligand's (bool, the shape of ``ids``): ids are the complex's, so an atom with id
    >= ``receptor.n_atoms``, a ring with id >= ``n_rings`` or an amide with id >= ``n_amides`` (``kind``: 'atom', 'ring',
    'amide').  Everything else is the receptor's, a receptor ring a pose affects included."""
    if kind not in ('atom', 'ring', 'amide'):
        raise ValueError("ligand_side: kind must be 'atom', 'ring' or 'amide'")
    n = dict(atom=receptor.n_atoms, ring=receptor.n_rings, amide=receptor.n_amides)[kind]
    return np.asarray(ids, np.int64) >= n


def plane_fingerprints(planes_table, receptor, ctype_mask=0x7F):
    """The host route to the class planes of the library fingerprints, over a fetched ``Context.library_planes`` table: per global
    pose the set of ``(node, plane)`` — plane 15 ... 28 as ``pose_fingerprints.CLASS_PLANE_NAMES`` numbers them — of the records
    whose ``ctype`` bit is in ``ctype_mask`` and of whose two entities exactly one is the ligand's (``ligand_side``).  The node
    is the residue of the receptor entity: ``res_id`` of an atom, ``amide_res`` of an amide and the RESIDENT ``ring_res`` of a
    ring, all of ``receptor`` alone (``poses.plane_fingerprints`` takes the first atom of the ring path instead: there the
    ligand is part of the structure and can have taken the ring's residue over).  A node outside [0, n_residues) is skipped.
    Returns a list of T sets."""
    res_id = np.asarray(receptor.res_id, np.int64).reshape(-1)
    ring_res = np.asarray(receptor.ring_res, np.int64).reshape(-1)
    am_res = np.asarray(receptor.amide_res, np.int64).reshape(-1)
    T = len(planes_table['summary'])
    out = [set() for _ in range(T)]

    def at(table, ids, lig):      # the residue of the receptor entities among ids (0 stands in where the ligand's are)
        ids = np.where(lig, 0, ids)
        return table[ids] if len(table) else np.full(ids.shape, -1, np.int64)

    def add(name, keep, node, plane):
        off = np.asarray(planes_table[name]['pose_off']).astype(np.int64)
        pose = np.repeat(np.arange(T), np.diff(off))
        ct = np.asarray(planes_table[name]['ctype']).astype(np.int64)
        keep = keep & (((int(ctype_mask) >> np.minimum(ct, 31)) & 1) != 0) & (ct < 7) & (node >= 0) & (node < receptor.n_residues)
        for t, u, q in zip(pose[keep].tolist(), node[keep].tolist(), np.broadcast_to(plane, keep.shape)[keep].tolist()):
            out[t].add((u, q))

    b = planes_table['atom_plane']
    a, r, mask = np.asarray(b['atom'], np.int64), np.asarray(b['ring'], np.int64), np.asarray(b['mask'], np.int64)
    la, lr = ligand_side(receptor, 'atom', a), ligand_side(receptor, 'ring', r)
    for bit in range(5 if len(a) else 0):
        add('atom_plane', (la != lr) & (((mask >> bit) & 1) != 0), np.where(la, at(ring_res, r, lr), at(res_id, a, la)),
            np.where(la, CLASS_PLANE + bit, CLASS_PLANE + 5 + bit))
    b = planes_table['plane_plane']
    r1, r2 = np.asarray(b['bgn'], np.int64), np.asarray(b['end'], np.int64)
    if len(r1):
        l1, l2 = ligand_side(receptor, 'ring', r1), ligand_side(receptor, 'ring', r2)
        add('plane_plane', l1 != l2, np.where(l1, at(ring_res, r2, l2), at(ring_res, r1, l1)), CLASS_PLANE + 10)
    b = planes_table['group_group']
    a1, a2 = np.asarray(b['bgn'], np.int64), np.asarray(b['end'], np.int64)
    if len(a1):
        l1, l2 = ligand_side(receptor, 'amide', a1), ligand_side(receptor, 'amide', a2)
        add('group_group', l1 != l2, np.where(l1, at(am_res, a2, l2), at(am_res, a1, l1)), CLASS_PLANE + 11)
    b = planes_table['group_plane']
    a, r = np.asarray(b['amide'], np.int64), np.asarray(b['ring'], np.int64)
    if len(a):
        la, lr = ligand_side(receptor, 'amide', a), ligand_side(receptor, 'ring', r)
        add('group_plane', la != lr, np.where(la, at(ring_res, r, lr), at(am_res, a, la)), np.where(la, CLASS_PLANE + 12, CLASS_PLANE + 13))
    return out


def _planes_per_pose(table, receptor, ligands):
    """(ligand, pose within it, the complex the ids are of, the pose's four bags) for every global pose."""
    both = {}
    for l, per in enumerate(split_planes(table)):
        for p, bags in enumerate(per):
            if l not in both:
                both[l] = complex_of(receptor, ligands[l])
                both[l].ensure_labels()
            yield l, p, both[l], bags


def planes_to_records(table, receptor, ligands, component_types=None):
    """The records as the dicts ``get_contacts`` returns for the four bags (export.py), each with its 'ligand' and 'pose' (the
    pose within the ligand).  Entities are labelled from the complex of the ligand (``complex_of``)."""
    from .core import export
    out = []
    for l, p, both, bags in _planes_per_pose(table, receptor, ligands):
        for rec in export.contacts_json(both, bags, {**both.component_types, **(component_types or {})}):
            rec['ligand'], rec['pose'] = l, p
            out.append(rec)
    return out


PLANES_CSV_HEADER = ['ligand'] + _poses.PLANES_CSV_HEADER


def write_planes_csv(path, table, receptor, ligands, component_types=None):
    """One row per record: ligand, pose within the ligand, then the columns of ``poses.write_planes_csv`` — bag, the two entities
    ('A/508/O' for an atom, 'ring/<id>' and 'amide/<id>' with the complex's ids), distance, contacts, interacting entities."""
    from .core import export
    labs = {}
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(PLANES_CSV_HEADER)
        for l, p, both, bags in _planes_per_pose(table, receptor, ligands):
            if l not in labs:
                labs[l] = export.Labels(both, {**both.component_types, **(component_types or {})})
            for row in _poses.planes_csv_rows(labs[l], bags):
                w.writerow([l, p] + row)


def write_library_planes(wd, sid, table, receptor, ligands, component_types=None):
    """'<id>.libraryplanes' in ``wd``."""
    path = os.path.join(wd, sid + '.libraryplanes')
    write_planes_csv(path, table, receptor, ligands, component_types)
    return path
