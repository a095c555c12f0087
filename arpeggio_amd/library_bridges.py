"""Host side of the library water bridges (``Context.library_water_bridges`` / ``InteractionComplex.run_library_water_bridges``):
which ligand atom of which pose is tied to which receptor atom through which structural water.

Two results are joined: the library result (``Context.library_contacts``: records (t, i, a) of T global poses) and the atom-atom
bag of a pass over the receptor ALONE with everything selected, same ``cutoff`` and ``vdw_comp``.

  RECEPTOR LEG  a bag record (i, j) with exactly one water atom (``config.F_WATER``) and ``(sift & sift_any) != 0``: the water is
                w, the other atom j (``water_bridges``' leg, unchanged)
  LIGAND LEG    of pose t: a library record (t, i, a) with F_WATER on receptor atom i, NONE on library atom a and a wanted bit;
                the water is w = i

A table is a dict of eight NumPy columns, one row (t, w, a, j) per ligand leg and receptor leg of the same water, ascending by
(pose, water, lig_atom, rec_atom) — no same-residue rule, a ligand is a residue of its own —:

    pose, water, lig_atom, rec_atom    int32    global pose, receptor id of the water, index within the ligand, receptor id
    dist_lig, dist_rec                 float32  the distances of the records (t, w, a) and (w, j)
    sift_lig, sift_rec                 uint16   the whole SIFt of each leg, not masked

and per pose ``bridge_off`` uint64 [T + 1] (row offsets), ``waters`` uint32 [T] (distinct waters with at least one row) and
``legs`` uint32 [T] (the ligand legs, whether or not their water has a receptor leg).  Without any ligand leg or without any
receptor leg the three are all zero.  Contact types are NOT columns: a record's type depends on the selection it was made under
(the ligand for the library record, everything for the receptor's pass), and neither is what a pass over the complex would print
for a bridge.

The yardstick: for pose t of ligand l, ``water_bridges.join`` over the bag of a whole-structure pass on
``ligand_library.complex_of(receptor, ligand_l, pose)``, cut by ``reference_rows``.

Out of scope: bridges through a LIGAND's water atom (a water ligand bridges nothing here), second-order (water-water) bridges,
bridge planes in the library fingerprint, a bridge slot in the shortlist's weights, a pose subset, the pose route.

Everything here is NumPy on the host: no GPU, no native library."""
import csv
import os

import numpy as np

from . import ligand_library as _ll
from . import water_bridges as _wb
from .core import config

COLUMNS = (('pose', np.int32), ('water', np.int32), ('lig_atom', np.int32), ('rec_atom', np.int32), ('dist_lig', np.float32),
           ('dist_rec', np.float32), ('sift_lig', np.uint16), ('sift_rec', np.uint16))
PER_POSE = (('bridge_off', np.uint64), ('waters', np.uint32), ('legs', np.uint32))
DEFAULT_CONTACTS = _wb.DEFAULT_CONTACTS
mask = _wb.mask


def empty(n_poses=0):
    """A table without rows over ``n_poses`` poses."""
    t = {k: np.zeros(0, dt) for k, dt in COLUMNS}
    t.update(bridge_off=np.zeros(int(n_poses) + 1, np.uint64), waters=np.zeros(int(n_poses), np.uint32), legs=np.zeros(int(n_poses), np.uint32))
    return t


def n_poses(table):
    return len(table['bridge_off']) - 1


def _check(table):
    for k, _ in COLUMNS + PER_POSE:
        if k not in table:
            raise ValueError(f'library_bridges: the table has no column {k!r}')
    B = len(table['pose'])
    if any(len(table[k]) != B for k, _ in COLUMNS):
        raise ValueError('library_bridges: the columns differ in length')
    T = n_poses(table)
    off = np.asarray(table['bridge_off']).astype(np.int64)
    if T < 0 or len(table['waters']) != T or len(table['legs']) != T:
        raise ValueError('library_bridges: bridge_off must be [T + 1], waters and legs [T]')
    if off[0] != 0 or off[-1] != B or (np.diff(off) < 0).any():
        raise ValueError('library_bridges: bridge_off must start at 0, not decrease and end at the number of rows')
    return T, off


def join(library_table, receptor_bag, receptor_flags, library, sift_any):
    """The NumPy mirror of the definition: ``library_table`` as ``Context.library_contacts`` returns it, ``receptor_bag`` a dict
    with the columns i, j, dist, sift of a pass over the receptor alone with everything selected (any order of records),
    ``receptor_flags`` the receptor's per-atom flags, ``library`` what ``ligand_library.pack`` made (``atom_off``, ``flags``)."""
    sift_any = _wb._check_mask(sift_any)
    T = len(library_table['pose_off']) - 1
    out = empty(T)
    out['sift_any'] = sift_any
    water = (np.asarray(receptor_flags).astype(np.int64) & config.F_WATER) != 0
    # ---- the receptor's legs, sorted by (water, partner)
    bi, bj = np.asarray(receptor_bag['i']).astype(np.int64), np.asarray(receptor_bag['j']).astype(np.int64)
    wi, wj = water[bi], water[bj]
    rleg = np.nonzero((wi != wj) & ((np.asarray(receptor_bag['sift']).astype(np.int64) & sift_any) != 0))[0]
    rw, rp = np.where(wi[rleg], bi[rleg], bj[rleg]), np.where(wi[rleg], bj[rleg], bi[rleg])
    order = np.lexsort((rp, rw))
    rleg, rw, rp = rleg[order], rw[order], rp[order]
    # ---- the ligand legs, in the table's (t, i, a) order
    li, la = np.asarray(library_table['i']).astype(np.int64), np.asarray(library_table['a']).astype(np.int64)
    t_of = _ll.pose_of(library_table).astype(np.int64)
    first_atom = np.asarray(library['atom_off']).astype(np.int64)[_ll.ligand_of(library_table)[t_of]] if len(t_of) else np.zeros(0, np.int64)
    lig_water = (np.asarray(library['flags']).astype(np.int64)[first_atom + la] & config.F_WATER) != 0
    lleg = np.nonzero(water[li] & ~lig_water & ((np.asarray(library_table['sift']).astype(np.int64) & sift_any) != 0))[0]
    if not len(lleg) or not len(rleg):
        return out
    t, w = t_of[lleg], li[lleg]
    lo, hi = np.searchsorted(rw, w, side='left'), np.searchsorted(rw, w, side='right')
    m = hi - lo
    # ---- one row per ligand leg and receptor leg of its water: leg-major, the water's legs in partner order
    x = np.repeat(np.arange(len(lleg)), m)
    y = np.repeat(lo, m) + np.arange(len(x)) - np.repeat(np.cumsum(m) - m, m)
    out.update(pose=t[x].astype(np.int32), water=w[x].astype(np.int32), lig_atom=la[lleg][x].astype(np.int32), rec_atom=rp[y].astype(np.int32),
               dist_lig=np.asarray(library_table['dist'])[lleg][x].astype(np.float32), dist_rec=np.asarray(receptor_bag['dist'])[rleg][y].astype(np.float32),
               sift_lig=np.asarray(library_table['sift'])[lleg][x].astype(np.uint16), sift_rec=np.asarray(receptor_bag['sift'])[rleg][y].astype(np.uint16))
    out['bridge_off'] = np.concatenate([[0], np.cumsum(np.bincount(t, weights=m, minlength=T).astype(np.int64))]).astype(np.uint64)
    out['legs'] = np.bincount(t, minlength=T).astype(np.uint32)
    pw = np.unique(np.stack([t[m > 0], w[m > 0]], axis=1), axis=0)
    out['waters'] = np.bincount(pw[:, 0], minlength=T).astype(np.uint32)
    return out


def reference_rows(complex_bridge_table, n_receptor):
    """Of the ``water_bridges`` table of a whole-structure pass over a complex (``ligand_library.complex_of``: the ligand's atoms
    are n_receptor + a) the rows in which exactly one partner is a ligand atom and the water is the receptor's, as this
    layout's columns without ``pose``, in (water, lig_atom, rec_atom) order: what a pose's rows must equal."""
    n = int(n_receptor)
    t = complex_bridge_table
    w, a, b = (np.asarray(t[k]).astype(np.int64) for k in ('water', 'a', 'b'))
    keep = ((a >= n) != (b >= n)) & (w < n)
    lig_is_b = (b >= n)[keep]
    pick = lambda ka, kb: np.where(lig_is_b, np.asarray(t[kb])[keep], np.asarray(t[ka])[keep])
    lig, rec = pick('a', 'b').astype(np.int64) - n, pick('b', 'a').astype(np.int64)
    order = np.lexsort((rec, lig, w[keep]))
    cols = dict(water=w[keep], lig_atom=lig, rec_atom=rec, dist_lig=pick('dist_a', 'dist_b'), dist_rec=pick('dist_b', 'dist_a'),
                sift_lig=pick('sift_a', 'sift_b'), sift_rec=pick('sift_b', 'sift_a'))
    return {k: np.asarray(cols[k])[order].astype(dt) for k, dt in COLUMNS if k != 'pose'}


def split(table):
    """Per pose, by ``bridge_off``: a list of T dicts of the eight columns."""
    T, off = _check(table)
    return [{k: np.asarray(table[k])[off[t]:off[t + 1]] for k, _ in COLUMNS} for t in range(T)]


def shift(table, first_pose):
    """The table of a launch over the global poses from ``first_pose`` on, with global pose ids."""
    _check(table)
    if int(first_pose) < 0:
        raise ValueError('library_bridges.shift: first_pose must not be negative')
    out = dict(table)
    out['pose'] = (np.asarray(table['pose']).astype(np.int64) + int(first_pose)).astype(np.int32)
    return out


def concat(chunks):
    """The tables of launches over consecutive ranges of the global poses as one table: every chunk's ``pose`` is local to its
    range (``shift`` is applied here, by the poses in front)."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError('library_bridges.concat: no table given')
    parts, first, rows, off = [], 0, 0, [np.zeros(1, np.int64)]
    for c in chunks:
        T, o = _check(c)
        if len(c['pose']) and (int(np.min(c['pose'])) < 0 or int(np.max(c['pose'])) >= T):
            raise ValueError('library_bridges.concat: a chunk names a pose outside its own range')
        parts.append(shift(c, first))
        off.append(o[1:] + rows)
        first, rows = first + T, rows + int(o[-1])
    out = {k: np.concatenate([np.asarray(p[k]) for p in parts]).astype(dt) for k, dt in COLUMNS}
    out['bridge_off'] = np.concatenate(off).astype(np.uint64)
    for k in ('waters', 'legs'):
        out[k] = np.concatenate([np.asarray(c[k]) for c in chunks]).astype(np.uint32)
    masks = {int(c['sift_any']) for c in chunks if 'sift_any' in c}
    if len(masks) > 1:
        raise ValueError('library_bridges.concat: the tables were made with different masks')
    if masks:
        out['sift_any'] = masks.pop()
    return out


BY_RESIDUE_COLUMNS = (('pose', np.int32), ('res', np.int32), ('n_waters', np.uint32), ('n_bridges', np.uint32), ('dist_min', np.float32))


def by_residue(table, res_id):
    """The table folded by pose and the residue of ``rec_atom``: one row per (pose, residue), ascending, with the distinct
    bridging waters, the rows and the smallest ``dist_lig + dist_rec`` (added in float32)."""
    _check(table)
    res = np.asarray(res_id).astype(np.int64)
    rec = np.asarray(table['rec_atom'], np.int64)
    if len(rec) and (rec.min() < 0 or rec.max() >= len(res)):
        raise ValueError('library_bridges.by_residue: a rec_atom lies outside res_id')
    r = res[rec]
    stride = int(r.max()) + 1 if len(r) else 1
    key, inv = np.unique(np.asarray(table['pose'], np.int64) * stride + r, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(key)
    path = (np.asarray(table['dist_lig'], np.float32) + np.asarray(table['dist_rec'], np.float32)).astype(np.float32)
    dmin = np.full(U, np.inf, np.float32)
    np.minimum.at(dmin, inv, path)
    pairs = np.unique(np.stack([inv, np.asarray(table['water'], np.int64)], axis=1), axis=0) if U else np.zeros((0, 2), np.int64)
    return {'pose': (key // stride).astype(np.int32), 'res': (key % stride).astype(np.int32),
            'n_waters': np.bincount(pairs[:, 0], minlength=U).astype(np.uint32), 'n_bridges': np.bincount(inv, minlength=U).astype(np.uint32),
            'dist_min': dmin}


def _names(bits):
    return [n for k, n in enumerate(config.SIFT_NAMES) if (int(bits) >> k) & 1]


def _rows(table, receptor, ligands, ligand_pose_off, component_types):
    from .core import export
    _check(table)
    lo = np.asarray(ligand_pose_off, np.int64)
    T = n_poses(table)
    if lo.ndim != 1 or len(lo) != len(ligands) + 1 or lo[0] != 0 or (np.diff(lo) < 0).any() or lo[-1] != T:
        raise ValueError('library_bridges: ligand_pose_off must be [L + 1] over the ligands, start at 0, not decrease and end at T')
    lig_of = np.repeat(np.arange(len(lo) - 1), np.diff(lo))
    rec = export.Labels(receptor, receptor.component_types if component_types is None else component_types)
    labs = {}
    for r in range(len(table['pose'])):
        t = int(table['pose'][r])
        l = int(lig_of[t])
        if l not in labs:
            labs[l] = export.Labels(ligands[l], ligands[l].ensure_labels().component_types)
        yield (l, t - int(lo[l]), rec, int(table['water'][r]), labs[l], int(table['lig_atom'][r]), int(table['rec_atom'][r]), table['dist_lig'][r],
               table['dist_rec'][r], _names(table['sift_lig'][r]), _names(table['sift_rec'][r]))


def to_records(table, receptor, ligands, ligand_pose_off, component_types=None):
    """The table as a list of dicts for JSON: 'ligand', 'pose' (within the ligand), the water, 'bgn' = the ligand's leg (the atom
    labelled from the ligand's own pack), 'end' = the receptor's leg."""
    return [{'ligand': l, 'pose': p, 'water': rec.atom_dict(w),
             'bgn': dict(lab.atom_dict(a), distance=float(dl), contact=nl), 'end': dict(rec.atom_dict(j), distance=float(dr), contact=nr),
             'type': 'library-water-bridge'}
            for l, p, rec, w, lab, a, j, dl, dr, nl, nr in _rows(table, receptor, ligands, ligand_pose_off, component_types)]


CSV_HEADER = ['ligand', 'pose', 'water', 'atom_ligand', 'atom_receptor', 'distance_ligand', 'distance_receptor', 'contacts_ligand',
              'contacts_receptor']


def write_csv(path, table, receptor, ligands, ligand_pose_off, component_types=None):
    """One row per bridge: ligand, pose within the ligand, the three atoms ('A/508/O'), the two distances (the shortest text that
    gives the float32 back) and each leg's contacts by name joined with '|'."""
    with open(path, 'w', newline='') as fh:
        out = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        out.writerow(CSV_HEADER)
        for l, p, rec, w, lab, a, j, dl, dr, nl, nr in _rows(table, receptor, ligands, ligand_pose_off, component_types):
            out.writerow([l, p, rec.atom_macro(w), lab.atom_macro(a), rec.atom_macro(j), str(dl), str(dr), '|'.join(nl), '|'.join(nr)])


def write_library_bridges(wd, sid, table, receptor, ligands, ligand_pose_off, component_types=None):
    """'<id>.librarybridges' in ``wd``."""
    path = os.path.join(wd, sid + '.librarybridges')
    write_csv(path, table, receptor, ligands, ligand_pose_off, component_types)
    return path
