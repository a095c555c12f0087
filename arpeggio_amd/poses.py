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

The ring and amide contacts of the same poses (``Context.poses_planes``, csrc/arp_poses_planes.h) have their host side in the
second half of this module: ``affected``, ``plane_reference_rows``, ``split_planes``, ``concat_planes``, ``planes_to_records``,
``write_planes_csv``.

Everything here is NumPy on the host; nothing imports the native library.
"""
import csv
import os

import numpy as np

from . import tables
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


def join_pose_off(offs):
    """The ``pose_off`` arrays of consecutive chunks as one (uint64): a chunk's records follow those of the chunks before it."""
    base, out = 0, [np.zeros(1, np.uint64)]
    for o in offs:
        o = np.asarray(o).astype(np.uint64)
        out.append(o[1:] + np.uint64(base))
        base += int(o[-1])
    return np.concatenate(out)


def join_poses(chunks):
    """``(pose_off, summary)`` of consecutive chunks of poses as one: what every ``concat`` over pose results shares."""
    return (join_pose_off(c['pose_off'] for c in chunks),
            np.concatenate([np.asarray(c['summary'], np.uint32).reshape(-1, SUMMARY) for c in chunks]))


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
    out['pose_off'], out['summary'] = join_poses(chunks)
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


# ---------------------------------------------------------------------------------------------------------------------
# Ring and amide contacts of the poses: host side of ``Context.poses_planes`` (arp_poses_planes_*, csrc/arp_poses_planes.h)
#
# A result (``table``) is a dict with one sub-table per bag — the columns ``Context.fetch_bag`` gives that bag plus ``pose_off``
# uint64 [P + 1], the records of a pose in the bag's canonical order —, ``summary`` uint32 [P, 16] and ``movable``.
# ---------------------------------------------------------------------------------------------------------------------
PLANE_TABLES = tables.PLANE_BAGS
# per table: id columns, value columns, byte columns, dtype of the value columns (the order of arp_poses_planes_fetch's arguments)
PLANE_COLUMNS = {name: (tuple(c for c, _ in b.ids), b.vals, b.bytes, b.vdt) for name, b in tables.BAGS.items()}
PLANE_ORDER = {name: b.order for name, b in tables.BAGS.items()}
PLANE_SUMMARY_SLOTS = ('atom_plane', 'plane_plane', 'group_group', 'group_plane', 'inter_carbonpi', 'inter_cationpi', 'inter_donorpi',
                       'inter_halogenpi', 'inter_metsulphurpi', 'inter_plane_plane', 'inter_group_group', 'inter_group_plane',
                       'affected_rings', 'rings_residue_changed', 'rings_without_residue', 'records')
CT_INTER = config.CONTACT_TYPE_NAMES.index('INTER')


def plane_columns(name):
    """Every record column of table ``name`` with its dtype, in fetch order."""
    return [(c, dt) for c, dt, _ in tables.bag_columns(name)]


def _kd2(a, b):
    """Bio.PDB.kdtrees' membership quantity between every row of ``a`` and every row of ``b``: float64 sum of squares in x, y, z
    order, no fusion (num::dist2_kd on the device)."""
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    r = d[..., 0] * d[..., 0]
    r = r + d[..., 1] * d[..., 1]
    r = r + d[..., 2] * d[..., 2]
    return r


def affected(pc, sel, xyz_pose):
    """What one pose of movable set ``sel`` affects: ``(moved_amides, affected_rings)``, ascending ids.  An amide is moved when
    its N, C or O is movable.  A ring is affected when a movable atom is in its path, or lies within 3.0 A (inclusive, float64
    sum of squares) of its resident centre at the atom's pose coordinate ``xyz_pose`` [S, 3] or at its resident coordinate."""
    m = _mask(pc, sel)
    atoms = np.nonzero(m)[0]
    x_pose = np.asarray(xyz_pose, np.float32).reshape(-1, 3)
    if len(x_pose) != len(atoms):
        raise ValueError(f'affected: xyz_pose must be [{len(atoms)}, 3]')
    am = np.asarray(pc.amide_atoms, np.int64).reshape(-1, 4)
    moved = np.nonzero(m[am[:, :3]].any(axis=1))[0] if len(am) else np.zeros(0, np.int64)
    nr = pc.n_rings
    aff = np.zeros(nr, bool)
    if nr:
        aff |= np.array([bool(m[np.asarray(a, np.int64)].any()) for a in pc.ring_atoms])
        ctr = np.asarray(pc.ring_center, np.float64).reshape(-1, 3)
        for x in (x_pose, np.asarray(pc.xyz, np.float32)[atoms]):
            aff |= (_kd2(ctr, x.astype(np.float64)) <= 9.0).any(axis=1)
    return moved.astype(np.int64), np.nonzero(aff)[0].astype(np.int64)


def plane_reference_rows(bags, pc, sel, xyz_pose):
    """Of the four ring / amide bags of a pass over one pose as a whole structure or model: the rows that involve an affected
    entity (``affected``), each bag in its canonical order — what the pose's records must equal."""
    m = _mask(pc, sel)
    moved, rings = affected(pc, sel, xyz_pose)
    am = np.zeros(pc.n_amides, bool)
    am[moved] = True
    rg = np.zeros(pc.n_rings, bool)
    rg[rings] = True
    keep = {'atom_plane': lambda b: m[b['atom']] | rg[b['ring']], 'plane_plane': lambda b: rg[b['bgn']] | rg[b['end']],
            'group_group': lambda b: am[b['bgn']] | am[b['end']], 'group_plane': lambda b: am[b['amide']] | rg[b['ring']]}
    out = {}
    for name in PLANE_TABLES:
        b = {c: np.asarray(bags[name][c]) for c, _ in plane_columns(name)}
        k = keep[name](b) if len(b[PLANE_ORDER[name][0]]) else np.zeros(0, bool)
        first, second = PLANE_ORDER[name]
        order = np.lexsort((b[second][k], b[first][k]))
        out[name] = {c: b[c][k][order].astype(dt) for c, dt in plane_columns(name)}
    return out


def summarise_planes(rows):
    """Slots 0 - 11 and 15 of the summary row of one pose's records (slots 12 - 14 count rings, not records: left 0)."""
    s = np.zeros(SUMMARY, np.uint32)
    for t, name in enumerate(PLANE_TABLES):
        ct = np.asarray(rows[name]['ctype'])
        s[t] = len(ct)
        inter = ct == CT_INTER
        if t == 0:
            mask = np.asarray(rows[name]['mask'])
            for b in range(5):
                s[4 + b] = int((inter & (((mask >> b) & 1) != 0)).sum())
        else:
            s[8 + t] = int(inter.sum())
    s[15] = int(s[:4].sum())
    return s


def empty_planes(n=0, movable_atoms=()):
    t = {name: dict({c: np.zeros(0, dt) for c, dt in plane_columns(name)}, pose_off=np.zeros(n + 1, np.uint64)) for name in PLANE_TABLES}
    t['summary'] = np.zeros((n, SUMMARY), np.uint32)
    t['movable'] = np.asarray(movable_atoms, np.int32)
    return t


def planes_from_rows(rows, movable_atoms, summary=None):
    """Per-pose rows (a list of ``plane_reference_rows`` results) as the table the device returns (summary slots 12 - 14 from
    ``summary`` when given, else 0)."""
    t = {}
    for name in PLANE_TABLES:
        t[name] = {c: (np.concatenate([r[name][c] for r in rows]) if rows else np.zeros(0)).astype(dt) for c, dt in plane_columns(name)}
        t[name]['pose_off'] = np.concatenate([[0], np.cumsum([len(r[name]['ctype']) for r in rows])]).astype(np.uint64)
    t['summary'] = np.stack([summarise_planes(r) for r in rows]) if rows else np.zeros((0, SUMMARY), np.uint32)
    if summary is not None:
        t['summary'][:, 12:15] = np.asarray(summary)[:, 12:15]
    t['movable'] = np.asarray(movable_atoms, np.int32)
    return t


def split_planes(table):
    """One dict of four bags per pose."""
    P = len(table['summary'])
    out = []
    for p in range(P):
        one = {}
        for name in PLANE_TABLES:
            off = np.asarray(table[name]['pose_off']).astype(np.int64)
            one[name] = {c: np.asarray(table[name][c])[off[p]:off[p + 1]] for c, _ in plane_columns(name)}
        out.append(one)
    return out


def concat_planes(chunks):
    """The results of consecutive chunks of poses as one."""
    chunks = list(chunks)
    if not chunks:
        return empty_planes()
    out = {}
    for name in PLANE_TABLES:
        out[name] = {c: np.concatenate([np.asarray(ch[name][c]) for ch in chunks]).astype(dt) for c, dt in plane_columns(name)}
        out[name]['pose_off'] = join_pose_off(ch[name]['pose_off'] for ch in chunks)
    out['summary'] = np.concatenate([np.asarray(ch['summary'], np.uint32).reshape(-1, SUMMARY) for ch in chunks])
    mv = [np.asarray(ch['movable']) for ch in chunks if 'movable' in ch]
    if mv:
        if any(not np.array_equal(mv[0], m) for m in mv[1:]):
            raise ValueError('concat_planes: the chunks have different movable sets')
        out['movable'] = mv[0]
    return out


CLASS_PLANE = 15          # the first class plane of a pose fingerprint (pose_fingerprints.CLASS_PLANE_NAMES, ARP_POSEFP_PLANES)


def ligand_side(pc, idx):
    """Which entities are the ligand's for movable set ``idx``: ``(atoms bool [n], rings bool [n_rings], amides bool [n_amides])``
    — a movable atom, a ring with a movable atom in its path, an amide whose N, C or O is movable.  A ring a pose merely comes
    near stays the receptor's."""
    m = _mask(pc, idx)
    rings = np.array([bool(m[np.asarray(a, np.int64)].any()) for a in pc.ring_atoms], bool).reshape(-1)
    am = np.asarray(pc.amide_atoms, np.int64).reshape(-1, 4)
    amides = m[am[:, :3]].any(axis=1) if len(am) else np.zeros(0, bool)
    return m, rings, amides


def ring_home_residue(pc):
    """int64 [n_rings]: the residue of the first atom of every ring's path — the node of a receptor ring in a pose
    fingerprint.  Not ``ring_res``: that is the nearest atom within 3 A of the centre, which a ligand atom on the ring takes over."""
    return np.array([int(pc.res_id[int(a[0])]) if len(a) else -1 for a in pc.ring_atoms], np.int64).reshape(-1)


def plane_fingerprints(planes_table, pc, idx, ctype_mask=0x7F):
    """The host route to the class planes of the pose fingerprints, over a fetched ``Context.poses_planes`` table: per pose the
    set of ``(node, plane)`` — plane 15 ... 28 as ``pose_fingerprints.CLASS_PLANE_NAMES`` numbers them, node the residue of the
    receptor entity — of the records whose ``ctype`` bit is in ``ctype_mask`` and of whose two entities exactly one is the
    ligand's (``ligand_side``).  A node outside [0, n_residues) is skipped.  Returns a list of P sets."""
    atoms, rings, amides = ligand_side(pc, idx)
    ring_res = ring_home_residue(pc)
    res_id = np.asarray(pc.res_id, np.int64)
    am_res = np.asarray(pc.amide_res, np.int64).reshape(-1)
    P = len(planes_table['summary'])
    out = [set() for _ in range(P)]

    def add(name, keep, node, plane):
        off = np.asarray(planes_table[name]['pose_off']).astype(np.int64)
        pose = np.repeat(np.arange(P), np.diff(off))
        ct = np.asarray(planes_table[name]['ctype']).astype(np.int64)
        keep = keep & (((int(ctype_mask) >> ct) & 1) != 0) & (node >= 0) & (node < pc.n_residues)
        for p, u, q in zip(pose[keep].tolist(), node[keep].tolist(), np.broadcast_to(plane, keep.shape)[keep].tolist()):
            out[p].add((u, q))

    b = planes_table['atom_plane']
    a, r, mask = np.asarray(b['atom'], np.int64), np.asarray(b['ring'], np.int64), np.asarray(b['mask'], np.int64)
    for bit in range(5 if len(a) else 0):
        add('atom_plane', (atoms[a] != rings[r]) & (((mask >> bit) & 1) != 0), np.where(atoms[a], ring_res[r], res_id[a]),
            np.where(atoms[a], CLASS_PLANE + bit, CLASS_PLANE + 5 + bit))
    b = planes_table['plane_plane']
    r1, r2 = np.asarray(b['bgn'], np.int64), np.asarray(b['end'], np.int64)
    if len(r1):
        add('plane_plane', rings[r1] != rings[r2], np.where(rings[r1], ring_res[r2], ring_res[r1]), CLASS_PLANE + 10)
    b = planes_table['group_group']
    a1, a2 = np.asarray(b['bgn'], np.int64), np.asarray(b['end'], np.int64)
    if len(a1):
        add('group_group', amides[a1] != amides[a2], np.where(amides[a1], am_res[a2], am_res[a1]), CLASS_PLANE + 11)
    b = planes_table['group_plane']
    a, r = np.asarray(b['amide'], np.int64), np.asarray(b['ring'], np.int64)
    if len(a):
        add('group_plane', amides[a] != rings[r], np.where(amides[a], ring_res[r], am_res[a]), np.where(amides[a], CLASS_PLANE + 12, CLASS_PLANE + 13))
    return out


def planes_to_records(table, pc, component_types=None):
    """The records as the dicts ``get_contacts`` returns for the four bags (export.py), each with its 'pose'.  Rings and amides
    are labelled by their resident residue."""
    from .core import export
    ctypes_ = pc.component_types if component_types is None else component_types
    out = []
    for p, bags in enumerate(split_planes(table)):
        for rec in export.contacts_json(pc, bags, ctypes_):
            rec['pose'] = p
            out.append(rec)
    return out


PLANES_CSV_HEADER = ['pose', 'type', 'bgn', 'end', 'distance', 'contacts', 'interacting_entities']


def planes_csv_rows(lab, bags):
    """The CSV rows of one pose's four bags, without the pose column: bag, the two entities, distance, contacts, interacting
    entities.  ``lab``: ``export.Labels`` of the structure the ids are of."""
    from .core import export
    ct, pp, ap = config.CONTACT_TYPE_NAMES, config.PLANE_PLANE_NAMES, config.ATOM_PLANE_NAMES
    b = bags['atom_plane']
    for a, r, d, m, c in zip(b['atom'].tolist(), b['ring'].tolist(), export.rounded(b['dist']), b['mask'].tolist(), b['ctype'].tolist()):
        yield ['atom-plane', lab.atom_macro(a), f'ring/{r}', d, '|'.join(n for k, n in enumerate(ap) if (m >> k) & 1), ct[c]]
    b = bags['plane_plane']
    for r1, r2, d, t1, t2, c in zip(b['bgn'].tolist(), b['end'].tolist(), export.rounded(b['dist']), b['type1'].tolist(), b['type2'].tolist(),
                                    b['ctype'].tolist()):
        yield ['plane-plane', f'ring/{r1}', f'ring/{r2}', d, '|'.join([pp[t1]] + ([pp[t2]] if t2 < config.PP_SAME else [])), ct[c]]
    b = bags['group_group']
    for a1, a2, d, c in zip(b['bgn'].tolist(), b['end'].tolist(), export.rounded(b['dist']), b['ctype'].tolist()):
        yield ['group-group', f'amide/{a1}', f'amide/{a2}', d, 'AMIDEAMIDE', ct[c]]
    b = bags['group_plane']
    for a, r, d, c in zip(b['amide'].tolist(), b['ring'].tolist(), export.rounded(b['dist']), b['ctype'].tolist()):
        yield ['group-plane', f'amide/{a}', f'ring/{r}', d, 'AMIDERING', ct[c]]


def write_planes_csv(path, table, pc, component_types=None):
    """One row per record: pose, bag, the two entities ('A/508/O' for an atom, 'ring/<id>' and 'amide/<id>' otherwise), the
    distance rounded as ``get_contacts`` rounds it, the contacts by name joined with '|', the interacting entities."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(PLANES_CSV_HEADER)
        for p, bags in enumerate(split_planes(table)):
            for row in planes_csv_rows(lab, bags):
                w.writerow([p] + row)


def write_pose_planes(wd, sid, table, pc, component_types=None):
    """'<id>.poseplanes' in ``wd``."""
    path = os.path.join(wd, sid + '.poseplanes')
    write_planes_csv(path, table, pc, component_types)
    return path
