"""Pose fingerprints with the ring and amide classes as planes (arp_poses_fingerprints_planes_launch, Context.poses_fingerprints with a
mask beyond bit 14, pose_fingerprints.planes(classes=...), poses.plane_fingerprints, run_pose_fingerprints(classes=...)).

The yardstick is plain Python over the tables ``Context.poses_planes`` and ``Context.poses_contacts`` fetch — pinned by
tests/test_poses_planes.py and tests/test_poses.py, code this feature does not touch — and the pack: the ligand side of every
entity is decided from ``ring_atoms``, ``amide_atoms`` and the selection, a pose's features are a set of (node, plane), and
``ids``, ``count``, ``cross``, ``occupancy``, ``inter`` and the packed ``bits`` follow from the sets.  It does not import
``poses.plane_fingerprints``.  Every comparison is exact equality of integers: no tolerance, no time.

The cases are those of tests/test_poses_planes.py — ``main`` (HEM, 70 poses), ``phe`` (48), ``lys`` (33) — on a RELABELLED copy of
the pack: every ``hbond donor`` atom is an ``xbond donor`` as well, every ``pos ionisable`` atom gets ``F_RES_MET | F_ELEM_S``;
without that, halogen-pi and Met-sulphur-pi never occur.  One thing is added so that the relabelled pack is still a valid input of
the atom-atom launch: the 20 water oxygens, hbond donors whose only neighbours are their hydrogens, have no single-bond
neighbour (``sb_nbr`` -1), and an xbond donor without one makes the reference raise (utils.py:173) and
``arp_poses_contacts_launch`` refuse with ARP_E_XBOND_NBR as soon as an acceptor of the ligand comes near — no atom-atom table would
exist to reduce.  They get their first bonded atom as that neighbour.  None of the four ring / amide loops reads ``sb_nbr``."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, pose_fingerprints as fp, poses
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex
from helpers import tiny_complex
import test_poses as tp
import test_poses_planes as tpp
from test_pose_fingerprints import _fetch_everything, _fetch_rc, _p, _same_bytes, differences, pack_bits

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
INTER = 1 << CT['INTER']
PARAMS = (5.0, 0.1, False)
ALL15 = 0x7FFF
ALL29 = (1 << 29) - 1
CLASSES = ALL29 & ~ALL15
MIX = sum(1 << b for b in (1, 9, 20, 25, 28))      # a non-contiguous mix of SIFt bits and class planes
KEYS = ('ids', 'count', 'cross', 'occupancy', 'bits')
NAMES = ('main', 'phe', 'lys')


# ------------------------------------------------------------------------------------------------------------- yardstick
def ligand_sides(pc, idx):
    """Which atoms, rings and amides are the ligand's: from the pack and the selection alone."""
    mine = set(int(a) for a in idx)
    atoms = [a in mine for a in range(pc.n_atoms)]
    rings = [any(int(a) in mine for a in path) for path in pc.ring_atoms]
    amides = [any(int(a) in mine for a in row[:3]) for row in np.asarray(pc.amide_atoms).reshape(-1, 4)]
    return atoms, rings, amides


def class_features(ptable, pc, idx, planes, ctype_mask):
    """Per pose the set of (node, plane >= 15) of the ring / amide records, record by record."""
    atoms, rings, amides = ligand_sides(pc, idx)
    res_id, am_res = pc.res_id, pc.amide_res
    ring_res = [int(res_id[int(path[0])]) for path in pc.ring_atoms]
    P = len(ptable['summary'])
    out = [set() for _ in range(P)]

    def records(name, *cols):
        t = ptable[name]
        off = t['pose_off'].astype(np.int64)
        for p in range(P):
            for r in range(off[p], off[p + 1]):
                if (ctype_mask >> int(t['ctype'][r])) & 1:
                    yield (p,) + tuple(int(t[c][r]) for c in cols)

    def put(p, node, plane):
        if (planes >> plane) & 1 and 0 <= node < pc.n_residues:
            out[p].add((node, plane))
    for p, a, r, mask in records('atom_plane', 'atom', 'ring', 'mask'):
        if atoms[a] != rings[r]:
            for b in range(5):
                if (mask >> b) & 1:
                    put(p, ring_res[r] if atoms[a] else int(res_id[a]), (15 if atoms[a] else 20) + b)
    for p, r1, r2 in records('plane_plane', 'bgn', 'end'):
        if rings[r1] != rings[r2]:
            put(p, ring_res[r2] if rings[r1] else ring_res[r1], 25)
    for p, a1, a2 in records('group_group', 'bgn', 'end'):
        if amides[a1] != amides[a2]:
            put(p, int(am_res[a2] if amides[a1] else am_res[a1]), 26)
    for p, a, r in records('group_plane', 'amide', 'ring'):
        if amides[a] != rings[r]:
            put(p, ring_res[r] if amides[a] else int(am_res[a]), 27 if amides[a] else 28)
    return out


def atom_features(table, pc, planes, ctype_mask):
    """Per pose the set of (receptor residue, SIFt bit) of the atom-atom records."""
    P = poses.n_poses(table)
    out = [set() for _ in range(P)]
    mv = set(int(a) for a in table['movable'])
    off = table['pose_off'].astype(np.int64)
    ci, cj, sift, ctype, res_id = (np.asarray(v).tolist() for v in (table['i'], table['j'], table['sift'], table['ctype'], pc.res_id))
    for p in range(P):
        for r in range(off[p], off[p + 1]):
            s = sift[r] & planes & ALL15
            if not s or not (ctype_mask >> ctype[r]) & 1:
                continue
            node = res_id[cj[r] if ci[r] in mv else ci[r]]
            if 0 <= node < pc.n_residues:
                out[p].update((node, b) for b in range(15) if (s >> b) & 1)
    return out


def results_of(feats, planes, n_refs=0, all_pairs=False):
    """ids, count, cross, occupancy, bits (and inter) of per-pose sets of (node, plane)."""
    P = len(feats)
    ids = sorted({u for f in feats for u, _ in f})
    axis = [b for b in range(29) if (planes >> b) & 1]
    sel = np.zeros((P, len(ids), len(axis)), bool)
    for p, f in enumerate(feats):
        for u, b in f:
            sel[p, ids.index(u), axis.index(b)] = True
    out = dict(ids=np.array(ids, np.int32), count=np.array([len(f) for f in feats], np.uint32),
               cross=np.array([[len(feats[p] & feats[q]) for q in range(n_refs)] for p in range(P)], np.uint32).reshape(P, n_refs),
               occupancy=sel[n_refs:].sum(axis=0).astype(np.uint32).reshape(len(ids), len(axis)), bits=pack_bits(sel), sel=sel)
    if all_pairs:
        out['inter'] = np.array([[len(feats[p] & feats[q]) for q in range(P)] for p in range(P)], np.uint32)
    return out


def features(table, ptable, pc, idx, planes, ctype_mask=0x7F):
    a = atom_features(table, pc, planes, ctype_mask)
    c = class_features(ptable, pc, idx, planes, ctype_mask)
    return [x | y for x, y in zip(a, c)]


def yardstick(table, ptable, pc, idx, planes, ctype_mask=0x7F, n_refs=0, all_pairs=False):
    return results_of(features(table, ptable, pc, idx, planes, ctype_mask), planes, n_refs, all_pairs)


# ------------------------------------------------------------------------------------------------------------- cases
def relabelled(pc):
    """The pack with every hbond donor an xbond donor too and every pos ionisable atom a Met sulphur too; a new xbond donor
    without a single-bond neighbour (the water oxygens) gets its first bonded atom as one (see the module's docstring)."""
    q = copy.copy(pc)
    tm, fl, sb = np.asarray(pc.type_mask).copy(), np.asarray(pc.flags).copy(), np.asarray(pc.sb_nbr).copy()
    donor = (tm & config.ATOM_TYPE_BIT['hbond donor']) != 0
    tm[donor] |= config.ATOM_TYPE_BIT['xbond donor']
    fl[(tm & config.ATOM_TYPE_BIT['pos ionisable']) != 0] |= config.F_RES_MET | config.F_ELEM_S
    for a in np.flatnonzero(donor & (sb < 0)):
        assert pc.bond_off[a + 1] > pc.bond_off[a]
        sb[a] = pc.bond_idx[pc.bond_off[a]]
    q.type_mask, q.flags, q.sb_nbr = tm, fl, sb
    return q


@functools.lru_cache(maxsize=None)
def case(name):
    pc, idx, x, h = tpp.CASES[name]()
    return relabelled(pc), idx, x, h


@functools.lru_cache(maxsize=None)
def oracle_table(name):
    """The ring / amide table of a relabelled case from the oracle alone (the CPU stand-in of tests/test_poses_planes.py)."""
    pc, idx, x, h = tpp.CASES[name]()
    pc = relabelled(pc)
    home = tpp.home_pack_cpu(pc)
    X, H = poses.as_models(pc, idx, x, h)
    m = tp._mask(pc, idx)
    rows, posed_res = [], []
    for p in range(len(X)):
        q = tpp.home_pack_cpu(tp.pose_pack(pc, X, H, p))
        rows.append(poses.plane_reference_rows(tpp.oracle_bags(q, m), home, idx, x[p]))
        posed_res.append(q.ring_res)
    return poses.planes_from_rows(rows, idx), posed_res


def _ctx(pc, idx):
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(tp._mask(pc, idx))
    ctx.set_plane_atoms(pc)
    return ctx


def both(ctx, x, h, params=PARAMS):
    """Both poses results of the same poses, fetched."""
    return ctx.poses_contacts(x, h, *params), ctx.poses_planes(x)


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_case():
    """Twelve atoms in four residues of three; the movable set is residue 0.  Ring 0 = atoms 0 1 2 is the ligand's, ring 1 =
    atoms 3 4 5 (residue 1) and ring 2 = atoms 7 8 6 (first atom 7: residue 2) are the receptor's; amide 0 (N 1, C 2, O 0) is the
    ligand's, amide 1 (residue 3) and amide 2 (residue 2) the receptor's.
      pose 0, one record of every (table, side) kind:
        atom 0 - ring 1, CARBONPI | DONORPI    ligand atom   -> (1, 15), (1, 17)
        atom 9 - ring 0, CATIONPI              ligand ring   -> (3, 21)
        ring 0 - ring 2                                       -> (2, 25)
        amide 1 - amide 0                                     -> (3, 26)
        amide 0 - ring 1                       ligand amide  -> (1, 27)
        amide 2 - ring 0                       ligand ring   -> (2, 28)
      pose 1: atom 1 - ring 0 and amide 0 - amide 0 (both the ligand's), atom 4 - ring 2 and ring 1 - ring 2 (neither): nothing;
              atom 2 - ring 2, METSULPHURPI, INTRA_SELECTION -> (2, 19) unless only INTER is admitted
      pose 2: no record"""
    pc = tiny_complex(np.arange(36, dtype=np.float64).reshape(12, 3), res_id=[0] * 3 + [1] * 3 + [2] * 3 + [3] * 3,
                      rings=(np.zeros((3, 3)), np.zeros((3, 3)), np.array([0, 1, 2], np.int32)),
                      amides=(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.array([0, 3, 2], np.int32)))
    pc.ring_atoms = [np.array([0, 1, 2], np.int32), np.array([3, 4, 5], np.int32), np.array([7, 8, 6], np.int32)]
    pc.amide_atoms = np.array([[1, 2, 0, 0], [9, 10, 11, 9], [6, 7, 8, 6]], np.int32)
    I, S = CT['INTER'], CT['INTRA_SELECTION']
    ap = lambda atom, ring, mask, ct: dict(atom=atom, ring=ring, dist=[4.0] * len(atom), theta=[10.0] * len(atom), mask=mask, ctype=ct)
    pp = lambda bgn, end: dict(bgn=bgn, end=end, dist=[4.0] * len(bgn), dihedral=[5.0] * len(bgn), theta_bgn=[1.0] * len(bgn), theta_end=[2.0] * len(bgn),
                               type1=[0] * len(bgn), type2=[255] * len(bgn), ctype=[I] * len(bgn))
    g = lambda first, second, a, b: {first: a, second: b, 'dist': [4.0] * len(a), 'dihedral': [5.0] * len(a), 'theta': [6.0] * len(a), 'ctype': [I] * len(a)}
    rows = [dict(atom_plane=ap([0, 9], [1, 0], [1 | 4, 2], [I, I]), plane_plane=pp([0], [2]), group_group=g('bgn', 'end', [1], [0]),
                 group_plane=g('amide', 'ring', [0, 2], [1, 0])),
            dict(atom_plane=ap([1, 4, 2], [0, 2, 2], [1, 1, 16], [I, I, S]), plane_plane=pp([1], [2]), group_group=g('bgn', 'end', [0], [0]),
                 group_plane=g('amide', 'ring', [], [])),
            dict(atom_plane=ap([], [], [], []), plane_plane=pp([], []), group_group=g('bgn', 'end', [], []), group_plane=g('amide', 'ring', [], []))]
    rows = [{n: {c: np.asarray(r[n][c], dt) for c, dt in poses.plane_columns(n)} for n in poses.PLANE_TABLES} for r in rows]
    return pc, np.array([0, 1, 2]), poses.planes_from_rows(rows, [0, 1, 2])


def test_the_host_route_and_the_yardstick_on_a_hand_made_table():
    pc, idx, t = hand_case()
    pose0 = {(1, 15), (1, 17), (3, 21), (2, 25), (3, 26), (1, 27), (2, 28)}
    atoms, rings, amides = poses.ligand_side(pc, idx)
    assert atoms.tolist() == [True] * 3 + [False] * 9 and rings.tolist() == [True, False, False] and amides.tolist() == [True, False, False]
    assert poses.ring_home_residue(pc).tolist() == [0, 1, 2]
    assert poses.plane_fingerprints(t, pc, idx) == [pose0, {(2, 19)}, set()]
    assert poses.plane_fingerprints(t, pc, idx, INTER) == [pose0, set(), set()]
    assert poses.plane_fingerprints(t, pc, idx, 1 << CT['INTRA_SELECTION']) == [set(), {(2, 19)}, set()]
    assert class_features(t, pc, idx, CLASSES, 0x7F) == [pose0, {(2, 19)}, set()] and class_features(t, pc, idx, CLASSES, INTER) == [pose0, set(), set()]
    # a plane that is not selected drops its features only
    assert class_features(t, pc, idx, CLASSES & ~(1 << 17) & ~(1 << 28), 0x7F) == [pose0 - {(1, 17), (2, 28)}, {(2, 19)}, set()]
    # a node outside the residues is skipped
    q = copy.copy(pc)
    q.amide_res = np.array([0, -1, 2], np.int32)
    assert poses.plane_fingerprints(t, q, idx)[0] == pose0 - {(3, 26)} == class_features(t, q, idx, CLASSES, 0x7F)[0]
    # the numbers that follow from the sets, pose 0 the reference
    r = results_of([pose0, {(2, 19)}, set()], CLASSES, n_refs=1, all_pairs=True)
    assert r['ids'].tolist() == [1, 2, 3] and r['count'].tolist() == [7, 1, 0] and r['cross'].tolist() == [[7], [0], [0]]
    assert r['occupancy'].shape == (3, 14) and r['occupancy'].sum() == 1 and r['occupancy'][1, 4] == 1      # (2, 19) alone lies behind the reference
    assert r['inter'].tolist() == [[7, 0, 0], [0, 1, 0], [0, 0, 0]] and r['bits'].shape == (3, 14, 1)
    assert [int(w) for w in r['bits'][0, :, 0]] == [1, 0, 1, 0, 0, 0, 4, 0, 0, 0, 2, 4, 1, 2]
    res = dict(r, planes=CLASSES, n_refs=1, level='residue')
    assert np.array_equal(fp.unpack(res), r['sel']) and fp.tanimoto(res).tolist() == [[1.0], [0.0], [0.0]]


def test_planes_names_shorthands_and_errors():
    assert fp.N_ALL_PLANES == 29 == _capi.POSEFP_ALL_PLANES and len(fp.CLASS_PLANE_NAMES) == 14
    assert fp.CLASS_PLANE_NAMES[:5] == tuple(n + '_LIGAND_ATOM' for n in config.ATOM_PLANE_NAMES)
    assert fp.CLASS_PLANE_NAMES[5:10] == tuple(n + '_LIGAND_RING' for n in config.ATOM_PLANE_NAMES)
    assert fp.CLASS_PLANE_NAMES[10:] == ('PLANE_PLANE', 'GROUP_GROUP', 'GROUP_PLANE_LIGAND_AMIDE', 'GROUP_PLANE_LIGAND_RING')
    base = fp.planes()
    assert base == ALL15 & ~BIT['proximal'] and fp.planes(None, ()) == base
    assert fp.planes(classes='all') == base | CLASSES and fp.planes(['hbond'], 'all') == BIT['hbond'] | CLASSES
    assert fp.planes([], 'all') == CLASSES
    assert fp.planes([], 'atom_plane') == 0x3FF << 15 and fp.planes([], ['plane_plane']) == 1 << 25 and fp.planes([], ('group_group',)) == 1 << 26
    assert fp.planes([], 'group_plane') == 3 << 27 and fp.planes([], ['CATIONPI_LIGAND_ATOM', 'HALOGENPI_LIGAND_RING']) == (1 << 16) | (1 << 23)
    assert fp.planes(['vdw'], ['GROUP_PLANE_LIGAND_RING', 'group_plane']) == BIT['vdw'] | (3 << 27)
    for bad in ('nonsense', ['PLANE_PLANE', 'hbond'], ['atom_atom']):
        with pytest.raises(ValueError):
            fp.planes(None, bad)
    with pytest.raises(ValueError):
        fp.planes([])
    # below bit 15 the names are what they were; above, the class names follow in plane order
    assert fp.plane_names(ALL15) == list(config.SIFT_NAMES[:15]) and fp.plane_names(BIT['hbond'] | BIT['vdw']) == ['vdw', 'hbond']
    assert fp.plane_names(ALL29) == list(config.SIFT_NAMES[:15]) + list(fp.CLASS_PLANE_NAMES)
    assert fp.plane_names(MIX) == [config.SIFT_NAMES[1], config.SIFT_NAMES[9], 'CARBONPI_LIGAND_RING', 'PLANE_PLANE', 'GROUP_PLANE_LIGAND_RING']
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert 'arp_poses_fingerprints_planes_launch' in _capi.SYMBOLS and 'int arp_poses_fingerprints_planes_launch(' in hdr
    assert '#define ARP_POSEFP_ALL_PLANES %d' % fp.N_ALL_PLANES in hdr


def test_merge_records_and_the_csv_header_with_class_planes(tmp_path):
    pc = tp.protein()
    planes = BIT['hbond'] | (1 << 25) | (1 << 28)
    a = dict(ids=np.array([3, 7], np.int32), count=np.array([2, 3], np.uint32), cross=np.array([[2], [1]], np.uint32),
             occupancy=np.array([[1, 0, 1], [0, 1, 0]], np.uint32), planes=planes, n_refs=1, level='residue')
    b = dict(ids=np.array([7, 9], np.int32), count=np.array([2, 1, 0], np.uint32), cross=np.array([[2], [0], [0]], np.uint32),
             occupancy=np.array([[0, 0, 1], [1, 0, 0]], np.uint32), planes=planes, n_refs=1, level='residue')
    m = fp.merge([a, b])
    assert m['ids'].tolist() == [3, 7, 9] and m['occupancy'].tolist() == [[1, 0, 1], [0, 1, 1], [1, 0, 0]] and m['planes'] == planes
    assert m['count'].tolist() == [2, 3, 1, 0] and m['cross'].tolist() == [[2], [1], [0], [0]]
    with pytest.raises(ValueError):
        fp.merge([a, dict(b, planes=planes | (1 << 26))])
    recs = fp.to_records(m, pc)
    assert recs[-1] == {'node': 'A/10/', 'type': 'pose-occupancy', 'level': 'residue', 'poses': {'hbond': 1, 'PLANE_PLANE': 0, 'GROUP_PLANE_LIGAND_RING': 0}}
    path = str(tmp_path / 'classes.csv')
    fp.write_csv(path, fp.strip_references(m), pc)
    lines = open(path).read().splitlines()
    assert lines[0] == 'pose,count,shared_0,tanimoto_0,recovery_0' and lines[4] == 'node,hbond,PLANE_PLANE,GROUP_PLANE_LIGAND_RING'
    assert lines[5:] == ['A/4/,1,0,1', 'A/8/,0,1,1', 'A/10/,1,0,0']


def test_run_pose_fingerprints_refuses_classes_at_atom_level():
    pc, idx, x, h = case('lys')
    with pytest.raises(ValueError, match="level='residue'"):
        InteractionComplex(copy.copy(pc)).run_pose_fingerprints(np.asarray(idx), x, h, *PARAMS, level='atom', classes='all')


def test_the_oracle_alone_meets_the_coverage_condition():
    """Asserted of the oracle's rows of the three relabelled cases, before any device is compared: every class plane has records,
    and records that must be left out — both sides the ligand's, neither — exist, as do empty tables and take-overs."""
    seen = {}
    for name in NAMES:
        pc, idx, x, h = case(name)
        t, posed_res = oracle_table(name)
        atoms, rings, amides = (np.array(v, bool) for v in ligand_sides(pc, idx))
        ap, pp, gg, gp = (t[k] for k in poses.PLANE_TABLES)
        feats = class_features(t, tpp.home_pack_cpu(pc), idx, CLASSES, 0x7F)
        assert feats == poses.plane_fingerprints(t, pc, idx)
        ring_res = poses.ring_home_residue(pc)
        pose = np.repeat(np.arange(len(x)), np.diff(ap['pose_off'].astype(np.int64)))
        lig_atom = atoms[ap['atom']] & ~rings[ap['ring']]
        posed = np.array([posed_res[p][r] for p, r in zip(pose, ap['ring'])], np.int64)
        seen[name] = dict(planes={q for f in feats for _, q in f}, sizes=[len(t[k]['ctype']) for k in poses.PLANE_TABLES],
                          both=[int((atoms[ap['atom']] & rings[ap['ring']]).sum()), int((rings[pp['bgn']] & rings[pp['end']]).sum()),
                                int((amides[gg['bgn']] & amides[gg['end']]).sum()), int((amides[gp['amide']] & rings[gp['ring']]).sum())],
                          neither=[int((~atoms[ap['atom']] & ~rings[ap['ring']]).sum()), int((~rings[pp['bgn']] & ~rings[pp['end']]).sum()),
                                   int((~amides[gg['bgn']] & ~amides[gg['end']]).sum()), int((~amides[gp['amide']] & ~rings[gp['ring']]).sum())],
                          lig_atom=int(lig_atom.sum()), takeover=int((posed[lig_atom] != ring_res[ap['ring']][lig_atom]).sum()))
        print(name, seen[name])
    main, phe, lys = (seen[k] for k in NAMES)
    assert main['planes'] | phe['planes'] | lys['planes'] == set(range(15, 29))
    assert {16, 19} <= lys['planes'] and {26, 27, 28} <= phe['planes'] and {20, 21, 22, 23, 24, 25, 28} <= main['planes']
    assert main['sizes'][3] == 29 and main['both'][1] == 89 and phe['both'][2:] == [9, 1]
    assert lys['neither'][:2] == [41, 101]
    assert lys['lig_atom'] > 0 and lys['takeover'] > 0      # a ligand atom on a ring takes the posed ring residue over
    assert lys['sizes'][1] == 101 and lys['sizes'][3] == 0 and main['sizes'][2] == 0      # empty tables, and one that only holds records to leave out
    assert lys['planes'] & {25} == set()


# ------------------------------------------------------------------------------------------------------------- GPU: contents
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_contents(name):
    pc, idx, x, h = case(name)
    ctx = _ctx(pc, idx)
    table, ptable = both(ctx, x, h)
    P = len(x)
    assert sum(len(ptable[k]['ctype']) for k in poses.PLANE_TABLES) > 0 and len(table['i']) > 0
    full = yardstick(table, ptable, pc, idx, ALL29)
    alone = yardstick(table, ptable, pc, idx, CLASSES)
    # class planes alone: the ring / amide nodes only, fewer than with the atom-atom records (asserted of the yardstick first)
    assert 0 < len(alone['ids']) < len(full['ids']) and set(alone['ids'].tolist()) < set(full['ids'].tolist())
    assert alone['count'].max() > 0 and (full['count'] >= alone['count']).all()
    for planes in (ALL29, CLASSES, MIX):
        for ctype_mask in (0x7F, INTER):
            feats = features(table, ptable, pc, idx, planes, ctype_mask)
            for Q in (0, 1, 2):
                want = results_of(feats, planes, Q)
                got = ctx.poses_fingerprints(planes, ctype_mask, n_refs=Q, bits=True)
                assert differences(got, want, KEYS) == [], (planes, ctype_mask, Q)
                NP, U = bin(planes).count('1'), len(want['ids'])
                assert got['planes'] == planes and got['bits'].shape == (P, NP, (U + 63) // 64) and got['occupancy'].shape == (U, NP)
                info = ctx.poses_fingerprints_info()
                assert (info['poses'], info['n_refs'], info['nodes'], info['planes'], info['words']) == (P, Q, U, NP, NP * ((U + 63) // 64))
                if U % 64:      # the padding bits of the last word
                    assert int((got['bits'][:, :, -1] >> np.uint64(U % 64)).max()) == 0
                assert np.array_equal(fp.unpack(got), want['sel'])      # plane order: the set bits of the mask, ascending
    if name == 'main':      # the one-type mask drops ring records (asserted of the yardstick's input)
        assert (ptable['atom_plane']['ctype'] != CT['INTER']).any() and (ptable['atom_plane']['ctype'] == CT['INTER']).any()
        want = yardstick(table, ptable, pc, idx, ALL29, 0x7F, 1, all_pairs=True)
        got = ctx.poses_fingerprints(ALL29, n_refs=1, all_pairs=True)
        assert P == 70 and differences(got, want, ('ids', 'count', 'cross', 'occupancy', 'inter')) == []
        assert np.array_equal(got['inter'], got['inter'].T) and np.array_equal(np.diagonal(got['inter']), got['count'])
        assert np.array_equal(got['inter'][:, 0], got['cross'][:, 0])
    ctx.close()


@pytest.mark.gpu
def test_poses_far_away():
    pc, idx, x, h = case('main')
    x, h = x[:7].copy(), h[:7]
    x[3] += np.float32(100.0)
    ctx = _ctx(pc, idx)
    table, ptable = both(ctx, x, h)
    for planes in (ALL29, CLASSES):
        got = ctx.poses_fingerprints(planes, n_refs=2, bits=True)
        assert differences(got, yardstick(table, ptable, pc, idx, planes, n_refs=2), KEYS) == []
        assert got['count'][3] == 0 and not got['cross'][3].any() and not got['bits'][3].any() and got['count'].max() > 0
    # every pose away, class planes alone: no column at all
    far = x + np.float32(100.0)
    table, ptable = both(ctx, far, h)
    assert len(table['i']) == 0
    assert yardstick(table, ptable, pc, idx, CLASSES)['ids'].shape == (0,)
    got = ctx.poses_fingerprints(CLASSES, n_refs=2, all_pairs=True, bits=True)
    assert got['ids'].shape == (0,) and got['count'].tolist() == [0] * 7 and got['cross'].tolist() == [[0, 0]] * 7
    assert got['occupancy'].shape == (0, 14) and got['bits'].shape == (7, 14, 0) and not got['inter'].any()
    assert ctx.poses_fingerprints_info()['nodes'] == 0
    ctx.close()


@pytest.mark.gpu
def test_chunks_merge_and_run_pose_fingerprints():
    pc, idx, x, h = case('main')
    ctx = _ctx(pc, idx)
    table, ptable = both(ctx, x, h)
    whole = ctx.poses_fingerprints(ALL29, n_refs=2)
    assert differences(whole, yardstick(table, ptable, pc, idx, ALL29, n_refs=2)) == []
    parts = []
    for a, b in ((2, 30), (30, 70)):
        both(ctx, np.concatenate([x[:2], x[a:b]]), np.concatenate([h[:2], h[a:b]]))
        parts.append(ctx.poses_fingerprints(ALL29, n_refs=2))
    assert differences(fp.merge(parts), whole) == []
    ctx.close()
    # end to end: the default reference is the resident pose, in front of every chunk
    ic = InteractionComplex(copy.copy(pc))
    one = ic.run_pose_fingerprints(np.asarray(idx), x, h, *PARAMS, classes='all')
    keys = ('ids', 'count', 'cross', 'occupancy', 'reference_count', 'reference_cross')
    chunked = ic.run_pose_fingerprints(np.asarray(idx), x, h, *PARAMS, classes='all', chunk=32)
    assert differences(chunked, one, keys) == [] and one['planes'] == fp.planes(None, 'all') and one['level'] == 'residue'
    atoms, rows = poses.movable(pc, idx)
    xx, hh = np.concatenate([pc.xyz[atoms][None].astype(np.float32), x]), np.concatenate([pc.h_xyz[rows][None], h])
    table, ptable = both(ic._ctx, xx, hh)
    want = yardstick(table, ptable, pc, idx, fp.planes(None, 'all'), n_refs=1)
    assert np.array_equal(one['ids'], want['ids']) and np.array_equal(one['occupancy'], want['occupancy'])
    assert np.array_equal(one['count'], want['count'][1:]) and np.array_equal(one['cross'], want['cross'][1:])
    assert np.array_equal(one['reference_count'], want['count'][:1])
    # pose 0 of synth.poses_of is the home pose: it recovers itself
    assert fp.tanimoto(one)[0, 0] == 1.0 and one['cross'][0, 0] == one['count'][0] == one['reference_count'][0] > 0
    plain = ic.run_pose_fingerprints(np.asarray(idx), x, h, *PARAMS)
    assert (one['count'] >= plain['count']).all() and one['count'].sum() > plain['count'].sum() and len(fp.plane_names(one['planes'])) == 28
    ic._ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
@pytest.mark.gpu
def test_a_launch_voids_nothing_and_same_arguments_do_no_work():
    pc, idx, x, h = case('main')
    ctx = _ctx(pc, idx)
    counts = ctx.run_launch(*PARAMS)
    assert counts['atom_atom'] > 0 and len(ctx.residue_pairs()['res_a']) > 0
    ptable = ctx.poses_planes(x[:9])
    table = ctx.poses_contacts(x[:9], h[:9], *PARAMS)
    before = _fetch_everything(ctx)
    first = ctx.poses_fingerprints(ALL29, n_refs=2, all_pairs=True, bits=True)
    assert differences(first, yardstick(table, ptable, pc, idx, ALL29, n_refs=2), KEYS) == []
    assert _same_bytes(_fetch_everything(ctx), before)
    launches = ctx.poses_fingerprints_info()['launches']
    again = ctx.poses_fingerprints(ALL29, n_refs=2, all_pairs=True, bits=True)
    assert ctx.poses_fingerprints_info()['launches'] == launches and _same_bytes(again, first)      # no work the second time
    # the old entry after the new one remakes the result, and the reverse
    old = ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    assert ctx.poses_fingerprints_info()['launches'] == launches + 1 and old['planes'] == ALL15
    assert differences(old, yardstick(table, ptable, pc, idx, ALL15, n_refs=2), KEYS) == []
    back = ctx.poses_fingerprints(ALL29, n_refs=2, all_pairs=True, bits=True)
    assert ctx.poses_fingerprints_info()['launches'] == launches + 2 and _same_bytes(back, first)
    # without a bit from 15 on the new entry is the old one: the same arguments through either do no work
    info = np.zeros(8, np.int64)
    assert ctx._L.arp_poses_fingerprints_planes_launch(ctx._h, ALL15, 0x7F, 1, 2, _p(info)) == _capi.ARP_OK and info[6] == launches + 3
    assert ctx._L.arp_poses_fingerprints_launch(ctx._h, ALL15, 0x7F, 1, 2, _p(info)) == _capi.ARP_OK and info[6] == launches + 3
    assert _same_bytes(ctx.poses_fingerprints(ALL15, n_refs=2, bits=True), old)
    assert _same_bytes(_fetch_everything(ctx), before)
    ctx.close()


@pytest.mark.gpu
def test_a_class_plane_result_goes_with_either_source():
    pc, idx, x, h = case('phe')
    m = tp._mask(pc, idx)
    ctx = _ctx(pc, idx)
    x, h = x[:9], h[:9]

    def make(planes=ALL29):
        both(ctx, x, h)
        got = ctx.poses_fingerprints(planes, n_refs=1)
        assert _fetch_rc(ctx)[0] == _capi.ARP_OK
        return got
    first = make()
    ctx.poses_planes_summary(x)                                  # a new poses-planes result, of the same poses
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG and 'no result' in _fetch_rc(ctx)[1]
    assert ctx.poses_fingerprints_info()['poses'] == 0
    assert _same_bytes(ctx.poses_fingerprints(ALL29, n_refs=1), first)      # both sources are valid: made again
    ctx.set_plane_atoms(pc)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG
    with pytest.raises(ValueError, match='no poses-planes result'):
        ctx.poses_fingerprints(ALL29, n_refs=1)
    make()
    ctx.poses_summary(x, h, *PARAMS)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG
    make()
    ctx.set_selection(m)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG
    with pytest.raises(ValueError, match='no poses result'):
        ctx.poses_fingerprints(ALL29, n_refs=1)
    ctx.set_plane_atoms(pc)
    make()
    ctx.set_complex(pc)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG
    ctx.set_selection(m)
    ctx.set_plane_atoms(pc)
    # a result without class planes is not touched by the poses-planes calls
    plain = make(ALL15)
    launches = ctx.poses_fingerprints_info()['launches']
    ctx.poses_planes_summary(x)
    ctx.set_plane_atoms(pc)
    assert _fetch_rc(ctx)[0] == _capi.ARP_OK and _same_bytes(ctx.poses_fingerprints(ALL15, n_refs=1), plain)
    assert ctx.poses_fingerprints_info()['launches'] == launches
    ctx.close()


@pytest.mark.gpu
def test_every_refusal_names_its_cause_and_touches_nothing():
    pc, idx, x, h = case('main')
    x, h = x[:9], h[:9]
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(tp._mask(pc, idx))
    L, hd = ctx._L, ctx._h
    info = np.zeros(8, np.int64)

    def refused(word, planes=ALL29, ctype_mask=0x7F, flags=1, n_refs=0, code=_capi.ARP_E_ARG, entry='arp_poses_fingerprints_planes_launch'):
        rc = getattr(L, entry)(hd, planes, ctype_mask, flags, n_refs, _p(info))
        msg = L.arp_last_error(hd).decode()
        assert rc == code and word in msg and entry + ':' in msg, (word, rc, msg)
    refused('no poses result')
    ctx.poses_contacts(x, h, *PARAMS)
    refused('no poses-planes result')
    ctx.set_plane_atoms(pc)
    refused('no poses-planes result')
    ptable = ctx.poses_planes(x)
    table = ctx.poses_contacts(x, h, *PARAMS)
    good = ctx.poses_fingerprints(ALL29, n_refs=2, bits=True)
    launches = ctx.poses_fingerprints_info()['launches']
    refused('planes mask of 0', planes=0)
    refused('beyond the 29 planes', planes=1 << 29)
    refused('beyond the 15 SIFt bits', planes=1 << 15, entry='arp_poses_fingerprints_launch')      # the old entry stays as it was
    refused('ARP_POSEFP_BY_RESIDUE', flags=0)
    refused('ARP_POSEFP_BY_RESIDUE', planes=1 << 25, flags=2)
    refused('ctype_mask of 0', ctype_mask=0)
    refused('beyond the 7 contact types', ctype_mask=0x80)
    refused('unknown flag', flags=5)
    refused('n_refs', n_refs=-1)
    refused('n_refs', n_refs=10)
    ctx.run_enqueue(*PARAMS)
    refused('not been waited for')
    ctx.run_wait()
    assert L.arp_poses_fingerprints_planes_launch(None, ALL29, 0x7F, 1, 0, _p(info)) == _capi.ARP_E_ARG
    assert L.arp_poses_fingerprints_planes_launch(hd, ALL29, 0x7F, 1, 0, None) == _capi.ARP_E_ARG
    assert ctx.poses_fingerprints_info()['launches'] == launches and _same_bytes(ctx.poses_fingerprints(ALL29, n_refs=2, bits=True), good)
    assert ctx.poses_fingerprints_info()['launches'] == launches      # ... the resident result is the one it was
    # another P
    ctx.poses_planes_summary(x[:8])
    refused('differ in P or S')
    # the same P, one float of the last pose differs by one step
    other = x.copy()
    other[-1, -1, 2] = np.nextafter(other[-1, -1, 2], np.float32(np.inf))
    ctx.poses_planes_summary(other)
    refused('made from different poses')
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG and 'no result' in _fetch_rc(ctx)[1]      # no fingerprint result is left ...
    assert ctx.poses_info()['poses'] == 9 and ctx.poses_planes_info()['poses'] == 9        # ... and both sources stay
    refused('made from different poses', planes=1 << 25)
    got = ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)                               # the atom-atom part alone does not ask
    assert differences(got, yardstick(table, ptable, pc, idx, ALL15, n_refs=2), KEYS) == []
    ctx.poses_planes_summary(x)
    assert _same_bytes(ctx.poses_fingerprints(ALL29, n_refs=2, bits=True), good)
    ctx.close()


@pytest.mark.gpu
def test_a_caller_owned_stream():
    from test_gpu_paths import _hip_runtime
    pc, idx, x, h = case('lys')
    ctx = _ctx(pc, idx)
    table, ptable = both(ctx, x, h)
    want = ctx.poses_fingerprints(ALL29, n_refs=2, bits=True)
    assert differences(want, yardstick(table, ptable, pc, idx, ALL29, n_refs=2), KEYS) == []
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    ctx.poses_summary(x, h, *PARAMS)
    ctx.poses_planes_summary(x)
    got = ctx.poses_fingerprints(ALL29, n_refs=2, bits=True)
    assert _same_bytes(got, want)
    ctx.use_stream(0)                                                 # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0
