"""Library fingerprints with the ring and amide classes as planes (arp_library_fingerprints_planes_launch, Context.library_fingerprints
with a mask or reference mask beyond bit 14, library_fingerprints.reference_from_plane_records / reference_from_pose(planes_result=...),
ligand_library.plane_fingerprints / ligand_side, run_library_fingerprints(classes=...)).

Two yardsticks, neither the code under test:

  (H) plain Python in this file over the tables ``Context.library_planes`` and ``Context.library_contacts`` fetch — pinned to the
      definition by tests/test_library_planes.py and tests/test_ligand_library.py — and the receptor pack's ``res_id``, ``ring_res``
      and ``amide_res``: an entity is the ligand's when its id lies behind the receptor's, a row's features are a set of (node,
      plane), and ``ids``, ``count``, ``cross``, ``occupancy``, the packed ``bits`` and the q32 best table follow from the sets with
      Python integers.  It does not import ``ligand_library.plane_fingerprints``.
  (P) the pose route: ``poses_fingerprints`` with classes on ``complex_of(receptor, ligand)`` for one ligand.  Compared only after
      the test has asserted, on the host, that every receptor ring's ``ring_res`` equals ``res_id`` of the first atom of its path:
      for any other receptor the two routes differ by contract (the node of a receptor ring).

The cases are the small ones of tests/test_library_planes.py — ``main`` (L = 7, 16 poses, one ligand without poses) and ``docked``
(all of its hand-docked poses: five of the arylamide, one of the amine, one of the halide, two of the biaryl, 9 in all) — on
RELABELLED packs as tests/test_pose_plane_fingerprints.py relabels its own: every ``hbond donor`` with a bonded heavy neighbour is
an ``xbond donor`` as well, every ``pos ionisable`` atom gets ``F_RES_MET | F_ELEM_S``; without that,
halogen-pi and Met-sulphur-pi occur on one side at most.  Every comparison is exact equality of integers: no tolerance, no time."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, poses, synth
from arpeggio_amd import library_clusters as lcl
from arpeggio_amd import library_fingerprints as lfp
from arpeggio_amd import library_shortlist as lsl
from arpeggio_amd import ligand_library as ll
from arpeggio_amd import pose_fingerprints as fp
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex
import test_library_planes as tlp
from test_library_fingerprints import BEST, _best_void, _fp_void, _p, _same_bytes, best_of, differences
from test_pose_fingerprints import pack_bits

CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
INTER = 1 << CT['INTER']
PARAMS = (5.0, 0.1, False)
ALL15 = 0x7FFF
ALL29 = (1 << 29) - 1
CLASSES = ALL29 & ~ALL15
MIX = sum(1 << b for b in (1, 9, 20, 25, 28))      # a non-contiguous mix of SIFt bits and class planes
KEYS = ('ids', 'count', 'cross', 'occupancy', 'bits')
TABLES = poses.PLANE_TABLES
NEW = 'arp_library_fingerprints_planes_launch'
OLD = 'arp_library_fingerprints_launch'


# ------------------------------------------------------------------------------------------------------------- cases
def relabelled(pc):
    """The pack with every hbond donor that has a bonded atom an xbond donor too (its single-bond neighbour, where it has none:
    its first bonded atom) and every pos ionisable atom a Met sulphur too."""
    q = copy.copy(pc)
    tm, fl, sb = np.asarray(pc.type_mask).copy(), np.asarray(pc.flags).copy(), np.asarray(pc.sb_nbr).copy()
    bonded = np.diff(np.asarray(pc.bond_off, np.int64)) > 0
    donor = ((tm & config.ATOM_TYPE_BIT['hbond donor']) != 0) & ((sb >= 0) | bonded)
    tm[donor] |= config.ATOM_TYPE_BIT['xbond donor']
    fl[(tm & config.ATOM_TYPE_BIT['pos ionisable']) != 0] |= config.F_RES_MET | config.F_ELEM_S
    for a in np.flatnonzero(donor & (sb < 0)):
        sb[a] = pc.bond_idx[pc.bond_off[a]]
    q.type_mask, q.flags, q.sb_nbr = tm, fl, sb
    return q


@functools.lru_cache(maxsize=None)
def case(name):
    rec, ligs, ps = dict(main=tlp.case_main, docked=tlp.case_docked)[name]()
    return relabelled(rec), tuple(relabelled(l) for l in ligs), ps


REF_POSES = dict(main=(0, 9, 14), docked=(0, 5, 7))      # poses of three different ligands


@functools.lru_cache(maxsize=None)
def receptor_gpu():
    return tlp.device_planes(case('main')[0])


# ------------------------------------------------------------------------------------------------------------- yardstick (H)
def class_features(ptable, rec, planes, ctype_mask):
    """Per global pose the set of (node, plane >= 15) of the ring / amide records, record by record."""
    n, nr, na, nres = rec.n_atoms, rec.n_rings, rec.n_amides, rec.n_residues
    res_id, ring_res, am_res = (np.asarray(v).tolist() for v in (rec.res_id, rec.ring_res, rec.amide_res))
    T = len(ptable['summary'])
    out = [set() for _ in range(T)]

    def records(name, *cols):
        t = ptable[name]
        off = t['pose_off'].astype(np.int64)
        for p in range(T):
            for r in range(off[p], off[p + 1]):
                if (ctype_mask >> int(t['ctype'][r])) & 1:
                    yield (p,) + tuple(int(t[c][r]) for c in cols)

    def put(p, node, plane):
        if (planes >> plane) & 1 and 0 <= node < nres:
            out[p].add((node, plane))
    for p, a, r, mask in records('atom_plane', 'atom', 'ring', 'mask'):
        if (a >= n) != (r >= nr):
            for b in range(5):
                if (mask >> b) & 1:
                    put(p, ring_res[r] if a >= n else res_id[a], (15 if a >= n else 20) + b)
    for p, r1, r2 in records('plane_plane', 'bgn', 'end'):
        if (r1 >= nr) != (r2 >= nr):
            put(p, ring_res[r2] if r1 >= nr else ring_res[r1], 25)
    for p, a1, a2 in records('group_group', 'bgn', 'end'):
        if (a1 >= na) != (a2 >= na):
            put(p, am_res[a2] if a1 >= na else am_res[a1], 26)
    for p, a, r in records('group_plane', 'amide', 'ring'):
        if (a >= na) != (r >= nr):
            put(p, ring_res[r] if a >= na else am_res[a], 27 if a >= na else 28)
    return out


def atom_features(table, rec, planes, ctype_mask):
    """Per global pose the set of (receptor residue, SIFt bit) of the atom-atom records."""
    off = table['pose_off'].astype(np.int64)
    ci, sift, ctype, res_id = (np.asarray(v).tolist() for v in (table['i'], table['sift'], table['ctype'], rec.res_id))
    out = [set() for _ in range(len(off) - 1)]
    for p in range(len(off) - 1):
        for r in range(off[p], off[p + 1]):
            s = sift[r] & planes & ALL15
            if s and (ctype_mask >> ctype[r]) & 1 and 0 <= res_id[ci[r]] < rec.n_residues:
                out[p].update((res_id[ci[r]], b) for b in range(15) if (s >> b) & 1)
    return out


def pose_features(table, ptable, rec, planes, ctype_mask=0x7F):
    return [x | y for x, y in zip(atom_features(table, rec, planes, ctype_mask), class_features(ptable, rec, planes, ctype_mask))]


def ref_features(refs, planes):
    return [{(int(u), b) for u, m in zip(nodes, masks) for b in range(29) if (int(m) & planes) >> b & 1} for nodes, masks in refs]


def results_of(rows, planes, Q):
    """ids, count, cross, occupancy, bits of Q reference rows and the pose rows behind them, sets of (node, plane)."""
    ids = sorted({u for f in rows for u, _ in f})
    axis = [b for b in range(29) if (planes >> b) & 1]
    on = np.zeros((len(rows), len(ids), len(axis)), bool)
    for p, f in enumerate(rows):
        for u, b in f:
            on[p, ids.index(u), axis.index(b)] = True
    return dict(ids=np.array(ids, np.int32), count=np.array([len(f) for f in rows], np.uint32),
                cross=np.array([[len(f & rows[q]) for q in range(Q)] for f in rows], np.uint32).reshape(len(rows), Q),
                occupancy=on[Q:].sum(axis=0).astype(np.uint32).reshape(len(ids), len(axis)), bits=pack_bits(on), on=on,
                planes=planes, n_refs=Q, level='residue')


def yardstick(table, ptable, rec, refs, planes, ctype_mask=0x7F):
    return results_of(ref_features(refs, planes) + pose_features(table, ptable, rec, planes, ctype_mask), planes, len(refs))


def as_reference(feats):
    """A set of (node, plane) as a (nodes, masks) pair."""
    nodes = sorted({u for u, _ in feats})
    return np.array(nodes, np.int32), np.array([sum(1 << b for u, b in feats if u == v) for v in nodes], np.uint32)


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_case():
    """A receptor of 12 atoms in four residues of three, rings 0 (residue 1), 1 (residue 2) and 2 (residue -1: no atom near its
    centre), amides 0 (residue 3) and 1 (residue 2); a ligand of 4 atoms with one ring and one amide: complex ids atoms 12 ... 15,
    ring 3, amide 2.  Two ligands of 2 and 1 poses.
      global pose 0, one record of every (table, side) kind, all INTER:
        atom 12 - ring 0, CARBONPI | DONORPI   ligand atom   -> (1, 15), (1, 17)
        atom 9  - ring 3, CATIONPI             ligand ring   -> (3, 21)
        ring 1  - ring 3                                      -> (2, 25)
        amide 0 - amide 2                                     -> (3, 26)
        amide 2 - ring 0                       ligand amide  -> (1, 27)
        amide 1 - ring 3                       ligand ring   -> (2, 28)
      global pose 1: atom 13 - ring 3 and amide 2 - amide 2 (both the ligand's), atom 4 - ring 1 and ring 0 - ring 1 (neither):
        nothing; atom 14 - ring 2 (residue -1): skipped; atom 15 - ring 1, METSULPHURPI, INTRA_SELECTION -> (2, 19) unless only
        INTER is admitted
      global pose 2 (the second ligand): no record"""
    from helpers import tiny_complex
    rec = tiny_complex(np.arange(36, dtype=np.float64).reshape(12, 3), res_id=[0] * 3 + [1] * 3 + [2] * 3 + [3] * 3,
                       rings=(np.zeros((3, 3)), np.zeros((3, 3)), np.array([1, 2, -1], np.int32)),
                       amides=(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), np.array([3, 2], np.int32)))
    I, S = CT['INTER'], CT['INTRA_SELECTION']
    ap = lambda atom, ring, mask, ct: dict(atom=atom, ring=ring, dist=[4.0] * len(atom), theta=[10.0] * len(atom), mask=mask, ctype=ct)
    pp = lambda bgn, end: dict(bgn=bgn, end=end, dist=[4.0] * len(bgn), dihedral=[5.0] * len(bgn), theta_bgn=[1.0] * len(bgn), theta_end=[2.0] * len(bgn),
                               type1=[0] * len(bgn), type2=[255] * len(bgn), ctype=[I] * len(bgn))
    g = lambda first, second, a, b: {first: a, second: b, 'dist': [4.0] * len(a), 'dihedral': [5.0] * len(a), 'theta': [6.0] * len(a), 'ctype': [I] * len(a)}
    rows = [[dict(atom_plane=ap([9, 12], [3, 0], [2, 1 | 4], [I, I]), plane_plane=pp([1], [3]), group_group=g('bgn', 'end', [0], [2]),
                  group_plane=g('amide', 'ring', [1, 2], [3, 0])),
             dict(atom_plane=ap([4, 13, 14, 15], [1, 3, 2, 1], [1, 1, 1, 16], [I, I, I, S]), plane_plane=pp([0], [1]), group_group=g('bgn', 'end', [2], [2]),
                  group_plane=g('amide', 'ring', [], []))],
            [dict(atom_plane=ap([], [], [], []), plane_plane=pp([], []), group_group=g('bgn', 'end', [], []), group_plane=g('amide', 'ring', [], []))]]
    rows = [[{n: {c: np.asarray(r[n][c], dt) for c, dt in poses.plane_columns(n)} for n in TABLES} for r in lig] for lig in rows]
    return rec, ll.planes_from_rows(rows)


POSE0 = {(1, 15), (1, 17), (3, 21), (2, 25), (3, 26), (1, 27), (2, 28)}


def test_both_host_functions_and_the_yardstick_on_a_hand_made_table():
    rec, t = hand_case()
    assert t['ligand_pose_off'].tolist() == [0, 2, 3]
    assert ll.ligand_side(rec, 'atom', [0, 11, 12, 15]).tolist() == [False, False, True, True]
    assert ll.ligand_side(rec, 'ring', [0, 2, 3]).tolist() == [False, False, True] and ll.ligand_side(rec, 'amide', [1, 2]).tolist() == [False, True]
    with pytest.raises(ValueError):
        ll.ligand_side(rec, 'residue', [0])
    assert ll.plane_fingerprints(t, rec) == [POSE0, {(2, 19)}, set()]
    assert ll.plane_fingerprints(t, rec, INTER) == [POSE0, set(), set()]
    assert ll.plane_fingerprints(t, rec, 1 << CT['INTRA_SELECTION']) == [set(), {(2, 19)}, set()]
    assert class_features(t, rec, CLASSES, 0x7F) == [POSE0, {(2, 19)}, set()] and class_features(t, rec, CLASSES, INTER) == [POSE0, set(), set()]
    # a plane that is not selected drops its features only
    assert class_features(t, rec, CLASSES & ~(1 << 17) & ~(1 << 28), 0x7F) == [POSE0 - {(1, 17), (2, 28)}, {(2, 19)}, set()]
    # a node outside the residues is skipped: an amide without a residue as the ring without one
    q = copy.copy(rec)
    q.amide_res = np.array([-1, 2], np.int32)
    assert ll.plane_fingerprints(t, q)[0] == POSE0 - {(3, 26)} == class_features(t, q, CLASSES, 0x7F)[0]
    # the resident ring_res names the node, not the first atom of a path (there is none here), and not the posed residue
    q = copy.copy(rec)
    q.ring_res = np.array([0, 2, 3], np.int32)
    assert ll.plane_fingerprints(t, q)[0] == (POSE0 - {(1, 15), (1, 17), (1, 27)}) | {(0, 15), (0, 17), (0, 27)}
    assert ll.plane_fingerprints(t, q)[1] == {(2, 19), (3, 15)} == class_features(t, q, CLASSES, 0x7F)[1]
    # the numbers that follow from the sets, pose 0 as the one reference
    r = results_of([POSE0, POSE0, {(2, 19)}, set()], CLASSES, 1)
    assert r['ids'].tolist() == [1, 2, 3] and r['count'].tolist() == [7, 7, 1, 0] and r['cross'].tolist() == [[7], [7], [0], [0]]
    assert r['occupancy'].shape == (3, 14) and r['occupancy'].sum() == 8 and r['occupancy'][1, 4] == 1 and r['bits'].shape == (4, 14, 1)
    assert [int(w) for w in r['bits'][1, :, 0]] == [1, 0, 1, 0, 0, 0, 4, 0, 0, 0, 2, 4, 1, 2]
    assert np.array_equal(fp.unpack(r), r['on']) and fp.tanimoto(r).tolist() == [[1.0], [1.0], [0.0], [0.0]]
    b = best_of(r, t['ligand_pose_off'])
    assert b['best_pose'].tolist() == [[0], [2]] and b['tanimoto_q32'].tolist() == [[1 << 32], [0]] and differences(lfp.best(r, t['ligand_pose_off']), b, BEST) == []


def test_reference_from_plane_records_and_the_merge_per_node():
    rec, t = hand_case()
    n, m = lfp.reference_from_plane_records(t, rec, 0)
    assert n.dtype == np.int32 and m.dtype == np.uint32
    assert n.tolist() == [1, 2, 3] and m.tolist() == [(1 << 15) | (1 << 17) | (1 << 27), (1 << 25) | (1 << 28), (1 << 21) | (1 << 26)]
    assert as_reference(POSE0)[0].tolist() == n.tolist() and as_reference(POSE0)[1].tolist() == m.tolist()
    assert [v.tolist() for v in lfp.reference_from_plane_records(t, rec, 1)] == [[2], [1 << 19]]
    assert [v.tolist() for v in lfp.reference_from_plane_records(t, rec, 1, ctype_mask=INTER)] == [[], []]
    assert [v.tolist() for v in lfp.reference_from_plane_records(t, rec, 2)] == [[], []]
    # every pose joined; a selection drops planes, and a node it empties
    assert [v.tolist() for v in lfp.reference_from_plane_records(t, rec)] == [[1, 2, 3], [m[0], m[1] | (1 << 19), m[2]]]
    assert [v.tolist() for v in lfp.reference_from_plane_records(t, rec, 0, planes=(1 << 25) | (1 << 26))] == [[2, 3], [1 << 25, 1 << 26]]
    with pytest.raises(ValueError, match='no global pose'):
        lfp.reference_from_plane_records(t, rec, 3)
    # merged with the atom-atom features of the same pose, per node
    lib = dict(i=np.array([0, 4, 9], np.int32), sift=np.array([1 << 3, 1 << 5, 1 << 7], np.uint16), ctype=np.array([CT['INTER']] * 3, np.uint8),
               pose_off=np.array([0, 2, 3, 3], np.uint64))
    n, m = lfp.reference_from_pose(lib, 0, planes_result=t, receptor=rec)
    assert n.tolist() == [0, 1, 2, 3] and m.tolist() == [1 << 3, (1 << 5) | (1 << 15) | (1 << 17) | (1 << 27), (1 << 25) | (1 << 28), (1 << 21) | (1 << 26)]
    assert [v.tolist() for v in lfp.reference_from_pose(lib, 1, planes_result=t, receptor=rec)] == [[2, 3], [1 << 19, 1 << 7]]
    assert [v.tolist() for v in lfp.reference_from_pose(lib, 0, planes=CLASSES, planes_result=t, receptor=rec)] == [[1, 2, 3], [(1 << 15) | (1 << 17) | (1 << 27), (1 << 25) | (1 << 28), (1 << 21) | (1 << 26)]]
    assert [v.tolist() for v in lfp.reference_from_pose(lib, 0, rec.res_id)] == [[0, 1], [1 << 3, 1 << 5]]      # without: as before
    with pytest.raises(ValueError, match="level='residue'"):
        lfp.reference_from_pose(lib, 0, planes_result=t, receptor=rec, level='atom')
    with pytest.raises(ValueError, match="receptor's pack"):
        lfp.reference_from_pose(lib, 0, planes_result=t)


def test_every_new_refusal_of_validate_by_name_and_the_entry_is_declared():
    good = lfp.references([([3, 5], [1, 1 << 28]), {7: CLASSES}], classes=True)
    assert good['ref_planes'].tolist() == [1, 1 << 28, CLASSES] and lfp.validate(good, 10, classes=True) is good
    assert lfp.ALL_CLASS_PLANES == ALL29 and lfp.N_ALL_PLANES == 29
    with pytest.raises(ValueError, match='beyond the 15 SIFt bits'):      # not told so: the 15 bits of before
        lfp.validate(good)
    with pytest.raises(ValueError, match='beyond the 15 SIFt bits'):
        lfp.references([([3], [1 << 15])])
    bad = dict(good, ref_planes=np.array([1, 1 << 29, 1], np.int64))
    with pytest.raises(ValueError, match='beyond the 29 planes'):
        lfp.validate(bad, classes=True)
    with pytest.raises(ValueError, match='beyond the 15 SIFt bits'):
        lfp.validate(bad)
    with pytest.raises(ValueError, match='beyond the 29 planes'):
        lfp.references([{2: 1 << 29}], classes=True)
    with pytest.raises(ValueError, match='strictly ascending'):           # an earlier cause wins
        lfp.validate(dict(bad, ref_node=np.array([5, 3, 7])), classes=True)
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert NEW in _capi.SYMBOLS and 'int %s(' % NEW in hdr
    rec, ligs, ps = case('docked')
    off, x, h = ll.flatten_poses(ll.pack(ligs), ps)
    with pytest.raises(ValueError, match="level='residue'"):
        InteractionComplex(copy.copy(rec)).run_library_fingerprints(ligs, off, x, h, [{1: 1}], level='atom', classes='all')


@functools.lru_cache(maxsize=None)
def oracle_tables(name):
    """The ring / amide table of a relabelled case from the oracle alone, and the receptor rings whose posed residue differs."""
    rec, ligs, ps = case(name)
    per = tlp.oracle_rows(rec, ligs, ps)
    return ll.planes_from_rows([[rows for rows, _ in lig] for lig in per]), sum(taken for lig in per for _, taken in lig)


def test_the_oracle_alone_meets_the_coverage_condition():
    """Asserted of the oracle's rows of the two relabelled cases, before any device is compared: every one of the 14 class planes
    occurs on a participating record, records that must be left out exist — both sides the ligand's, neither —, and a ligand
    atom takes a receptor ring's posed residue over, so the posed residue and the resident one differ."""
    planes, both_, neither, taken = set(), 0, 0, 0
    for name in ('main', 'docked'):
        rec, ligs, ps = case(name)
        home = tlp.planes_cpu(rec)
        t, k = oracle_tables(name)
        feats = class_features(t, home, CLASSES, 0x7F)
        assert feats == ll.plane_fingerprints(t, home)
        planes |= {q for f in feats for _, q in f}
        taken += k
        n, nr, na = rec.n_atoms, rec.n_rings, rec.n_amides
        ap, pp, gg, gp = (t[k_] for k_ in TABLES)
        sides = [(ap['atom'] >= n, ap['ring'] >= nr), (pp['bgn'] >= nr, pp['end'] >= nr), (gg['bgn'] >= na, gg['end'] >= na), (gp['amide'] >= na, gp['ring'] >= nr)]
        both_ += sum(int((a & b).sum()) for a, b in sides)
        neither += sum(int((~a & ~b).sum()) for a, b in sides)
        print(name, sorted({q for f in feats for _, q in f}), [len(t[k_]['ctype']) for k_ in TABLES])
    assert planes == set(range(15, 29)), sorted(set(range(15, 29)) - planes)
    assert both_ > 0 and neither > 0 and taken > 0


# ------------------------------------------------------------------------------------------------------------- GPU: helpers
def context(ligs):
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)
    ctx.set_complex(receptor_gpu())
    ctx.set_ligand_library(lib)
    ctx.set_ligand_library_planes(lib)
    return ctx, lib


def both(ctx, lib, ps):
    """Both library results of the same poses, fetched."""
    off, x, h = ll.flatten_poses(lib, ps)
    return ctx.library_contacts(off, x, h, *PARAMS), ctx.library_planes(off, x)


def pose_refs(table, ptable, rec, which):
    return [lfp.reference_from_pose(table, t, planes_result=ptable, receptor=rec) for t in which]


def check(ctx, table, ptable, rec, refs, planes, ctype_mask=0x7F):
    """A launch against (H): the four arrays, the bit matrix with its padding and plane order, the best table."""
    got = ctx.library_fingerprints(lfp.references(refs, rec.n_residues, classes=True), planes, ctype_mask, bits=True)
    want = yardstick(table, ptable, rec, refs, planes, ctype_mask)
    assert differences(got, want, KEYS) == [], (hex(planes), hex(ctype_mask), len(refs))
    NP, U, P = bin(planes).count('1'), len(want['ids']), len(want['count'])
    assert got['planes'] == planes and got['n_refs'] == len(refs) and got['bits'].shape == (P, NP, (U + 63) // 64) and got['occupancy'].shape == (U, NP)
    if U % 64:      # the padding bits of the last word
        assert int((got['bits'][:, :, -1] >> np.uint64(U % 64)).max()) == 0
    assert np.array_equal(fp.unpack(got), want['on'])      # plane order: the set bits of the mask, ascending
    info = ctx.library_fingerprints_info()
    assert (info['rows'], info['n_refs'], info['nodes'], info['planes'], info['words']) == (P, len(refs), U, NP, NP * ((U + 63) // 64))
    if refs:
        assert differences(ctx.library_fingerprints_best(), best_of(want, table['ligand_pose_off']), BEST) == []
    return got, want


def planes_resident(ctx):
    """The resident library-planes result, fetched without a launch."""
    info = ctx.library_planes_info()
    out, n = {}, C.c_int64(0)
    summary = np.empty((info['poses'], 16), np.uint32)
    for t, name in enumerate(TABLES):
        tab, args = ctx._plane_table_buffers(name, info[name], info['poses'] + 1)
        ctx._check(ctx._L.arp_library_planes_fetch(ctx._h, t, info[name], _p(tab['pose_off']), *args, _p(summary) if t == 0 else None, C.byref(n)), 'fetch')
        out[name] = tab
    out['summary'] = summary
    return out


# ------------------------------------------------------------------------------------------------------------- GPU: contents
@pytest.mark.gpu
@pytest.mark.parametrize('name', ('main', 'docked'))
def test_contents(name):
    rec_cpu, ligs, ps = case(name)
    rec = receptor_gpu()
    ctx, lib = context(ligs)
    table, ptable = both(ctx, lib, ps)
    T = len(ptable['summary'])
    assert sum(len(ptable[k]['ctype']) for k in TABLES) > 0 and len(table['i']) > 0 and T == (16 if name == 'main' else 9)
    for ctype_mask in (0x7F, INTER):      # the host route against (H) on the device's tables
        assert ll.plane_fingerprints(ptable, rec, ctype_mask) == class_features(ptable, rec, CLASSES, ctype_mask)
    refs3 = pose_refs(table, ptable, rec, REF_POSES[name])
    feats = pose_features(table, ptable, rec, ALL29)
    for q, t in enumerate(REF_POSES[name]):      # a reference made from a pose holds that pose's features
        assert ref_features(refs3, ALL29)[q] == feats[t]
    assert len({int(ll.ligand_of(table)[t]) for t in REF_POSES[name]}) == 3 and all(len(n) > 0 for n, _ in refs3)
    full, alone = yardstick(table, ptable, rec, [], ALL29), yardstick(table, ptable, rec, [], CLASSES)
    assert 0 < len(alone['ids']) <= len(full['ids']) and set(alone['ids'].tolist()) <= set(full['ids'].tolist())
    assert alone['count'].max() > 0 and (full['count'] >= alone['count']).all() and full['count'].sum() > alone['count'].sum()
    for planes in (ALL29, CLASSES, MIX):
        for ctype_mask in (0x7F, INTER):
            for Q in (0, 1, 3):
                got, want = check(ctx, table, ptable, rec, refs3[:Q], planes, ctype_mask)
                for q, t in enumerate(REF_POSES[name][:Q]):      # a reference that is a pose of the launch equals that pose's row
                    if ctype_mask == 0x7F:
                        assert got['count'][q] == got['count'][Q + t] == got['cross'][Q + t, q] and np.array_equal(got['cross'][q], got['cross'][Q + t])
    if name == 'docked':      # the one-type mask drops ring records (asserted of the yardstick's input)
        cts = np.concatenate([ptable[k]['ctype'] for k in TABLES])
        assert (cts != CT['INTER']).any() and (cts == CT['INTER']).any()
    ctx.close()


@pytest.mark.gpu
def test_a_reference_feature_no_pose_has_and_one_whose_plane_is_not_selected():
    rec_cpu, ligs, ps = case('docked')
    rec = receptor_gpu()
    ctx, lib = context(ligs)
    table, ptable = both(ctx, lib, ps)
    planes = ALL29 & ~(1 << 26)
    home = pose_refs(table, ptable, rec, (0,))[0]
    assert (home[1] >> 25 & 1).any()      # the face-to-face pose stacks on a receptor ring
    touched = set(yardstick(table, ptable, rec, [], ALL29)['ids'].tolist())
    untouched = next(r for r in range(rec.n_residues) if r not in touched)
    dropped = next(r for r in range(rec.n_residues) if r not in touched and r != untouched)
    more = dict(zip(home[0].tolist(), home[1].tolist()))
    more[untouched] = (1 << 25) | (1 << 21)
    more[dropped] = 1 << 26                                  # its only plane is not selected
    plus = (np.array(sorted(more), np.int32), np.array([more[k] for k in sorted(more)], np.uint32))
    got, want = check(ctx, table, ptable, rec, [home, plus], planes)
    ids = got['ids'].tolist()
    u = ids.index(untouched)
    # the node no pose touches: a column with occupancy 0 that counts in the reference and lowers the Tanimoto
    assert not got['occupancy'][u].any() and got['count'][1] == got['count'][0] + 2 and got['cross'][1, 0] == got['count'][0]
    tan = lfp.tanimoto(got)
    assert tan[2, 0] == 1.0 and tan[2, 1] == got['count'][0] / (got['count'][0] + 2) < 1.0
    assert dropped not in ids and len(ids) == len(set(yardstick(table, ptable, rec, [], planes)['ids'].tolist())) + 1
    ctx.close()


@pytest.mark.gpu
def test_one_ligand_equals_the_pose_route():
    rec_cpu, ligs, _ = case('main')
    # the stand-in receptor has rings whose nearest atom lies in another residue than their path: there the two routes differ by
    # contract.  (P) is asked of the receptor WITHOUT those rings, and the condition is asserted of what the device then holds
    first = np.array([int(rec_cpu.res_id[int(a[0])]) for a in rec_cpu.ring_atoms])
    keep = np.flatnonzero(tlp.planes_cpu(rec_cpu).ring_res == first)
    assert 0 < len(keep) < rec_cpu.n_rings
    cut = copy.copy(rec_cpu)
    cut.ring_atoms = [rec_cpu.ring_atoms[r] for r in keep]
    cut.ring_center, cut.ring_normal, cut.ring_res = rec_cpu.ring_center[keep], rec_cpu.ring_normal[keep], rec_cpu.ring_res[keep]
    rec = tlp.device_planes(cut)
    assert [int(v) for v in rec.ring_res] == [int(rec.res_id[int(a[0])]) for a in rec.ring_atoms] and rec.n_rings == len(keep)
    l = 4                                                    # the arylamide: a ring, an amide; five poses over a ring that is left
    _, c, nrm = tlp._ring(rec, 'PHE', 0)
    ps = [None] * len(ligs)
    ps[l] = synth.library_poses_of(rec, ligs[l], c + 3.8 * nrm, 5, seed=7, shift=2.0)
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    ctx.set_ligand_library_planes(lib)
    table, ptable = both(ctx, lib, ps)
    refs = pose_refs(table, ptable, rec, (0, 1))
    got = ctx.library_fingerprints(lfp.references(refs, classes=True), ALL29)
    ctx.close()
    far = np.array([1000.0, 0.0, 0.0])
    home = tlp.device_planes(ll.complex_of(rec, ligs[l], ligs[l].xyz + far.astype(np.float32), ligs[l].h_xyz + far))
    other = _capi.Context(0)
    other.set_complex(home)
    other.set_selection(tlp._lig_mask(rec, ligs[l]))
    other.set_plane_atoms(home)
    other.poses_summary(ps[l][0], ps[l][1], *PARAMS)
    other.poses_planes_summary(ps[l][0])
    want = other.poses_fingerprints(ALL29, n_refs=2)
    other.close()
    assert np.array_equal(got['ids'], want['ids']) and len(want['ids']) > 3 and (want['count'] > 0).all()
    assert np.array_equal(got['count'][2:], want['count']) and np.array_equal(got['cross'][2:], want['cross'])
    assert np.array_equal(got['count'][:2], want['count'][:2]) and np.array_equal(got['cross'][:2], want['cross'][:2])
    classes_alone = yardstick(table, ptable, rec, [], CLASSES)
    assert classes_alone['count'].sum() > 0      # the class planes take part in what was compared


@pytest.mark.gpu
def test_poses_far_away():
    rec_cpu, ligs, ps = case('docked')
    rec = receptor_gpu()
    ctx, lib = context(ligs)
    moved = [(p[0].copy(), p[1].copy()) for p in ps]
    moved[0][0][3] += np.float32(100.0)                      # global pose 3
    moved[0][1][3] += 100.0
    table, ptable = both(ctx, lib, moved)
    refs = pose_refs(table, ptable, rec, (0, 5))
    for planes in (ALL29, CLASSES):
        got, _ = check(ctx, table, ptable, rec, refs, planes)
        assert got['count'][2 + 3] == 0 and not got['cross'][2 + 3].any() and not got['bits'][2 + 3].any() and got['count'].max() > 0
    # every pose away, class planes alone, no reference: no column at all
    away = [(p[0] + np.float32(100.0), p[1] + 100.0) for p in ps]
    table, ptable = both(ctx, lib, away)
    assert len(table['i']) == 0 and yardstick(table, ptable, rec, [], CLASSES)['ids'].shape == (0,)
    got = ctx.library_fingerprints(None, CLASSES, bits=True)
    assert got['ids'].shape == (0,) and got['count'].tolist() == [0] * 9 and got['cross'].shape == (9, 0)
    assert got['occupancy'].shape == (0, 14) and got['bits'].shape == (9, 14, 0) and ctx.library_fingerprints_info()['nodes'] == 0
    # ... and with a reference the columns are the reference's alone
    ref = (np.array([2], np.int32), np.array([(1 << 25) | 1], np.uint32))
    got, _ = check(ctx, table, ptable, rec, [ref], ALL29)
    assert got['ids'].tolist() == [2] and got['count'].tolist() == [2] + [0] * 9
    ctx.close()


@pytest.mark.gpu
def test_shortlist_and_clusters_over_the_class_plane_fingerprint():
    rec_cpu, ligs, ps = case('main')
    rec = receptor_gpu()
    ctx, lib = context(ligs)
    table, ptable = both(ctx, lib, ps)
    refs = pose_refs(table, ptable, rec, REF_POSES['main'])
    got, want = check(ctx, table, ptable, rec, refs, CLASSES)
    lo = table['ligand_pose_off']
    assert (want['count'][3:] > 0).sum() > 3
    for unit in ('ligands', 'poses'):
        for ref in (0, 2, -1):
            sc = lsl.scores('tanimoto', count=want['count'], cross=want['cross'], n_refs=3, ref=ref)
            short = ctx.library_shortlist('tanimoto', unit=unit, ref=ref, k=5)
            order = lsl.order(sc, lo, unit, 5)
            assert short['pose'].tolist() == order.tolist() and short['score'].tolist() == [sc[t] for t in order], (unit, ref)
            assert short['ligand'].tolist() == ll.ligand_of(table)[order].tolist()
    for threshold in (lcl.threshold_q32(0.3), lcl.threshold_q32(1.0)):
        mirror = lcl.leader(want, threshold, ligand_of=lcl.ligands_of(lo))
        cl = ctx.library_clusters(threshold)
        assert [k for k in lcl.PER_POSITION + lcl.PER_CLUSTER if not np.array_equal(cl[k], mirror[k]) or cl[k].dtype != mirror[k].dtype] == []
        assert cl['unassigned'] == mirror['unassigned'] == 0 and 1 < len(cl['leader']) <= 16
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
@pytest.mark.gpu
def test_a_launch_voids_nothing_and_each_entry_remakes_the_others_result():
    rec_cpu, ligs, ps = case('main')
    rec = receptor_gpu()
    ctx, lib = context(ligs)
    hem = np.nonzero(rec.res_id == int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]))[0]
    m = np.zeros(rec.n_atoms, np.uint8)
    m[hem] = 1
    ctx.set_selection(m)
    px, ph = synth.poses_of(rec, hem, 6, seed=11, shift=2.0)
    ctx.poses_contacts(px, ph, *PARAMS)
    ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    pose_launches = ctx.poses_fingerprints_info()['launches']
    table, ptable = both(ctx, lib, ps)
    ctx.library_best(np.arange(16, dtype=np.int64) - 4)
    refs = lfp.references(pose_refs(table, ptable, rec, REF_POSES['main']), classes=True)

    def everything():
        got = ctx._pose_records_fetch('arp_library_contacts_fetch', 'a', 16, len(table['i']))
        n = C.c_int64(0)
        best = dict(n_poses=np.empty(7, np.int64), best_pose=np.empty(7, np.int32), score=np.empty(7, np.int64))
        ctx._check(ctx._L.arp_library_best_fetch(ctx._h, 7, _p(best['n_poses']), _p(best['best_pose']), _p(best['score']), C.byref(n)), 'best')
        return got, best, planes_resident(ctx), ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    before = everything()
    assert _same_bytes(before[2], {k: ptable[k] for k in before[2]})
    first = ctx.library_fingerprints(refs, ALL29, bits=True)      # made and fetched
    first_best = ctx.library_fingerprints_best()
    assert all(_same_bytes(a, b) for a, b in zip(everything(), before)) and ctx.poses_fingerprints_info()['launches'] == pose_launches
    launches = ctx.library_fingerprints_info()['launches']
    # the old entry after the new one remakes the result (the best table goes), and the reverse
    plain = lfp.references([(n, mk & ALL15) for n, mk in pose_refs(table, ptable, rec, REF_POSES['main'])])
    old = ctx.library_fingerprints(plain, ALL15, bits=True)
    assert old['planes'] == ALL15 and _best_void(ctx) and ctx.library_fingerprints_info()['launches'] == launches + 1
    assert differences(old, yardstick(table, ptable, rec, pose_refs(table, ptable, rec, REF_POSES['main']), ALL15), KEYS) == []
    back = ctx.library_fingerprints(refs, ALL29, bits=True)
    assert _same_bytes(back, first) and _same_bytes(ctx.library_fingerprints_best(), first_best)
    # without a bit from 15 on the new entry does what the old one does
    info = np.zeros(8, np.int64)
    a = [np.ascontiguousarray(plain[k]) for k in ('ref_off', 'ref_node', 'ref_planes')]
    assert getattr(ctx._L, NEW)(ctx._h, ALL15, 0x7F, 1, 3, _p(a[0]), _p(a[1]), _p(a[2]), _p(info)) == _capi.ARP_OK
    n = C.c_int64(0)
    again = {k: np.empty_like(old[k]) for k in KEYS}
    ctx._check(ctx._L.arp_library_fingerprints_fetch(ctx._h, len(old['ids']), *(_p(again[k]) for k in KEYS), C.byref(n)), 'fetch')
    assert all(_same_bytes(again[k], old[k]) for k in KEYS)
    assert all(_same_bytes(a_, b) for a_, b in zip(everything(), before))
    ctx.close()


@pytest.mark.gpu
def test_a_class_plane_result_goes_with_either_source_and_a_plain_one_survives():
    rec_cpu, ligs, ps = case('docked')
    rec = receptor_gpu()
    ctx, lib = context(ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    ref = lfp.references([{2: (1 << 25) | 1}], classes=True)

    def make(planes=ALL29):
        ctx.library_summary(off, x, h, *PARAMS)
        ctx.library_planes_summary(off, x)
        got = ctx.library_fingerprints(ref if planes >> 15 else lfp.references([{2: 1}]), planes)
        ctx.library_fingerprints_best()
        assert not _fp_void(ctx) and not _best_void(ctx)
        return got
    first = make()
    ctx.library_planes_summary(off, x)                       # a new library-planes result, of the same poses
    assert _fp_void(ctx) and _best_void(ctx) and ctx.library_fingerprints_info()['rows'] == 0
    assert _same_bytes(ctx.library_fingerprints(ref, ALL29), first)      # both sources are valid: made again
    ctx.set_ligand_library_planes(lib)
    assert _fp_void(ctx) and _best_void(ctx)
    with pytest.raises(ValueError, match='no library-planes result'):
        ctx.library_fingerprints(ref, ALL29)
    make()
    ctx.library_summary(off, x, h, *PARAMS)                  # a new library result
    assert _fp_void(ctx) and _best_void(ctx)
    make()
    ctx.set_ligand_library(lib)                              # a new library (the plane table goes with it)
    assert _fp_void(ctx) and _best_void(ctx)
    with pytest.raises(ValueError, match='no library result'):
        ctx.library_fingerprints(ref, ALL29)
    ctx.set_ligand_library_planes(lib)
    make()
    ctx.set_complex(rec)                                     # a new structure
    assert _fp_void(ctx) and _best_void(ctx)
    # a result without class planes is not touched by the two planes calls
    plain = make(ALL15)
    launches = ctx.library_fingerprints_info()['launches']
    ctx.library_planes_summary(off, x)
    ctx.set_ligand_library_planes(lib)
    assert not _fp_void(ctx) and not _best_void(ctx) and ctx.library_fingerprints_info()['launches'] == launches
    n = C.c_int64(0)
    count = np.empty(10, np.uint32)
    ctx._check(ctx._L.arp_library_fingerprints_fetch(ctx._h, 0, None, _p(count), None, None, None, C.byref(n)), 'fetch')
    assert np.array_equal(count, plain['count'])
    ctx.close()


@pytest.mark.gpu
def test_every_new_refusal_names_its_cause_in_order_and_touches_nothing():
    rec_cpu, ligs, ps = case('docked')
    rec = receptor_gpu()
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    ctx = _capi.Context(0)
    L, hd = ctx._L, ctx._h
    info = np.zeros(8, np.int64)
    good = dict(off=[0, 1], node=[2], mask=[(1 << 25) | 1])

    def refused(word, planes=ALL29, ctype_mask=0x7F, flags=1, n_refs=1, entry=NEW, **kw):
        a = {k: np.array(kw.get(k, good[k]), d) for k, d in (('off', np.int64), ('node', np.int32), ('mask', np.uint32))}
        rc = getattr(L, entry)(hd, planes, ctype_mask, flags, n_refs, _p(a['off']), _p(a['node']), _p(a['mask']), _p(info))
        msg = L.arp_last_error(hd).decode()
        assert rc == _capi.ARP_E_ARG and word in msg and entry + ':' in msg, (word, rc, msg)
    refused('no library result', planes=0)
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    ctx.library_summary(off, x, h, *PARAMS)
    # in the order of the header: an earlier cause wins over a later one
    refused('no library-planes result', planes=1 << 29, flags=0)
    ctx.set_ligand_library_planes(lib)
    refused('no library-planes result', flags=0)
    fewer = list(ps[:-1]) + [None]                           # another T
    off2, x2, _ = ll.flatten_poses(lib, fewer)
    ctx.library_planes_summary(off2, x2)
    refused('differ in T', flags=0)
    ctx.library_planes_summary(off, x)
    table = ctx.library_contacts(off, x, h, *PARAMS)
    ptable = planes_resident(ctx)
    ptable['ligand_pose_off'] = off
    good_refs = lfp.references([(good['node'], good['mask'])], classes=True)
    want = ctx.library_fingerprints(good_refs, ALL29, bits=True)
    ctx.library_fingerprints_best()
    launches = ctx.library_fingerprints_info()['launches']
    refused('ARP_POSEFP_BY_RESIDUE', flags=0, ctype_mask=0)
    refused('ARP_POSEFP_BY_RESIDUE', planes=1 << 29, flags=0)
    refused('planes mask of 0', planes=0, ctype_mask=0)
    refused('beyond the 29 planes', planes=1 << 29, ctype_mask=0)
    refused('ctype_mask of 0', ctype_mask=0, flags=3)
    refused('unknown flag', flags=3, n_refs=65)
    refused('n_refs', n_refs=65)
    refused('strictly ascending', off=[0, 2], node=[3, 3], mask=[1 << 29, 1])
    refused('a reference mask has bits beyond the 29 planes', mask=[1 << 29])
    # the old entry stays as it was
    refused('beyond the 15 SIFt bits', planes=1 << 15, entry=OLD)
    refused('planes has bits beyond the 15 SIFt bits', planes=ALL29, flags=0, entry=OLD)
    refused('a reference mask has bits beyond the 15 SIFt bits', planes=ALL15, mask=[1 << 15], entry=OLD)
    ctx.run_enqueue(*PARAMS)
    refused('not been waited for', planes=0)
    ctx.run_wait()
    assert getattr(L, NEW)(None, ALL29, 0x7F, 1, 0, None, None, None, _p(info)) == _capi.ARP_E_ARG
    assert getattr(L, NEW)(hd, ALL29, 0x7F, 1, 0, None, None, None, None) == _capi.ARP_E_ARG
    assert not _fp_void(ctx) and not _best_void(ctx) and ctx.library_fingerprints_info()['launches'] == launches
    n = C.c_int64(0)
    count = np.empty(10, np.uint32)
    ctx._check(L.arp_library_fingerprints_fetch(hd, 0, None, _p(count), None, None, None, C.byref(n)), 'fetch')
    assert np.array_equal(count, want['count'])               # ... the resident result is the one it was
    # the same T, one float of the last pose differs by one step
    other = x.copy()
    other[-1] = np.nextafter(other[-1], np.float32(np.inf))
    ctx.library_planes_summary(off, other)
    refused('made from different poses')
    assert _fp_void(ctx) and _best_void(ctx)                  # no fingerprint is left ...
    assert ctx.library_info()['poses'] == 9 and ctx.library_planes_info()['poses'] == 9      # ... and both sources stay
    refused('made from different poses', planes=1 << 25)
    got = ctx.library_fingerprints(lfp.references([(good['node'], [1])]), ALL15, bits=True)  # the atom-atom part alone does not ask
    assert differences(got, yardstick(table, ptable, rec, [(good['node'], [1])], ALL15), KEYS) == []
    ctx.library_planes_summary(off, x)
    assert _same_bytes(ctx.library_fingerprints(good_refs, ALL29, bits=True), want)
    ctx.close()


@pytest.mark.gpu
def test_a_caller_owned_stream_and_run_library_fingerprints_chunked():
    from test_gpu_paths import _hip_runtime
    rec_cpu, ligs, ps = case('main')
    rec = receptor_gpu()
    ctx, lib = context(ligs)
    table, ptable = both(ctx, lib, ps)
    refs = pose_refs(table, ptable, rec, REF_POSES['main'])
    whole, want = check(ctx, table, ptable, rec, refs, ALL29)
    whole_best = ctx.library_fingerprints_best()
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    off, x, h = ll.flatten_poses(lib, ps)
    ctx.library_summary(off, x, h, *PARAMS)
    ctx.library_planes_summary(off, x)
    assert _same_bytes(ctx.library_fingerprints(lfp.references(refs, classes=True), ALL29, bits=True), whole)
    assert _same_bytes(ctx.library_fingerprints_best(), whole_best)
    ctx.use_stream(0)                                        # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0
    # end to end: every contact but bare proximity and all 14 classes
    ic = InteractionComplex(copy.copy(rec))
    one = ic.run_library_fingerprints(ligs, off, x, h, refs, classes='all')
    mask = fp.planes(None, 'all')
    want = yardstick(table, ptable, rec, refs, mask)
    keys = ('ids', 'count', 'cross', 'occupancy', 'reference_count', 'reference_cross')
    assert one['planes'] == mask and len(fp.plane_names(one['planes'])) == 28 and one['count'].shape == (16,) and one['cross'].shape == (16, 3)
    assert np.array_equal(one['count'], want['count'][3:]) and np.array_equal(one['cross'], want['cross'][3:]) and np.array_equal(one['ids'], want['ids'])
    assert np.array_equal(one['occupancy'], want['occupancy']) and np.array_equal(one['reference_count'], want['count'][:3])
    assert differences(one['best'], best_of(want, table['ligand_pose_off']), BEST) == []
    assert np.diff(table['ligand_pose_off'])[[0, 2, 4]].min() > 1 and table['ligand_pose_off'].tolist()[1:5] == [3, 4, 7, 9]
    part = ic.run_library_fingerprints(lib, off, x, h, lfp.references(refs, classes=True), classes='all', chunk=4)      # cuts the haem 4 | 5 6 and the arylamide
    assert differences(part, one, keys) == [] and differences(part['best'], one['best'], BEST) == []
    plain = ic.run_library_fingerprints(ligs, off, x, h, [(n, m & ALL15) for n, m in refs])
    assert (one['count'] >= plain['count']).all() and one['count'].sum() > plain['count'].sum()
    ic._ctx.close()
