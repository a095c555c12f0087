"""Library fingerprints (arp_library_fingerprints_launch / _fetch / _info, arp_library_fingerprints_best_launch / _fetch;
Context.library_fingerprints / library_fingerprints_best / library_fingerprints_info; InteractionComplex.run_library_fingerprints;
arpeggio_amd.library_fingerprints).

Two yardsticks, neither the code under test:

  (H) the host fold: ``fold`` below, Python sets over the records ``library_contacts`` returns (tests/test_ligand_library.py pins
      those records to the pose route and to the oracle); the q32 scores of ``best_of`` are Python integers
  (P) the pose route: ``poses_fingerprints`` on ``complex_of(receptor, ligand)`` with the ligand selected and its first poses as
      the references, against the library route with references made from those same poses' records

Every comparison is exact integers.  No tolerance anywhere, no time asserted."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, synth
from arpeggio_amd import library_fingerprints as lfp
from arpeggio_amd import ligand_library as ll
from arpeggio_amd import pose_fingerprints as fp
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex
from test_ligand_library import PARAMS, case_docked, case_main, launch, oracle_rows, pose_route_rows      # noqa: F401

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
ALL15 = (1 << 15) - 1
ONE = 1 << 32
KEYS = ('ids', 'count', 'cross', 'occupancy')
BEST = ('n_poses', 'best_pose', 'tanimoto_q32', 'shared', 'count')
ENTRIES = ('arp_library_fingerprints_launch', 'arp_library_fingerprints_fetch', 'arp_library_fingerprints_info',
           'arp_library_fingerprints_best_launch', 'arp_library_fingerprints_best_fetch')


# ------------------------------------------------------------------------------------------------------------- yardstick (H)
def pose_features(table, t, res_id, planes, ctype_mask, level):
    """The set of (node, plane) of global pose ``t``: the receptor side of every participating record."""
    off = np.asarray(table['pose_off']).astype(np.int64)
    out = set()
    for i, s, c in zip(table['i'][off[t]:off[t + 1]].tolist(), table['sift'][off[t]:off[t + 1]].tolist(), table['ctype'][off[t]:off[t + 1]].tolist()):
        if not (ctype_mask >> c) & 1:
            continue
        node = int(res_id[i]) if level == 'residue' else i
        out |= {(node, b) for b in range(15) if (s & planes) >> b & 1}
    return out


def ref_features(nodes, masks, planes):
    return {(int(n), b) for n, m in zip(nodes, masks) for b in range(15) if (int(m) & planes) >> b & 1}


def fold(table, refs, res_id, planes, ctype_mask=0x7F, level='residue'):
    """(H): the result a launch must give, from the records of a library result and the references as (nodes, masks) pairs."""
    T = len(table['pose_off']) - 1
    rows = [ref_features(n, m, planes) for n, m in refs] + [pose_features(table, t, res_id, planes, ctype_mask, level) for t in range(T)]
    Q = len(refs)
    sel = [b for b in range(15) if planes >> b & 1]
    ids = sorted({n for r in rows for n, _ in r})
    occ = [[sum((u, b) in r for r in rows[Q:]) for b in sel] for u in ids]
    return dict(ids=np.array(ids, np.int32), count=np.array([len(r) for r in rows], np.uint32),
                cross=np.array([[len(r & rows[q]) for q in range(Q)] for r in rows], np.uint32).reshape(len(rows), Q),
                occupancy=np.array(occ, np.uint32).reshape(len(ids), len(sel)),
                on=np.array([[[(u, b) in r for b in sel] for u in ids] for r in rows], bool).reshape(len(rows), len(ids), len(sel)))


def best_of(want, lig_off):
    """The test's own mirror of the best-pose table, from (H)'s count and cross with Python integers."""
    Q = want['cross'].shape[1]
    count, cross = want['count'].tolist(), want['cross'].tolist()
    L = len(lig_off) - 1
    out = dict(n_poses=np.diff(np.asarray(lig_off, np.int64)), best_pose=np.full((L, Q), -1, np.int32), tanimoto_q32=np.full((L, Q), -1, np.int64),
               shared=np.zeros((L, Q), np.uint32), count=np.zeros((L, Q), np.uint32))
    for l in range(L):
        for q in range(Q):
            for t in range(int(lig_off[l]), int(lig_off[l + 1])):
                x, n = cross[Q + t][q], count[Q + t]
                u = n + count[q] - x
                s = ONE if u == 0 else (x << 32) // u
                if out['best_pose'][l, q] < 0 or s > out['tanimoto_q32'][l, q]:      # (ascending t: the lower pose keeps a tie)
                    out['best_pose'][l, q], out['tanimoto_q32'][l, q], out['shared'][l, q], out['count'][l, q] = t, s, x, n
    return out


def differences(got, want, keys=KEYS):
    return [k for k in keys if np.asarray(got[k]).dtype != np.asarray(want[k]).dtype or np.asarray(got[k]).shape != np.asarray(want[k]).shape or
            not np.array_equal(got[k], want[k])]


def check(ctx, table, refs, res_id, planes, ctype_mask=0x7F, level='residue'):
    """A launch against (H): the four arrays, the bit matrix, and the best table where there is a reference."""
    got = ctx.library_fingerprints(lfp.references(refs), planes, ctype_mask, by_residue=level == 'residue', bits=True)
    want = fold(table, refs, res_id, planes, ctype_mask, level)
    assert differences(got, want) == [], (level, hex(planes), hex(ctype_mask))
    assert got['bits'].shape == (len(want['count']), bin(planes).count('1'), (len(want['ids']) + 63) // 64)
    assert np.array_equal(fp.unpack(got), want['on'])
    assert got['n_refs'] == len(refs) and got['level'] == level and got['planes'] == planes
    if refs:
        assert differences(ctx.library_fingerprints_best(), best_of(want, table['ligand_pose_off']), BEST) == []
    return got, want


def _ctx(pc):
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    return ctx


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def main_launch():
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    return rec, ligs, poses, lib, ctx, launch(ctx, lib, poses)


def water_alone(n):
    """The first ``n`` poses of the water of the main case, the other ligands empty in pose_off."""
    _, ligs, poses = case_main()
    return [(poses[0][0][:n], poses[0][1][:n])] + [None] * (len(ligs) - 1)


def _fp_void(ctx):
    n = C.c_int64(0)
    return ctx._L.arp_library_fingerprints_fetch(ctx._h, 0, None, None, None, None, None, C.byref(n)) == _capi.ARP_E_ARG


def _best_void(ctx):
    n, q = C.c_int64(0), C.c_int64(0)
    return ctx._L.arp_library_fingerprints_best_fetch(ctx._h, 0, None, None, None, None, None, C.byref(n), C.byref(q)) == _capi.ARP_E_ARG


def _same_bytes(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same_bytes(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------- CPU
def test_the_entries_are_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    for s in ENTRIES:
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    assert '#define ARP_LIBFP_MAX_FEATURES (1 << 22)' in hdr and _capi.LIBFP_MAX_FEATURES == lfp.MAX_FEATURES == 1 << 22
    assert all(hasattr(_capi.Context, m) for m in ('library_fingerprints', 'library_fingerprints_best', 'library_fingerprints_info'))
    assert lfp.tanimoto is fp.tanimoto and lfp.recovery is fp.recovery and lfp.rank is fp.rank and lfp.merge is fp.merge
    assert lfp.strip_references is fp.strip_references and lfp.unpack is fp.unpack


def test_every_refusal_of_references_and_validate_by_name():
    good = lfp.references([([3, 5, 9], [1, 2, 4]), {}, {7: 3, 2: 0x7FFF}])
    assert good['ref_off'].tolist() == [0, 3, 3, 5] and good['ref_node'].tolist() == [3, 5, 9, 2, 7] and good['ref_planes'].tolist() == [1, 2, 4, 0x7FFF, 3]
    assert good['ref_off'].dtype == np.int64 and good['ref_node'].dtype == np.int32 and good['ref_planes'].dtype == np.uint32
    assert lfp.n_references(good) == 3 and lfp.validate(good, 10) is good and lfp.n_references(lfp.references([])) == 0

    def broken(**kw):
        r = {k: np.array(v, np.int64) for k, v in good.items()}
        r.update({k: np.array(v, np.int64) for k, v in kw.items()})
        return r
    for cause, r, n in (('MAX_REFS', broken(ref_off=np.zeros(66)), None), ('ref_off must start at 0', broken(ref_off=[1, 3, 3, 5]), None),
                        ('ref_off must not decrease', broken(ref_off=[0, 3, 2, 5]), None),
                        ('MAX_FEATURES', broken(ref_off=[0, 3, 3, (1 << 22) + 1]), None),
                        ('ref_off\\[-1\\] entries', broken(ref_node=[3, 5, 9, 2]), None), ('ref_off\\[-1\\] entries', broken(ref_planes=[1, 2]), None),
                        ('outside', broken(ref_node=[-1, 5, 9, 2, 7]), None), ('outside', good, 9),
                        ('strictly ascending', broken(ref_node=[3, 3, 9, 2, 7]), None), ('strictly ascending', broken(ref_node=[3, 5, 9, 7, 2]), None),
                        ('beyond the 15 SIFt bits', broken(ref_planes=[1, 2, 4, 1 << 15, 3]), None)):
        with pytest.raises(ValueError, match=cause):
            lfp.validate(r, n)
    # an earlier cause wins over a later one
    with pytest.raises(ValueError, match='ref_off must not decrease'):
        lfp.validate(broken(ref_off=[0, 3, 2, 5], ref_node=[-1, 5, 9, 2, 7]))
    with pytest.raises(ValueError, match='outside'):
        lfp.validate(broken(ref_node=[-1, -1, 9, 2, 7], ref_planes=[1 << 15] * 5))
    assert lfp.validate(broken(ref_node=[3, 5, 9, 3, 5]))                       # ascending WITHIN a reference: 9 -> 3 is a seam
    with pytest.raises(ValueError, match='MAX_REFS'):
        lfp.references([{}] * 65)
    with pytest.raises(ValueError, match='one mask per node'):
        lfp.references([([1, 2], [1])])
    with pytest.raises(ValueError, match='outside'):
        lfp.references([{12: 1}], n_nodes=12)


def test_reference_from_records_on_a_hand_made_table():
    res_id = np.array([0, 0, 1, 1, 2, 3], np.int32)
    i = [0, 1, 1, 2, 4, 5, 5]
    sift = [BIT['hbond'], BIT['vdw'], BIT['hbond'] | BIT['proximal'], BIT['proximal'], BIT['ionic'], BIT['vdw'], BIT['polar']]
    ctype = [CT['INTER'], CT['INTER'], CT['INTER'], CT['INTER'], CT['INTER'], CT['NON_SELECTION_WATER'], CT['INTER']]
    n, m = lfp.reference_from_records(i, sift, ctype, res_id)
    assert n.tolist() == [0, 1, 2, 3] and m.tolist() == [BIT['hbond'] | BIT['vdw'] | BIT['proximal'], BIT['proximal'], BIT['ionic'], BIT['vdw'] | BIT['polar']]
    assert n.dtype == np.int32 and m.dtype == np.uint32
    n, m = lfp.reference_from_records(i, sift, ctype, level='atom')
    assert n.tolist() == [0, 1, 2, 4, 5] and m[1] == BIT['vdw'] | BIT['hbond'] | BIT['proximal']
    # the selection empties residue 1 (bare proximity) and the water record's residue 3 keeps only its INTER record
    n, m = lfp.reference_from_records(i, sift, ctype, res_id, planes=ALL15 & ~BIT['proximal'], ctype_mask=1 << CT['INTER'])
    assert n.tolist() == [0, 2, 3] and m.tolist() == [BIT['hbond'] | BIT['vdw'], BIT['ionic'], BIT['polar']]
    table = dict(i=np.array(i, np.int32), sift=np.array(sift, np.uint16), ctype=np.array(ctype, np.uint8), pose_off=np.array([0, 3, 3, 7], np.uint64))
    assert lfp.reference_from_pose(table, 0, res_id)[0].tolist() == [0] and lfp.reference_from_pose(table, 1, res_id)[0].tolist() == []
    assert lfp.reference_from_pose(table, 2, level='atom')[0].tolist() == [2, 4, 5]
    with pytest.raises(ValueError):
        lfp.reference_from_pose(table, 3, res_id)
    with pytest.raises(ValueError):
        lfp.reference_from_records(i, sift, ctype)                               # residue level without res_id


def hand_result():
    """Q = 2, three ligands with 3, 0 and 2 poses.  Reference counts 4 and 0.  Scores against reference 0: poses 0 and 1 tie at
    2 / (2 + 4 - 2) = 1 / 2, pose 2 is 3 / (5 + 4 - 3) = 1 / 2 as well; poses 3, 4: 4 / 4 = 1 and 1 / 7.  Against the empty
    reference 1 every pose here has features and scores 0."""
    count = np.array([4, 0, 2, 2, 5, 4, 4], np.uint32)
    cross = np.array([[4, 0], [0, 0], [2, 0], [2, 0], [3, 0], [4, 0], [1, 0]], np.uint32)
    return dict(ids=np.arange(6, dtype=np.int32), count=count, cross=cross, occupancy=np.zeros((6, 1), np.uint32), planes=1, n_refs=2, level='residue')


def test_best_and_merge_best_on_a_hand_made_table():
    r = hand_result()
    lo = [0, 3, 3, 5]
    b = lfp.best(r, lo)
    assert b['n_poses'].tolist() == [3, 0, 2] and b['best_pose'].tolist() == [[0, 0], [-1, -1], [3, 3]]      # ties: the lower pose
    assert b['tanimoto_q32'].tolist() == [[ONE // 2, 0], [-1, -1], [ONE, 0]] and b['shared'].tolist() == [[2, 0], [0, 0], [4, 0]]
    assert b['count'].tolist() == [[2, 2], [0, 0], [4, 4]]
    assert all(b[k].dtype == lfp.BEST_DTYPES[k] for k in lfp.BEST_KEYS) and b['n_poses'].dtype == np.int64
    assert differences(b, best_of(r, lo), BEST) == [] and differences(lfp.best(lfp.strip_references(r), lo), b, BEST) == []
    # a pose without features against the empty reference: 0 / 0 is 2^32
    r2 = copy.deepcopy(r)
    r2['count'][4], r2['cross'][4] = 0, 0
    assert lfp.best(r2, lo)['tanimoto_q32'][0].tolist() == [ONE // 2, ONE] and lfp.best(r2, lo)['best_pose'][0].tolist() == [0, 2]
    with pytest.raises(ValueError):
        lfp.best(r, [0, 3, 3, 4])
    with pytest.raises(ValueError, match='no reference'):
        lfp.best(dict(r, n_refs=0, cross=np.zeros((7, 0), np.uint32)), [0, 3, 3, 7])
    # chunks of 2, 2 and 1 global poses: ligand 0 is cut between the first two (its tie crosses the cut), ligand 2 between the last two

    def chunk(a, b_, off):
        sub = dict(r, count=np.concatenate([r['count'][:2], r['count'][2 + a:2 + b_]]), cross=np.concatenate([r['cross'][:2], r['cross'][2 + a:2 + b_]]))
        return lfp.best(sub, off), a
    parts = [chunk(0, 2, [0, 2, 2, 2]), chunk(2, 4, [0, 1, 1, 2]), chunk(4, 5, [0, 0, 0, 1])]
    assert parts[1][0]['best_pose'].tolist() == [[0, 0], [-1, -1], [1, 1]]                                    # (within the chunk)
    assert differences(lfp.merge_best(parts), b, BEST) == []
    assert differences(lfp.merge_best(parts[::-1]), b, BEST) == []             # the lower pose wins whatever the order of arrival
    assert differences(lfp.merge_best([(b, 0)]), b, BEST) == []
    with pytest.raises(ValueError):
        lfp.merge_best([])
    with pytest.raises(ValueError):
        lfp.merge_best([(b, 0), (lfp.best(r, [0, 5]), 0)])


def test_to_records_and_the_csv_text(tmp_path):
    r = hand_result()
    lo = [0, 3, 3, 5]
    b = lfp.best(r, lo)
    recs = lfp.to_records(b, r['count'][:2], lo)
    assert len(recs) == 6 and [(x['ligand'], x['reference']) for x in recs] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert recs[0] == dict(ligand=0, reference=0, type='library-fingerprint', n_poses=3, best_pose=0, tanimoto_q32=ONE // 2, tanimoto=0.5, shared=2,
                           count=2, recovery=0.5, pose=0)
    assert recs[2]['best_pose'] == -1 and recs[2]['tanimoto'] is None and recs[2]['recovery'] is None and recs[2]['pose'] == -1
    assert recs[4]['pose'] == 0 and recs[4]['best_pose'] == 3 and recs[4]['tanimoto'] == 1.0 and recs[5]['recovery'] == 1.0      # an empty reference
    ic = InteractionComplex(synth.proteinlike(n_res=8, seed=2))
    ic.library_fingerprints = dict(lfp.strip_references(r), best=b, ligand_pose_off=np.array(lo))
    path = ic.write_library_fingerprints(str(tmp_path))
    lines = open(path).read().splitlines()
    assert path.endswith('proteinlike.libraryfp') and lines[0] == ','.join(lfp.CSV_HEADER + ['pose']) and len(lines) == 7
    assert lines[1] == f'0,0,3,0,{ONE // 2},0.5,2,2,0.5,0' and lines[3] == '1,0,0,-1,-1,,0,0,,-1' and lines[5] == f'2,0,2,3,{ONE},1.0,4,4,1.0,0'
    with pytest.raises(AttributeError):
        InteractionComplex(synth.proteinlike(n_res=8, seed=2)).write_library_fingerprints(str(tmp_path))


def test_the_oracle_alone_meets_the_coverage_conditions():
    """Of the oracle's rows on the main case, all 15 planes and all contact types: more than 128 receptor atoms take part (three
    words a plane or more at atom level, W > 32: more than one word slice of k_pfp_cross, its atomic path) and at most 64
    residues (exactly one word a plane at residue level)."""
    rec, ligs, poses = case_main()
    rows = [r for lig in oracle_rows(rec, ligs, poses, PARAMS[0]) for r in lig]
    atoms = np.unique(np.concatenate([r['i'][(r['sift'] & ALL15) != 0] for r in rows]))
    assert len(atoms) > 128 and len(np.unique(rec.res_id[atoms])) <= 64


# ------------------------------------------------------------------------------------------------------------- GPU: parity
def main_refs(table, res_id, level):
    """Three references from poses of three different ligands: the water's first pose, the haem's, the halide's."""
    lo = table['ligand_pose_off']
    return [lfp.reference_from_pose(table, int(lo[l]), res_id, level=level) for l in (0, 2, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize('level', fp.LEVELS)
def test_main_case_equals_the_host_fold(level):
    rec, ligs, poses, lib, ctx, t = main_launch()
    assert t['ligand_pose_off'].tolist() == [0, 70, 71, 74, 74, 79, 81, 82]
    # the ligand side is a valid receptor id of another residue in many records: a node taken from it would show
    assert (rec.res_id[t['a']] != rec.res_id[t['i']]).any() and int(t['a'].max()) < rec.n_atoms
    refs = main_refs(t, rec.res_id, level)
    assert all(len(n) > 0 for n, _ in refs)
    got, want = check(ctx, t, refs, rec.res_id, ALL15, 0x7F, level)
    assert got['count'].shape == (85,) and got['cross'].shape == (85, 3) and (got['count'][3:] > 0).any()
    # a reference that is a pose of the launch equals that pose's row
    lo = t['ligand_pose_off']
    for q, l in enumerate((0, 2, 4)):
        assert got['count'][q] == got['count'][3 + lo[l]] == got['cross'][3 + lo[l], q] and np.array_equal(got['cross'][q], got['cross'][3 + lo[l]])
    info = ctx.library_fingerprints_info()
    assert info['rows'] == 85 and info['n_refs'] == 3 and info['nodes'] == len(want['ids']) and info['planes'] == 15
    if level == 'atom':      # more than one word slice of k_pfp_cross (its atomic path); one at residue level
        assert info['nodes'] > 128 and info['words'] > 32 and info['slices'] > 1
    else:
        assert info['nodes'] <= 64 and info['words'] == 15 and info['slices'] == 1
    # named contacts and a subset of the entity kinds; the references keep their masks of before the selection
    sub = (1 << CT['INTER']) | (1 << CT['NON_SELECTION_WATER'])
    got2, _ = check(ctx, t, refs, rec.res_id, fp.planes(None), 1 << CT['INTER'], level)
    check(ctx, t, refs, rec.res_id, BIT['hbond'] | BIT['hydrophobic'], sub, level)
    assert got2['count'].sum() < got['count'].sum() and ctx.library_fingerprints_info()['launches'] == 3
    # the host functions of the pose fingerprints apply unchanged
    tan = lfp.tanimoto(got)
    assert tan.shape == (85, 3) and tan[0, 0] == 1.0 and tan[3 + lo[2], 1] == 1.0 and lfp.rank(got, 1)[0] in (1, 3 + lo[2])
    s = lfp.strip_references(got)
    assert s['count'].shape == (82,) and np.array_equal(s['reference_count'], got['count'][:3])
    ctx.close()


@pytest.mark.gpu
def test_one_ligand_equals_the_pose_route():
    rec, ligs, poses = case_main()
    l = 4                                                   # the halide: five poses, hydrogen rows
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    alone = [None] * len(ligs)
    alone[l] = poses[l]
    t = launch(ctx, lib, alone)
    refs = [lfp.reference_from_pose(t, q, rec.res_id) for q in range(2)]
    got = ctx.library_fingerprints(lfp.references(refs), ALL15)
    other = _capi.Context(0)
    both = ll.complex_of(rec, ligs[l])
    other.set_complex(both)
    m = np.zeros(both.n_atoms, np.uint8)
    m[rec.n_atoms:] = 1
    other.set_selection(m)
    other.poses_summary(poses[l][0], poses[l][1], *PARAMS[0])
    want = other.poses_fingerprints(ALL15, n_refs=2)
    other.close()
    assert np.array_equal(got['ids'], want['ids']) and len(want['ids']) > 3
    assert np.array_equal(got['count'][2:], want['count']) and np.array_equal(got['cross'][2:], want['cross'])
    assert np.array_equal(got['count'][:2], want['count'][:2]) and np.array_equal(got['cross'][:2], want['cross'][:2])
    # (occupancy: the pose route leaves its two reference poses out, the library route counts all five poses)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('T,Q', [(63, 1), (64, 1), (64, 0), (64, 64)], ids=['64-rows', '65-rows', 'no-reference', '64-references'])
def test_row_seams_of_the_64_row_tile(T, Q):
    rec, ligs, _ = case_main()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    t = launch(ctx, lib, water_alone(T))
    assert len(t['pose_off']) == T + 1 and len(t['i']) > 0
    refs = [lfp.reference_from_pose(t, q, level='atom') for q in range(Q)]      # each reference from one water pose
    got, _ = check(ctx, t, refs, rec.res_id, ALL15, 0x7F, 'atom')
    assert got['cross'].shape == (Q + T, Q) and ctx.library_fingerprints_info()['rows'] == Q + T
    check(ctx, t, [lfp.reference_from_pose(t, q, rec.res_id) for q in range(Q)], rec.res_id, ALL15, 0x7F, 'residue')
    if Q == 0:
        with pytest.raises(ValueError, match='no reference'):
            ctx.library_fingerprints_best()
        assert _best_void(ctx)
    ctx.close()


@pytest.mark.gpu
def test_edges_untouched_node_dropped_plane_empty_reference_and_a_tie():
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    hem, water = ligs[2], ligs[0]
    x0 = hem.xyz.astype(np.float32)
    far = np.array([100.0, 0.0, 0.0], np.float32)
    wx, wh = poses[0][0][:1] + far, poses[0][1][:1] + far.astype(np.float64)
    alone = [(wx, wh), None, (np.stack([x0 + far, x0, x0]), None)] + [None] * 4      # the water far away; the haem far away, at home twice
    t = launch(ctx, lib, alone)
    off = t['pose_off'].astype(np.int64)
    assert off[2] == 0 and off[3] - off[2] == off[4] - off[3] > 100                   # poses 0, 1: no record; poses 2, 3: identical
    planes = ALL15 & ~BIT['proximal']
    home = lfp.reference_from_pose(t, 2, rec.res_id)
    touched = set(fold(t, [], rec.res_id, planes)['ids'].tolist())
    untouched = next(r for r in range(rec.n_residues) if r not in touched and r not in set(home[0].tolist()))
    only_proximal = next(r for r in range(rec.n_residues) if r not in touched and r != untouched)
    more = dict(zip(home[0].tolist(), home[1].tolist()))
    more[untouched] = BIT['hbond'] | BIT['vdw']
    more[only_proximal] = BIT['proximal']                                              # its only plane is not selected
    plus = (np.array(sorted(more), np.int32), np.array([more[k] for k in sorted(more)], np.uint32))
    refs = [home, plus, (np.zeros(0, np.int32), np.zeros(0, np.uint32))]
    got, want = check(ctx, t, refs, rec.res_id, planes)
    ids = got['ids'].tolist()
    # the node no pose touches: a column with occupancy 0 that counts in the reference and lowers the Tanimoto
    u = ids.index(untouched)
    assert not got['occupancy'][u].any() and got['count'][1] == got['count'][0] + 2 and got['cross'][1, 0] == got['count'][0]
    tan = lfp.tanimoto(got)
    assert tan[3 + 2, 0] == 1.0 and tan[3 + 2, 1] == got['count'][0] / (got['count'][0] + 2) < 1.0
    # the feature whose plane is not selected: dropped, and its node is no column
    assert only_proximal not in ids and len(ids) == len(touched) + 1
    # the empty reference against the poses 100 A away: both without features
    assert got['count'][2] == 0 and got['count'][3] == got['count'][4] == 0
    b = ctx.library_fingerprints_best()
    assert b['n_poses'].tolist() == [1, 0, 3, 0, 0, 0, 0]
    assert b['tanimoto_q32'][0].tolist() == [0, 0, ONE] and b['best_pose'][0].tolist() == [0, 0, 0] and tan[3, 2] == 1.0
    assert b['best_pose'][2].tolist() == [2, 2, 1] and b['tanimoto_q32'][2].tolist()[0] == ONE and b['tanimoto_q32'][2, 2] == ONE
    # ... two identical poses: the lower id; shared and count are that pose's
    assert want['cross'][3 + 2, 0] == want['cross'][3 + 3, 0] and b['shared'][2, 0] == b['count'][2, 0] == got['count'][0]
    assert b['best_pose'][1].tolist() == [-1] * 3 and b['tanimoto_q32'][1].tolist() == [-1] * 3 and not b['shared'][1].any() and not b['count'][1].any()
    ctx.close()


@pytest.mark.gpu
def test_best_pose_per_ligand_equals_the_mirror():
    rec, ligs, poses, lib, ctx, t = main_launch()
    for level in fp.LEVELS:
        refs = main_refs(t, rec.res_id, level) + [(np.zeros(0, np.int32), np.zeros(0, np.uint32))]
        got = ctx.library_fingerprints(lfp.references(refs), fp.planes(None), by_residue=level == 'residue')
        b = ctx.library_fingerprints_best()
        want = best_of(fold(t, refs, rec.res_id, fp.planes(None), 0x7F, level), t['ligand_pose_off'])
        assert differences(b, want, BEST) == [] and differences(b, lfp.best(got, t['ligand_pose_off']), BEST) == [], level
        assert b['best_pose'].shape == (7, 4) and b['n_poses'].tolist() == [70, 1, 3, 0, 5, 2, 1]
        assert (b['best_pose'][3] == -1).all() and (b['tanimoto_q32'][3] == -1).all() and not b['shared'][3].any() and not b['count'][3].any()
        # a reference made from a ligand's pose is recovered by that pose
        assert b['best_pose'][0, 0] == 0 and b['tanimoto_q32'][0, 0] == ONE and b['best_pose'][2, 1] == 71 and b['best_pose'][4, 2] == 74
        lo = t['ligand_pose_off']
        has = np.diff(lo) > 0
        assert ((b['best_pose'][has] >= lo[:-1][has][:, None]) & (b['best_pose'][has] < lo[1:][has][:, None])).all()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
@pytest.mark.gpu
def test_what_voids_the_fingerprint_and_its_best_table():
    rec, ligs, poses, lib, ctx, t = main_launch()
    refs = lfp.references(main_refs(t, rec.res_id, 'residue'))
    assert _fp_void(ctx) and _best_void(ctx) and ctx.library_fingerprints_info()['rows'] == 0

    def make():
        ctx.library_fingerprints(refs, ALL15)
        ctx.library_fingerprints_best()
        assert not _fp_void(ctx) and not _best_void(ctx)
    make()
    launch(ctx, lib, poses)                                  # a new library launch: both
    assert _fp_void(ctx) and _best_void(ctx) and ctx.library_fingerprints_info()['rows'] == 0
    make()
    ctx.set_ligand_library(lib)                              # a new library: both (and the library result)
    assert _fp_void(ctx) and _best_void(ctx)
    with pytest.raises(ValueError, match='no library result'):
        ctx.library_fingerprints(refs, ALL15)
    launch(ctx, lib, poses)
    make()
    ctx.set_complex(rec)                                     # a new structure: both
    assert _fp_void(ctx) and _best_void(ctx)
    launch(ctx, lib, poses)
    make()
    m = np.zeros(rec.n_atoms, np.uint8)
    m[:20] = 1
    ctx.set_selection(m)                                     # reads no selection: neither
    assert not _fp_void(ctx) and not _best_void(ctx)
    before = ctx.library_fingerprints_info()['launches']
    ctx.library_fingerprints(refs, ALL15)                    # a new fingerprint launch, same arguments: launched again, the best table goes
    assert not _fp_void(ctx) and _best_void(ctx) and ctx.library_fingerprints_info()['launches'] == before + 1
    with pytest.raises(ValueError, match='planes mask of 0'):      # a refusal touches neither
        ctx.library_fingerprints(refs, 0)
    ctx.library_fingerprints_best()
    with pytest.raises(ValueError, match='planes mask of 0'):
        ctx.library_fingerprints(refs, 0)
    assert not _fp_void(ctx) and not _best_void(ctx)
    ctx.close()


@pytest.mark.gpu
def test_the_other_results_stay_byte_identical():
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    hem = np.nonzero(rec.res_id == int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]))[0]
    m = np.zeros(rec.n_atoms, np.uint8)
    m[hem] = 1
    ctx.set_selection(m)
    px, ph = synth.poses_of(rec, hem, 6, seed=11, shift=2.0)
    ctx.poses_contacts(px, ph, 5.0, 0.1, False)
    ctx.set_ligand_library(lib)
    t = launch(ctx, lib, poses)
    w = np.arange(16, dtype=np.int64) - 4

    def everything():
        got = ctx._pose_records_fetch('arp_library_contacts_fetch', 'a', 82, len(t['i']))
        n = C.c_int64(0)
        best = dict(n_poses=np.empty(7, np.int64), best_pose=np.empty(7, np.int32), score=np.empty(7, np.int64))
        ctx._check(ctx._L.arp_library_best_fetch(ctx._h, 7, _p(best['n_poses']), _p(best['best_pose']), _p(best['score']), C.byref(n)), 'best')
        return got, best, ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    ctx.library_best(w)
    ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    launches = ctx.poses_fingerprints_info()['launches']
    before = everything()
    refs = lfp.references(main_refs(t, rec.res_id, 'atom'))
    ctx.library_fingerprints(refs, ALL15, by_residue=False, bits=True)            # made and fetched
    ctx.library_fingerprints_best()
    assert all(_same_bytes(a, b) for a, b in zip(everything(), before))
    ctx.library_fingerprints(refs, fp.planes(None), by_residue=False)             # replaced: the best table is void
    assert _best_void(ctx) and all(_same_bytes(a, b) for a, b in zip(everything(), before))
    assert ctx.poses_fingerprints_info()['launches'] == launches and ctx.library_info()['best']
    ctx.close()


@pytest.mark.gpu
def test_every_host_refusal_names_its_cause_in_order():
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)
    L, hd = ctx._L, ctx._h
    info = np.zeros(8, np.int64)
    N, NR = rec.n_atoms, rec.n_residues
    good = dict(off=[0, 2, 3], node=[3, 5, 4], mask=[1, 2, 4])

    def refused(word, planes=ALL15, ctype_mask=0x7F, flags=1, n_refs=2, code=_capi.ARP_E_ARG, hd=hd, **kw):
        a = {k: (None if kw.get(k, good[k]) is None else np.array(kw.get(k, good[k]), d)) for k, d in (('off', np.int64), ('node', np.int32), ('mask', np.uint32))}
        rc = L.arp_library_fingerprints_launch(hd, planes, ctype_mask, flags, n_refs, _p(a['off']), _p(a['node']), _p(a['mask']), _p(info))
        msg = L.arp_last_error(hd).decode()
        assert rc == code and word in msg, (word, rc, msg)
    refused('no library result', planes=0)
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    refused('no library result', planes=0)
    t = launch(ctx, lib, poses)
    # in the order of the header: an earlier cause wins over a later one
    refused('planes mask of 0', planes=0, ctype_mask=0)
    refused('beyond the 15 SIFt bits', planes=1 << 15, ctype_mask=0)
    refused('ctype_mask of 0', ctype_mask=0, flags=2)
    refused('beyond the 7 contact types', ctype_mask=0x80, flags=2)
    refused('unknown flag', flags=2, n_refs=65)               # (ARP_POSEFP_ALL_PAIRS: there is no all-pairs matrix)
    refused('unknown flag', flags=5, n_refs=65)
    refused('n_refs', n_refs=65, off=None)
    refused('n_refs', n_refs=-1, off=None)
    refused('a reference array is missing', off=None)
    refused('a reference array is missing', node=None, off=[1, 2, 3])
    refused('a reference array is missing', mask=None, off=[1, 2, 3])
    refused('ref_off must start at 0', off=[1, 2, 3], node=[-1, 5, 4])
    refused('ref_off must not decrease', off=[0, 2, 1], node=[-1, 5, 4])
    refused('ARP_LIBFP_MAX_FEATURES', off=[0, 2, (1 << 22) + 1], node=[-1, 5, 4])
    refused('outside', node=[-1, 5, 4], mask=[1 << 15, 2, 4])
    refused('outside', node=[3, NR, 4])                       # residues: [0, n_residues)
    refused('outside', flags=0, node=[3, N, 4])               # atoms: [0, n)
    refused('strictly ascending', node=[5, 5, 4], mask=[1 << 15, 2, 4])
    refused('strictly ascending', node=[5, 3, 4])
    refused('beyond the 15 SIFt bits', mask=[1, 1 << 15, 4])
    assert _fp_void(ctx) and ctx.library_fingerprints_info()['launches'] == 0
    m = np.zeros(rec.n_atoms, np.uint8)
    m[:20] = 1
    ctx.set_selection(m)
    ctx.run_enqueue(5.0, 0.1, False)
    refused('not been waited for', planes=0)
    assert L.arp_library_fingerprints_best_launch(hd) == _capi.ARP_E_ARG and 'not been waited for' in L.arp_last_error(hd).decode()
    ctx.run_wait()
    assert L.arp_library_fingerprints_best_launch(hd) == _capi.ARP_E_ARG and 'no library fingerprint' in L.arp_last_error(hd).decode()
    # what is accepted: nodes that descend across the seam of two references, Q = 0 with NULL arrays, atom ids at atom level
    a = {k: np.array(v, d) for (k, v), d in zip(good.items(), (np.int64, np.int32, np.uint32))}
    assert L.arp_library_fingerprints_launch(hd, ALL15, 0x7F, 1, 2, _p(a['off']), _p(a['node']), _p(a['mask']), _p(info)) == _capi.ARP_OK and info[0] == 84
    assert L.arp_library_fingerprints_launch(hd, ALL15, 0x7F, 0, 0, None, None, None, _p(info)) == _capi.ARP_OK and info[1] == 0 and info[6] == 2
    assert L.arp_library_fingerprints_best_launch(hd) == _capi.ARP_E_ARG and 'no reference' in L.arp_last_error(hd).decode()
    assert L.arp_library_fingerprints_launch(None, ALL15, 0x7F, 0, 0, None, None, None, _p(info)) == _capi.ARP_E_ARG
    assert L.arp_library_fingerprints_launch(hd, ALL15, 0x7F, 0, 0, None, None, None, None) == _capi.ARP_E_ARG
    # the fetches: the needed size, nothing written when it does not fit, any pointer may be NULL
    want = ctx.library_fingerprints(lfp.references(main_refs(t, rec.res_id, 'atom')), ALL15, by_residue=False, bits=True)
    U, n, q = len(want['ids']), C.c_int64(0), C.c_int64(0)
    ids = np.full(U, -7, np.int32)
    assert L.arp_library_fingerprints_fetch(hd, U - 1, _p(ids), None, None, None, None, C.byref(n)) == _capi.ARP_E_CAPACITY and n.value == U and (ids == -7).all()
    assert L.arp_library_fingerprints_fetch(hd, U, _p(ids), None, None, None, None, C.byref(n)) == _capi.ARP_OK and np.array_equal(ids, want['ids'])
    count = np.zeros(85, np.uint32)
    assert L.arp_library_fingerprints_fetch(hd, 0, None, _p(count), None, None, None, C.byref(n)) == _capi.ARP_OK and np.array_equal(count, want['count'])
    assert L.arp_library_fingerprints_fetch(hd, 0, None, None, None, None, None, None) == _capi.ARP_E_ARG
    b = ctx.library_fingerprints_best()
    pose = np.full((7, 3), -7, np.int32)
    assert L.arp_library_fingerprints_best_fetch(hd, 6, None, _p(pose), None, None, None, C.byref(n), C.byref(q)) == _capi.ARP_E_CAPACITY
    assert n.value == 7 and q.value == 3 and (pose == -7).all()
    assert L.arp_library_fingerprints_best_fetch(hd, 7, None, _p(pose), None, None, None, C.byref(n), C.byref(q)) == _capi.ARP_OK and np.array_equal(pose, b['best_pose'])
    ctx.close()
    # by residue without residues resident: the atoms with their bonds, hydrogens and neighbours, no arp_set_residues (and no rings
    # or amides, which a library launch does not read either); a library launch reads no residue table, so a result is resident.  The cause comes before the Q check, and the atom level is accepted
    bare = _capi.Context(0)
    bh = bare._h
    for entry, args in (('arp_set_atoms', (rec.n_atoms, _p(rec.xyz), _p(rec.vdw), _p(rec.cov), _p(rec.type_mask), _p(rec.flags), _p(rec.res_id))),
                        ('arp_set_bonds', (_p(rec.bond_off), _p(rec.bond_idx))), ('arp_set_hydrogens', (_p(rec.h_off), _p(rec.h_xyz))),
                        ('arp_set_single_bond_neighbours', (_p(rec.sb_nbr),))):
        bare._check(getattr(L, entry)(bh, *args), entry)
    bare.set_ligand_library(lib)
    tb = launch(bare, lib, water_alone(4))
    assert len(tb['i']) > 0 and bare.library_info()['poses'] == 4
    refused('planes mask of 0', planes=0, hd=bh)
    refused('unknown flag', flags=3, n_refs=65, hd=bh)
    refused('no residues resident', flags=1, n_refs=65, hd=bh)
    refused('no residues resident', flags=1, off=None, hd=bh)
    refused('n_refs', flags=0, n_refs=65, hd=bh)
    assert _fp_void(bare)
    got = bare.library_fingerprints(lfp.references([lfp.reference_from_pose(tb, 0, level='atom')]), ALL15, by_residue=False)
    assert differences(got, fold(tb, [lfp.reference_from_pose(tb, 0, level='atom')], rec.res_id, ALL15, 0x7F, 'atom')) == []
    bare.close()
    # the Python layer checks the lengths the library cannot see
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    launch(ctx, lib, water_alone(4))
    with pytest.raises(ValueError, match='ref_off\\[-1\\] entries'):
        ctx.library_fingerprints(dict(ref_off=[0, 3], ref_node=[1, 2], ref_planes=[1, 1]), ALL15)
    assert ctx.library_fingerprints(None, ALL15)['cross'].shape == (4, 0)
    ctx.close()


@pytest.mark.gpu
def test_a_caller_owned_stream_and_run_library_fingerprints_chunked(tmp_path):
    from test_gpu_paths import _hip_runtime
    rec, ligs, poses, lib, ctx, t = main_launch()
    refs = main_refs(t, rec.res_id, 'residue')
    whole = ctx.library_fingerprints(lfp.references(refs), fp.planes(None), bits=True)
    whole_best = ctx.library_fingerprints_best()
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    launch(ctx, lib, poses)
    assert _same_bytes(ctx.library_fingerprints(lfp.references(refs), fp.planes(None), bits=True), whole)
    assert _same_bytes(ctx.library_fingerprints_best(), whole_best)
    ctx.use_stream(0)                                               # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0
    off, x, h = ll.flatten_poses(lib, poses)
    ic = InteractionComplex(copy.copy(rec))
    one = ic.run_library_fingerprints(ligs, off, x, h, refs)
    keys = KEYS + ('reference_count', 'reference_cross')
    assert ic.library_fingerprints is one and one['count'].shape == (82,) and one['cross'].shape == (82, 3)
    assert np.array_equal(one['count'], whole['count'][3:]) and np.array_equal(one['cross'], whole['cross'][3:]) and np.array_equal(one['ids'], whole['ids'])
    assert np.array_equal(one['occupancy'], whole['occupancy']) and differences(one['best'], whole_best, BEST) == []
    for chunk in (32, 72):                                          # 72: the haem's three poses are cut between two launches
        part = ic.run_library_fingerprints(lib, off, x, h, lfp.references(refs), chunk=chunk)
        assert differences(part, one, keys) == [] and differences(part['best'], whole_best, BEST) == [], chunk
    # atom level, named contacts, one kind of entity: against (H)
    arefs = main_refs(t, rec.res_id, 'atom')
    atom = ic.run_library_fingerprints(ligs, off, x, h, arefs, contacts=['hbond', 'hydrophobic'], interacting_entities=['INTER'], level='atom', chunk=40)
    want = fold(t, arefs, rec.res_id, BIT['hbond'] | BIT['hydrophobic'], 1 << CT['INTER'], 'atom')
    assert np.array_equal(atom['count'], want['count'][3:]) and np.array_equal(atom['cross'], want['cross'][3:]) and np.array_equal(atom['ids'], want['ids'])
    assert np.array_equal(atom['occupancy'], want['occupancy']) and differences(atom['best'], best_of(want, t['ligand_pose_off']), BEST) == []
    path = ic.write_library_fingerprints(str(tmp_path))
    lines = open(path).read().splitlines()
    assert os.path.basename(path) == 'proteinlike.libraryfp' and len(lines) == 1 + 7 * 3 and lines[0] == ','.join(lfp.CSV_HEADER + ['pose', 'name'])
    with pytest.raises(ValueError, match='references'):
        ic.run_library_fingerprints(ligs, off, x, h, [])
    with pytest.raises(ValueError, match='level'):
        ic.run_library_fingerprints(ligs, off, x, h, refs, level='chain')
