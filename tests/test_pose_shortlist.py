"""Pose shortlist (arp_poses_shortlist_launch / _fetch / _planes_fetch / _info, Context.poses_shortlist,
arpeggio_amd.pose_shortlist, InteractionComplex.run_pose_shortlist).

The yardstick is NumPy over what the untouched full routes fetch (``Context.poses_contacts``, ``poses_planes``,
``poses_fingerprints``): scores in Python integers, the order by a stable sort of the negated score, the records by slicing with
``pose_off`` and masking (``pose_shortlist.take`` / ``take_planes``, checked by hand below).  Every comparison is exact: integers as
integers, floats as bytes, dtypes and shapes included.  No tolerance and no time anywhere."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, pose_fingerprints as fp, pose_shortlist as sl, poses
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex
from helpers import tiny_complex
from test_pose_fingerprints import ALL15, BIT, CT, PARAMS, SCATTERED, _ctx, _mask, _p, _same_bytes, chain_case, hem_case, protein

INTER = 1 << CT['INTER']
I64_MIN = -(1 << 63)


# ------------------------------------------------------------------------------------------------------------- yardstick
def expected(table, chosen, score, sift_mask=0, ctype_mask=0x7F, ptable=None, tables=('atom_atom',)):
    """What a shortlist of the poses ``chosen`` (in that order) must hold, from fully fetched tables."""
    chosen = np.asarray(chosen, np.int64).reshape(-1)
    want = dict(pose=chosen.astype(np.int32), score=np.array([int(score[p]) for p in chosen.tolist()], np.int64).reshape(-1),
                summary=np.asarray(table['summary'], np.uint32)[chosen])
    if 'atom_atom' in tables:
        t = sl.take(table, chosen, sift_mask, ctype_mask)
        want.update({c: t[c] for c in poses.COLUMNS})
        want['pose_off'] = t['pose_off']
    if ptable is not None:
        names = [n for n in tables if n != 'atom_atom']
        pt = sl.take_planes(ptable, chosen, ctype_mask, names)
        want['planes_summary'] = np.asarray(ptable['summary'], np.uint32)[chosen]
        want.update({n: pt[n] for n in names})
    return want


def differences(got, want):
    """The keys of ``want`` that ``got`` lacks or holds with another dtype, shape or bytes (sub-tables: 'table.column')."""
    bad = []
    for k, v in want.items():
        if isinstance(v, dict):
            bad += [f'{k}.{c}' for c in differences(got.get(k, {}), v)]
        elif k not in got or not _same_bytes(got[k], v):
            bad.append(k)
    return bad


def summary_scores(table, w, ptable=None):
    return sl.scores('summary', table['summary'], None if ptable is None else ptable['summary'], w)


def mixed_weights(table=None):
    """Weights of both signs on occurring slots.  Given a table, the negative weight on 'records' balances the positive ones
    over all poses: the scores scatter about zero, some poses below it."""
    plus = {'hydrophobic': 50, 'vdw': 30, 'hbond': 400, 'weak_polar': 20, 'proximal': 10}
    if table is None:
        return sl.weights(atom_atom=dict(plus, records=-15))
    total = np.asarray(table['summary']).astype(np.int64).sum(axis=0)
    gain = sum(v * int(total[config.SIFT_NAMES.index(n)]) for n, v in plus.items())
    return sl.weights(atom_atom=dict(plus, records=-int(round(gain / max(int(total[15]), 1)))))


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_table():
    """Two references and four poses.  Records per pose: 2, 1, 3, 0, 2, 2; atoms 0 and 1 are the ligand.
        pose  record  i  j   sift                 ctype
        0     0       0  5   hbond|proximal       INTER
              1       1  6   hydrophobic|vdw      INTER
        1     2       0  5   hbond|proximal       INTER
        2     3       0  5   proximal             INTER
              4       0  7   hydrophobic|vdw      INTRA_NON_SELECTION (by hand: another type)
              5       1  6   vdw                  INTER
        3     (none)
        4     6       0  8   proximal             INTRA_NON_SELECTION
              7       1  9   proximal             INTRA_NON_SELECTION
        5     8       0  5   hbond|proximal       INTER
              9       1  6   hydrophobic|vdw      INTER"""
    hp, hv, p_, v_ = BIT['hbond'] | BIT['proximal'], BIT['hydrophobic'] | BIT['vdw'], BIT['proximal'], BIT['vdw']
    other = CT['INTRA_NON_SELECTION']
    t = dict(i=np.array([0, 1, 0, 0, 0, 1, 0, 1, 0, 1], np.int32), j=np.array([5, 6, 5, 5, 7, 6, 8, 9, 5, 6], np.int32),
             dist=np.array([2.9, 3.8, 3.0, 4.6, 3.9, 3.7, 4.8, 4.9, 2.9, 3.8], np.float32),
             sift=np.array([hp, hv, hp, p_, hv, v_, p_, p_, hp, hv], np.uint16),
             ctype=np.array([CT['INTER']] * 4 + [other, CT['INTER'], other, other, CT['INTER'], CT['INTER']], np.uint8),
             pose_off=np.array([0, 2, 3, 6, 6, 8, 10], np.uint64), movable=np.array([0, 1], np.int32))
    t['summary'] = np.stack([poses.summarise(s) for s in np.split(t['sift'], t['pose_off'][1:-1].astype(np.int64))])
    return t


def test_weights_by_name():
    w = sl.weights(atom_atom={'hbond': 7, 'records': -2}, planes={'group_plane': 3, 'inter_cationpi': -(1 << 24)})
    assert w.dtype == np.int32 and w.shape == (32,)
    assert w[config.SIFT_NAMES.index('hbond')] == 7 and w[15] == -2 and w[16 + 3] == 3 and w[16 + 5] == -(1 << 24)
    assert int(np.count_nonzero(w)) == 4 and not sl.weights().any()
    for bad in (dict(atom_atom={'nonsense': 1}), dict(planes={'hbond': 1}), dict(atom_atom={'hbond': (1 << 24) + 1}), dict(atom_atom={'hbond': 0.5})):
        with pytest.raises(ValueError):
            sl.weights(**bad)
    assert sl.KINDS == ('list', 'summary', 'tanimoto') and sl.TABLES == ('atom_atom',) + poses.PLANE_TABLES
    assert sl.tables_mask('atom_atom') == 1 and sl.tables_mask(sl.TABLES) == 31 and sl.tables_mask(['group_group']) == 8
    with pytest.raises(ValueError):
        sl.tables_mask([])
    with pytest.raises(ValueError):
        sl.tables_mask(['atoms'])


def test_tanimoto_q32_by_hand():
    # references 0 (3 features) and 1 (0 features); poses: equal to ref 0, a third of it, nothing, disjoint
    count = np.array([3, 0, 3, 1, 0, 2], np.uint32)
    cross = np.array([[3, 0], [0, 0], [3, 0], [1, 0], [0, 0], [0, 0]], np.uint32)
    one = 1 << 32
    assert sl.tanimoto_q32(count, cross, 2, 0) == [one, 0, one, 1431655765, 0, 0]      # t = u; 1 / 3 = floor(2^32 / 3)
    assert sl.tanimoto_q32(count, cross, 2, 1) == [0, one, 0, 0, one, 0]               # 0 / 0 is 1.0
    assert sl.tanimoto_q32(count, cross, 2, -1) == [one, one, one, 1431655765, one, 0]
    assert all(isinstance(v, int) for v in sl.tanimoto_q32(count, cross, 2, -1))
    # the 0 / 0 rule is pose_fingerprints.tanimoto's
    t = fp.tanimoto(dict(count=count, cross=cross, n_refs=2))
    assert [int(v * one) for v in t[:, 1]] == sl.tanimoto_q32(count, cross, 2, 1)
    big = np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint32)      # beyond 2^31: Python integers do not wrap
    assert sl.tanimoto_q32(big, np.array([[0xFFFFFFFF], [0xFFFFFFFE]], np.uint32), 1, 0) == [one, (0xFFFFFFFE << 32) // 0x100000000]
    for bad in ((2, 2), (2, -2), (0, 0)):
        with pytest.raises(ValueError):
            sl.tanimoto_q32(count, cross, *bad)
    assert sl.scores('tanimoto', count=count, cross=cross, n_refs=2, ref=0) == sl.tanimoto_q32(count, cross, 2, 0)
    assert sl.scores('list', n_poses=3) == [0, 0, 0]


def test_scores_and_order_with_ties_and_skip():
    t = hand_table()
    w = sl.weights(atom_atom={'hbond': 10, 'hydrophobic': 1, 'proximal': -2})
    s = sl.scores('summary', t['summary'], None, w)
    assert s == [9, 8, -1, 0, -4, 9] and all(isinstance(v, int) for v in s)
    assert sl.order(s).tolist() == [0, 5, 1, 3, 2, 4] and sl.order(s).dtype == np.int64      # the tie 0 / 5 goes to the lower id
    assert sl.order(s, skip=1).tolist() == [5, 1, 3, 2, 4] and sl.order(s, skip=2, k=2).tolist() == [5, 3]
    assert sl.order(s, k=100).tolist() == [0, 5, 1, 3, 2, 4]
    assert sl.order(s, min_score=8).tolist() == [0, 5, 1] and sl.order(s, min_score=9, k=1).tolist() == [0] and sl.order(s, min_score=10).tolist() == []
    assert sl.order([0] * 5, skip=2).tolist() == [2, 3, 4]
    # the planes half of the weights
    ps = np.zeros((6, 16), np.uint32)
    ps[:, 3] = [0, 0, 0, 4, 0, 0]
    w2 = sl.weights(atom_atom={'hbond': 10, 'hydrophobic': 1, 'proximal': -2}, planes={'group_plane': 3})
    assert sl.scores('summary', t['summary'], ps, w2) == [9, 8, -1, 12, -4, 9]
    with pytest.raises(ValueError):
        sl.scores('summary', t['summary'], None, w2)
    with pytest.raises(ValueError):
        sl.scores('rank', t['summary'], None, w)
    # the extremes fit: 32 slots of 2^32 - 1 at weight -2^24
    full = np.full((1, 16), 0xFFFFFFFF, np.uint32)
    assert sl.scores('summary', full, full, np.full(32, -(1 << 24), np.int32)) == [-32 * (1 << 24) * 0xFFFFFFFF]


def test_take_with_both_masks_and_a_pose_that_loses_every_record():
    t = hand_table()
    ids = [2, 0, 3, 4, 0]
    got = sl.take(t, ids)
    assert got['pose_off'].tolist() == [0, 3, 5, 5, 7, 9] and got['pose_off'].dtype == np.uint64
    assert got['j'].tolist() == [5, 7, 6, 5, 6, 8, 9, 5, 6] and got['pose'].tolist() == ids and got['pose'].dtype == np.int32
    assert all(got[c].dtype == poses.DTYPES[c] for c in poses.COLUMNS) and np.array_equal(got['summary'], t['summary'][ids])
    assert np.array_equal(got['movable'], t['movable']) and got['dist'].tobytes() == t['dist'][[3, 4, 5, 0, 1, 6, 7, 0, 1]].tobytes()
    got = sl.take(t, ids, sift_mask=BIT['hbond'] | BIT['hydrophobic'])      # at least one of the two bits
    assert got['pose_off'].tolist() == [0, 1, 3, 3, 3, 5] and got['j'].tolist() == [7, 5, 6, 5, 6]
    got = sl.take(t, ids, ctype_mask=INTER)
    assert got['pose_off'].tolist() == [0, 2, 4, 4, 4, 6] and got['j'].tolist() == [5, 6, 5, 6, 5, 6]      # pose 4 loses every record
    got = sl.take(t, ids, sift_mask=BIT['hydrophobic'], ctype_mask=INTER)
    assert got['pose_off'].tolist() == [0, 0, 1, 1, 1, 2] and got['j'].tolist() == [6, 6]
    assert np.array_equal(got['summary'], t['summary'][ids])               # the summary counts what the pose has
    assert sl.take(t, [])['pose_off'].tolist() == [0] and len(sl.take(t, [])['i']) == 0
    # ... and the ring / amide tables: the columns of poses_planes, filtered by ctype alone
    pt = poses.empty_planes(6)
    gg = pt['group_group']
    gg.update(bgn=np.array([1, 2, 3], np.int32), end=np.array([4, 5, 6], np.int32), dist=np.array([3.5, 3.6, 3.7], np.float32),
              dihedral=np.zeros(3, np.float32), theta=np.zeros(3, np.float32), ctype=np.array([CT['INTER'], CT['INTRA_SELECTION'], CT['INTER']], np.uint8),
              pose_off=np.array([0, 1, 1, 3, 3, 3, 3], np.uint64))
    got = sl.take_planes(pt, [2, 2, 0], INTER)
    assert got['group_group']['bgn'].tolist() == [3, 3, 1] and got['group_group']['pose_off'].tolist() == [0, 1, 2, 3]
    assert got['group_group']['dist'].dtype == np.float32 and got['atom_plane']['dist'].dtype == np.float64 and got['summary'].shape == (3, 16)
    assert sl.take_planes(pt, [2], 0x7F, ['group_group'])['group_group']['end'].tolist() == [5, 6]


def _short_of(t, ids, score, base=0):
    s = sl.take(t, ids)
    s['score'] = np.asarray(score, np.int64)
    return sl.shift(s, base)


def test_merge_with_a_tie_across_chunks_and_k_larger_than_what_there_is():
    t = hand_table()
    # chunk a holds the global poses 0 ... 2, chunk b 3 ... 5 (local ids 0 ... 2 of a table of its own)
    tb = sl.take(t, [3, 4, 5])
    a = _short_of(t, [0, 1], [9, 8])
    b = _short_of(tb, [2, 0], [9, 0], base=3)
    m = sl.merge([b, a], 3)
    assert m['pose'].tolist() == [0, 5, 1] and m['score'].tolist() == [9, 9, 8] and m['score'].dtype == np.int64      # the tie: lower global id
    assert m['pose_off'].tolist() == [0, 2, 4, 5] and m['j'].tolist() == [5, 6, 5, 6, 5]
    assert np.array_equal(m['summary'], t['summary'][[0, 5, 1]]) and np.array_equal(m['movable'], t['movable'])
    assert all(m[c].dtype == poses.DTYPES[c] for c in poses.COLUMNS)
    m = sl.merge([a, b], 100)
    assert m['pose'].tolist() == [0, 5, 1, 3] and m['pose_off'].tolist() == [0, 2, 4, 5, 5]
    assert sl.merge([a], 1)['pose'].tolist() == [0] and sl.merge([a, b], 0)['pose'].tolist() == []
    with pytest.raises(ValueError):
        sl.merge([], 3)


def test_records_and_the_csv_text(tmp_path):
    pc = protein()
    t = hand_table()
    s = _short_of(t, [5, 3, 2], [9, 0, -1])
    recs = sl.to_records(s, pc)
    assert len(recs) == 5 and [(r['rank'], r['pose'], r['score']) for r in recs] == [(0, 5, 9), (0, 5, 9), (2, 2, -1), (2, 2, -1), (2, 2, -1)]
    assert recs[0]['contact'] == ['proximal', 'hbond'] and recs[0]['type'] == 'atom-atom' and recs[2]['interacting_entities'] == 'INTER'
    ic = InteractionComplex(pc)
    with pytest.raises(AttributeError):
        ic.write_pose_shortlist(str(tmp_path))
    ic.pose_shortlist = s
    path = ic.write_pose_shortlist(str(tmp_path))
    assert os.path.basename(path) == 'proteinlike.shortlist'
    from arpeggio_amd.core import export
    lab = export.Labels(pc, pc.component_types)
    name = [lab.atom_macro(k) for k in range(10)]
    assert name[0] == 'A/1/%s' % pc.atom_name[0]
    assert open(path).read().splitlines() == [
        'rank,pose,score,atom_bgn,atom_end,distance,contacts,interacting_entities',
        f'0,5,9,{name[0]},{name[5]},2.9,proximal|hbond,INTER',
        f'0,5,9,{name[1]},{name[6]},3.8,vdw|hydrophobic,INTER',
        f'2,2,-1,{name[0]},{name[5]},4.6,proximal,INTER',
        f'2,2,-1,{name[0]},{name[7]},3.9,vdw|hydrophobic,INTRA_NON_SELECTION',
        f'2,2,-1,{name[1]},{name[6]},3.7,vdw,INTER']


def test_the_header_and_the_binding_name_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    for s in ('arp_poses_shortlist_launch', 'arp_poses_shortlist_fetch', 'arp_poses_shortlist_planes_fetch', 'arp_poses_shortlist_info'):
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    for name, v in (('LIST', _capi.SHORTLIST_LIST), ('SUMMARY', _capi.SHORTLIST_SUMMARY), ('TANIMOTO', _capi.SHORTLIST_TANIMOTO),
                    ('TABLES', _capi.SHORTLIST_TABLES)):
        assert '#define ARP_SHORTLIST_%s %d' % (name, v) in hdr
    assert '#define ARP_SHORTLIST_MAX_WEIGHT (1 << 24)' in hdr and sl.MAX_WEIGHT == _capi.SHORTLIST_MAX_WEIGHT == 1 << 24
    assert [sl.KINDS.index(k) for k in ('list', 'summary', 'tanimoto')] == [_capi.SHORTLIST_LIST, _capi.SHORTLIST_SUMMARY, _capi.SHORTLIST_TANIMOTO]
    assert sl.NO_THRESHOLD == _capi.INT64_MIN == I64_MIN and len(sl.TABLES) == _capi.SHORTLIST_TABLES


# ------------------------------------------------------------------------------------------------------------- GPU: contents
@pytest.mark.gpu
@pytest.mark.parametrize('params', PARAMS, ids=[f'{c}-{v}-{int(s)}' for c, v, s in PARAMS])
def test_contents_on_the_haem(params):
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, *params)
    w = mixed_weights(table)
    score = summary_scores(table, w)
    assert min(score) < 0 < max(score) and len(set(score)) > 20                      # the sign of the key is exercised
    per_pose = np.diff(table['pose_off'].astype(np.int64))
    assert per_pose.max() > 128 and (per_pose % 64 != 0).any()                      # segments far longer than a wave
    for skip in (0, 3):
        ranked = sl.order(score, skip)
        for k in (1, 7, 64, 65, 1000):
            got = ctx.poses_shortlist('summary', weights=w, skip=skip, k=k)
            want = expected(table, ranked[:k], score)
            assert len(want['pose']) == min(k, 70 - skip)
            assert differences(got, want) == [], (skip, k)
            info = ctx.poses_shortlist_info()
            assert (info['chosen'], info['atom_atom'], info['kind']) == (len(want['pose']), len(want['i']), _capi.SHORTLIST_SUMMARY)
            assert info['atom_plane'] == info['group_plane'] == 0 and 'planes_summary' not in got and np.array_equal(got['movable'], table['movable'])
    # the shortlist is a poses table of K poses
    got = ctx.poses_shortlist('summary', weights=w, k=7)
    per = poses.split(got)
    full = poses.split(table)
    assert len(per) == 7 and all(_same_bytes(per[r], full[p]) for r, p in enumerate(got['pose'].tolist()))
    assert _same_bytes(poses.fingerprints(got, pc)[0].any(axis=1), poses.fingerprints(table, pc)[0][got['pose']].any(axis=1))
    assert len(poses.to_records(got, pc)) == len(got['i'])
    ctx.close()


@pytest.mark.gpu
def test_ties_and_empty_segments():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, False)
    zero = sl.weights()
    for skip in (0, 3):      # every pose ties: the poses in order
        got = ctx.poses_shortlist('summary', weights=zero, skip=skip, k=10)
        assert got['pose'].tolist() == list(range(skip, skip + 10)) and not got['score'].any()
        assert differences(got, expected(table, range(skip, skip + 10), [0] * 70)) == []
    ctx.close()
    pc, idx, x, h = chain_case(12)
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, True)
    per_pose = np.diff(table['pose_off'].astype(np.int64)).tolist()
    assert per_pose == [2] + [3] * 10 + [2, 0]                                      # interior poses tie; the far pose has no record
    w = sl.weights(atom_atom={'records': 1})
    score = summary_scores(table, w)
    got = ctx.poses_shortlist('summary', weights=w)
    assert got['pose'].tolist() == list(range(1, 11)) + [0, 11, 12] == sl.order(score).tolist()
    assert differences(got, expected(table, sl.order(score), score)) == [] and got['pose_off'].tolist()[-2:] == [34, 34]
    w = sl.weights(atom_atom={'records': -1})
    score = summary_scores(table, w)
    got = ctx.poses_shortlist('summary', weights=w)
    assert got['pose'].tolist() == [12, 0, 11] + list(range(1, 11)) and got['pose_off'].tolist()[:3] == [0, 0, 2]      # the empty segment in front
    assert differences(got, expected(table, sl.order(score), score)) == []
    ctx.close()


@functools.lru_cache(maxsize=None)
def seam_case():
    """Three clusters of 63, 64 and 65 receptor atoms, a residue each, on 4 A spheres about centres 40 A apart, and one movable
    atom: pose k sits at centre k, pose 3 is 100 A away."""
    def sphere(n):
        k = np.arange(n) + 0.5
        phi, th = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
        return 4.0 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    centres = np.array([[0.0, 0.0, 0.0], [40.0, 0.0, 0.0], [80.0, 0.0, 0.0]])
    atoms = np.concatenate([centres[c] + sphere(n) for c, n in enumerate((63, 64, 65))])
    pc = tiny_complex(np.concatenate([atoms, [[0.0, -200.0, 0.0]]]))
    x = np.concatenate([centres, [[0.0, 100.0, 0.0]]]).astype(np.float32)[:, None, :]
    return pc, np.array([len(atoms)]), x, np.zeros((4, 0, 3))


@pytest.mark.gpu
def test_segment_lengths_on_the_wave_seam():
    pc, idx, x, h = seam_case()
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, True)
    assert np.diff(table['pose_off'].astype(np.int64)).tolist() == [63, 64, 65, 0]      # the condition, on the yardstick
    for ids in ((2, 0, 3, 1), (3,), (1, 1, 2)):
        got = ctx.poses_shortlist('list', pose_ids=ids)
        assert differences(got, expected(table, ids, [0] * 4)) == [], ids
        assert got['pose'].tolist() == list(ids) and not got['score'].any() and ctx.poses_shortlist_info()['kind'] == _capi.SHORTLIST_LIST
    w = sl.weights(atom_atom={'records': 1})
    score = summary_scores(table, w)
    got = ctx.poses_shortlist('summary', weights=w, k=4)
    assert got['pose'].tolist() == [2, 1, 0, 3] and got['pose_off'].tolist() == [0, 65, 129, 192, 192]
    assert differences(got, expected(table, [2, 1, 0, 3], score)) == []
    # a filter that keeps everything takes the counting path over the same seams
    got = ctx.poses_shortlist('list', pose_ids=(1, 2, 0), sift_mask=ALL15)
    want = expected(table, (1, 2, 0), [0] * 4, sift_mask=ALL15)
    assert differences(got, want) == [] and want['pose_off'].tolist() == [0, 64, 129, 192]
    ctx.close()


@pytest.mark.gpu
def test_the_record_filter():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, False)
    w = mixed_weights(table)
    score = summary_scores(table, w)
    ranked = sl.order(score)
    rare = next(b for b in sorted(BIT.values(), key=lambda b: int(((table['sift'] & b) != 0).sum())) if ((table['sift'] & b) != 0).any())
    nothing = 0
    for sift_mask, ctype_mask in ((SCATTERED, 0x7F), (0, INTER), (SCATTERED, INTER), (rare, INTER), (rare, 0x7F)):
        for k in (9, 70):
            want = expected(table, ranked[:k], score, sift_mask, ctype_mask)
            got = ctx.poses_shortlist('summary', weights=w, k=k, sift_mask=sift_mask, ctype_mask=ctype_mask)
            assert differences(got, want) == [], (sift_mask, ctype_mask, k)
            assert len(want['i']) < int(table['pose_off'][-1])                      # the filter drops records ...
            assert len(want['i']) > 0 or sift_mask == rare                          # ... and not all (the rare bit may keep none of nine poses)
            assert np.array_equal(got['summary'], table['summary'][ranked[:k]])     # ... the summary rows stay the unfiltered ones
            nothing += int((np.diff(want['pose_off'].astype(np.int64)) == 0).sum())
    assert nothing > 0                                                              # a chosen pose that keeps nothing (of the yardstick)
    ctx.close()


@pytest.mark.gpu
def test_min_score():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, False)
    w = mixed_weights(table)
    score = summary_scores(table, w)
    levels = sorted(set(score), reverse=True)
    assert levels[4] - levels[5] >= 1
    between, equal = levels[5] + (1 if levels[4] - levels[5] > 1 else 0), levels[7]
    for thr in (between, equal):
        for k in (1000, 3):
            want_ids = sl.order(score, 0, k, thr)
            got = ctx.poses_shortlist('summary', weights=w, k=k, min_score=thr)
            assert differences(got, expected(table, want_ids, score)) == [], (thr, k)
    assert len(sl.order(score, 0, None, equal)) == sum(1 for v in score if v >= equal) and min(got['score'].tolist()) >= equal
    assert equal in ctx.poses_shortlist('summary', weights=w, min_score=equal)['score'].tolist()      # inclusive
    # above the best score: a valid, empty shortlist
    got = ctx.poses_shortlist('summary', weights=w, k=5, min_score=levels[0] + 1)
    assert differences(got, expected(table, [], score)) == [] and got['pose'].shape == (0,) and got['pose_off'].tolist() == [0]
    info = ctx.poses_shortlist_info()
    assert (info['chosen'], info['atom_atom'], info['kind']) == (0, 0, _capi.SHORTLIST_SUMMARY) and info['launches'] >= 1
    n, m = C.c_int64(-1), C.c_int64(-1)
    buf = np.zeros(16, np.int64)
    rc = ctx._L.arp_poses_shortlist_fetch(ctx._h, 0, 0, _p(buf), _p(buf), _p(buf), None, _p(buf), None, None, None, None, None, C.byref(n), C.byref(m))
    assert rc == _capi.ARP_OK and (n.value, m.value) == (0, 0) and not buf.any()
    ctx.close()


@pytest.mark.gpu
def test_tanimoto():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, False)
    f = ctx.poses_fingerprints(ALL15 & ~BIT['proximal'], n_refs=2)
    for ref in (0, 1, -1):
        score = sl.tanimoto_q32(f['count'], f['cross'], 2, ref)
        assert len(set(score[2:])) > 10 and max(score[2:]) < 1 << 32
        for k in (5, 1000):
            got = ctx.poses_shortlist('tanimoto', ref=ref, skip=2, k=k)
            assert differences(got, expected(table, sl.order(score, 2, k), score)) == [], (ref, k)
        assert 0 not in got['pose'].tolist() and 1 not in got['pose'].tolist() and ctx.poses_shortlist_info()['kind'] == _capi.SHORTLIST_TANIMOTO
    best = [max(a, b) for a, b in zip(sl.tanimoto_q32(f['count'], f['cross'], 2, 0), sl.tanimoto_q32(f['count'], f['cross'], 2, 1))]
    assert best == sl.tanimoto_q32(f['count'], f['cross'], 2, -1) and best != sl.tanimoto_q32(f['count'], f['cross'], 2, 0)
    # skip = 0 ranks the references too: a reference is its own best match
    got = ctx.poses_shortlist('tanimoto', ref=0, k=1)
    assert got['pose'].tolist() == [0] and got['score'].tolist() == [1 << 32]
    ctx.close()
    # 0 / 0: the reference and one pose are both far away
    pc, idx, x, h = chain_case(12)
    x = np.concatenate([x[12:], x[:12], x[12:]])
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, np.zeros((14, 0, 3)), 5.0, 0.1, True)
    f = ctx.poses_fingerprints(ALL15, n_refs=1)
    score = sl.tanimoto_q32(f['count'], f['cross'], 1, 0)
    assert f['count'][0] == 0 and score[13] == 1 << 32 and max(score[1:13]) == 0
    got = ctx.poses_shortlist('tanimoto', ref=0, skip=1)
    assert got['pose'].tolist() == [13] + list(range(1, 13)) and got['score'][0] == 1 << 32
    assert differences(got, expected(table, sl.order(score, 1), score)) == []
    ctx.close()


@functools.lru_cache(maxsize=None)
def ring_case():
    """The mid-chain PHE of the relabelled small protein: a moved ring and two amides — records in all four ring / amide tables."""
    import test_pose_plane_fingerprints as tppf
    return tppf.case('phe')


def _ring_ctx():
    pc, idx, x, h = ring_case()
    ctx = _ctx(pc, idx)
    ctx.set_plane_atoms(pc)
    return ctx, pc, idx, x, h


@pytest.mark.gpu
def test_the_planes_tables_and_a_fingerprint_with_class_planes():
    ctx, pc, idx, x, h = _ring_ctx()
    table = ctx.poses_contacts(x, h, 5.0, 0.1, False)
    ptable = ctx.poses_planes(x)
    w = sl.weights(atom_atom={'hbond': 1}, planes={'group_plane': 1000, 'group_group': 100, 'plane_plane': 7, 'atom_plane': -3})
    score = summary_scores(table, w, ptable)
    ranked = sl.order(score)
    types = sorted(set(np.concatenate([ptable[n]['ctype'] for n in poses.PLANE_TABLES]).tolist()))
    assert len(types) >= 2
    partial = 1 << types[0]
    for ctype_mask in (0x7F, partial):
        want = expected(table, ranked[:24], score, 0, ctype_mask, ptable, sl.TABLES)
        for name in poses.PLANE_TABLES:      # every table holds kept records of a chosen pose (of the yardstick)
            assert len(want[name]['ctype']) > 0, (name, ctype_mask)
        if ctype_mask == partial:
            assert any(len(want[n]['ctype']) < len(expected(table, ranked[:24], score, 0, 0x7F, ptable, sl.TABLES)[n]['ctype']) for n in poses.PLANE_TABLES)
        got = ctx.poses_shortlist('summary', weights=w, k=24, tables=sl.TABLES, ctype_mask=ctype_mask)
        assert differences(got, want) == [], ctype_mask
        assert got['group_group']['dist'].dtype == np.float32 and got['group_plane']['dist'].dtype == np.float64
        info = ctx.poses_shortlist_info()
        assert [info[n] for n in sl.TABLES] == [len(want['i'])] + [len(want[n]['ctype']) for n in poses.PLANE_TABLES]
        per = poses.split_planes(dict(got, summary=got['planes_summary']))
        assert len(per) == 24 and len(per[0]['group_plane']['ctype']) == int(np.diff(want['group_plane']['pose_off'].astype(np.int64))[0])
    # without the atom-atom table
    names = ('plane_plane', 'group_plane')
    got = ctx.poses_shortlist('summary', weights=w, k=9, tables=names, ctype_mask=partial)
    want = expected(table, ranked[:9], score, 0, partial, ptable, names)
    assert differences(got, want) == [] and 'i' not in got and 'pose_off' not in got and 'atom_plane' not in got
    n, m = C.c_int64(0), C.c_int64(0)
    off = np.zeros(10, np.uint64)
    args = (None,) * 5
    assert ctx._L.arp_poses_shortlist_fetch(ctx._h, 9, 0, None, None, None, None, _p(off), *args, C.byref(n), C.byref(m)) == _capi.ARP_E_ARG
    assert 'not requested' in ctx._L.arp_last_error(ctx._h).decode()
    assert ctx._L.arp_poses_shortlist_planes_fetch(ctx._h, 0, 9, 0, _p(off), *([None] * 9), C.byref(m)) == _capi.ARP_E_ARG
    assert 'not requested' in ctx._L.arp_last_error(ctx._h).decode()
    v = np.zeros(64, np.float64)
    assert ctx._L.arp_poses_shortlist_planes_fetch(ctx._h, 3, 9, 64, None, None, None, None, None, None, _p(v), None, None, None, C.byref(m)) == _capi.ARP_E_ARG
    assert 'no such value column' in ctx._L.arp_last_error(ctx._h).decode()
    assert ctx._L.arp_poses_shortlist_planes_fetch(ctx._h, 3, 9, 64, None, None, None, None, None, None, None, None, _p(v), None, C.byref(m)) == _capi.ARP_E_ARG
    assert 'no such byte column' in ctx._L.arp_last_error(ctx._h).decode()
    # the kind does not care which entry made the fingerprint: one with class planes
    f = ctx.poses_fingerprints(fp.planes(classes='all'), n_refs=2)
    ts = sl.tanimoto_q32(f['count'], f['cross'], 2, -1)
    got = ctx.poses_shortlist('tanimoto', ref=-1, skip=2, k=6, tables=('atom_atom', 'atom_plane'))
    assert differences(got, expected(table, sl.order(ts, 2, 6), ts, 0, 0x7F, ptable, ('atom_atom', 'atom_plane'))) == []
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
def _launch(ctx, kind=1, weights=None, ref=0, ids=None, skip=0, k=5, min_score=I64_MIN, tables=1, sift_mask=0, ctype_mask=0x7F, n_ids=None):
    info = np.zeros(8, np.int64)
    w = None if weights is None else np.ascontiguousarray(weights, np.int32)
    i = None if ids is None else np.ascontiguousarray(ids, np.int32)
    rc = ctx._L.arp_poses_shortlist_launch(ctx._h, kind, _p(w), ref, _p(i), (0 if i is None else len(i)) if n_ids is None else n_ids, skip, k, min_score,
                                           tables, sift_mask, ctype_mask, _p(info))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), info


def _same_resident(a, b):
    return a[0] == b[0] and _same_bytes(a[2], b[2])


def _resident(ctx, planes=False):
    """The resident shortlist, fetched without a launch: (rc, message, arrays)."""
    info = ctx.poses_shortlist_info()
    K, k = info['chosen'], info['atom_atom']
    out = dict(pose=np.empty(K, np.int32), score=np.empty(K, np.int64), summary=np.empty((K, 16), np.uint32), off=np.empty(K + 1, np.uint64),
               i=np.empty(k, np.int32), j=np.empty(k, np.int32), dist=np.empty(k, np.float32), sift=np.empty(k, np.uint16), ctype=np.empty(k, np.uint8))
    if planes:
        out['planes_summary'] = np.empty((K, 16), np.uint32)
    n, m = C.c_int64(-1), C.c_int64(-1)
    rc = ctx._L.arp_poses_shortlist_fetch(ctx._h, K, k, _p(out['pose']), _p(out['score']), _p(out['summary']), _p(out.get('planes_summary')), _p(out['off']),
                                          _p(out['i']), _p(out['j']), _p(out['dist']), _p(out['sift']), _p(out['ctype']), C.byref(n), C.byref(m))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), out


@pytest.mark.gpu
def test_every_refusal_names_its_cause_and_touches_nothing():
    ctx, pc, idx, x, h = _ring_ctx()
    w = mixed_weights()
    rc, msg, _ = _launch(ctx, weights=w)
    assert rc == _capi.ARP_E_ARG and 'no poses result' in msg
    ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    good = ctx.poses_shortlist('summary', weights=w, k=5)
    launches = ctx.poses_shortlist_info()['launches']
    before = _resident(ctx)
    assert before[0] == _capi.ARP_OK and np.array_equal(before[2]['pose'], good['pose'])
    wp = w.copy()
    wp[16] = 1
    big = w.copy()
    big[3] = (1 << 24) + 1

    def refused(word, code=_capi.ARP_E_ARG, **kw):
        kw.setdefault('weights', w)
        rc, msg, _ = _launch(ctx, **kw)
        assert rc == code and word in msg, (word, rc, msg)
    refused('unknown kind', kind=3)
    refused('unknown kind', kind=-1)
    refused('weights missing', weights=None)
    refused('weights has an entry beyond', weights=big)
    refused('weights has an entry beyond', weights=-big)
    refused('pose_ids missing', kind=0, k=0)
    refused('n_ids', kind=0, k=0, ids=[0], n_ids=0)
    refused('n_ids', kind=0, k=0, ids=[0], n_ids=(1 << 20) + 1)
    refused('pose_ids has an id outside', kind=0, k=0, ids=[0, 9])
    refused('pose_ids has an id outside', kind=0, k=0, ids=[-1])
    refused('ARP_SHORTLIST_LIST takes skip = 0', kind=0, k=1, ids=[0])
    refused('ARP_SHORTLIST_LIST takes skip = 0', kind=0, k=0, skip=1, ids=[0])
    refused('ARP_SHORTLIST_LIST takes skip = 0', kind=0, k=0, min_score=0, ids=[0])
    refused('skip must be in', skip=-1)
    refused('skip must be in', skip=9)
    refused('k must be at least 1', k=0)
    refused('tables must be', tables=0)
    refused('tables must be', tables=32)
    refused('sift_mask has bits beyond', sift_mask=1 << 15)
    refused('ctype_mask has bits beyond', ctype_mask=0x80)
    refused('ctype_mask of 0', ctype_mask=0)
    refused('no fingerprint result', kind=2)
    refused('no poses-planes result', tables=3)
    refused('no poses-planes result', weights=wp)
    ctx.run_enqueue(5.0, 0.1, False)
    refused('not been waited for')
    ctx.run_wait()
    ctx.poses_fingerprints(ALL15, n_refs=0)
    refused('no references', kind=2)
    ctx.poses_fingerprints(ALL15, n_refs=2)
    refused('ref must be', kind=2, ref=2)
    refused('ref must be', kind=2, ref=-2)
    ctx.poses_planes(x[:8])
    refused('differ in P or S', tables=2)
    refused('differ in P or S', weights=wp)
    # none of them touched the resident shortlist
    assert ctx.poses_shortlist_info()['launches'] == launches and _same_resident(_resident(ctx), before)
    ctx.close()


@pytest.mark.gpu
def test_refusals_leave_the_resident_shortlist_byte_equal():
    ctx, pc, idx, x, h = _ring_ctx()
    w = mixed_weights()
    ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    ctx.poses_shortlist('summary', weights=w, k=5, sift_mask=SCATTERED)
    launches = ctx.poses_shortlist_info()
    before = _resident(ctx)
    assert before[0] == _capi.ARP_OK and len(before[2]['i']) > 0 and launches['launches'] == 1
    ctx.poses_planes(x[:8])
    rc, msg, _ = _launch(ctx, weights=w, tables=2)
    assert rc == _capi.ARP_E_ARG and 'differ in P or S' in msg
    assert ctx.poses_shortlist_info() == launches and _same_resident(_resident(ctx), before)
    assert ctx._L.arp_poses_shortlist_launch(None, 1, _p(w), 0, None, 0, 0, 5, I64_MIN, 1, 0, 0x7F, _p(np.zeros(8, np.int64))) == _capi.ARP_E_ARG
    assert ctx._L.arp_poses_shortlist_launch(ctx._h, 1, _p(w), 0, None, 0, 0, 5, I64_MIN, 1, 0, 0x7F, None) == _capi.ARP_E_ARG
    # made from different poses: found on the device, no shortlist is left
    other = x[:9].copy()
    other[4, 0, 0] += np.float32(0.5)
    ctx.poses_planes(other)
    rc, msg, _ = _launch(ctx, weights=w, tables=3)
    assert rc == _capi.ARP_E_ARG and 'made from different poses' in msg
    rc, msg, _ = _resident(ctx)
    assert rc == _capi.ARP_E_ARG and 'no result' in msg and ctx.poses_shortlist_info()['chosen'] == 0
    # ... and the same poses are accepted
    ctx.poses_planes(x[:9])
    assert _launch(ctx, weights=w, tables=3)[0] == _capi.ARP_OK and _resident(ctx, planes=True)[0] == _capi.ARP_OK
    ctx.close()


@pytest.mark.gpu
def test_the_shortlist_goes_with_its_sources():
    ctx, pc, idx, x, h = _ring_ctx()
    m = _mask(pc, idx)
    w = mixed_weights()
    params = (5.0, 0.1, False)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and 'no result' in _resident(ctx)[1]
    assert ctx.poses_shortlist_info() == dict(chosen=0, atom_atom=0, atom_plane=0, plane_plane=0, group_group=0, group_plane=0, launches=0, kind=0)
    table = ctx.poses_contacts(x[:9], h[:9], *params)
    first = ctx.poses_shortlist('summary', weights=w, k=5)
    # a repeated launch with other arguments remakes the result
    second = ctx.poses_shortlist('list', pose_ids=[8, 1])
    assert ctx.poses_shortlist_info()['launches'] == 2 and differences(second, expected(table, [8, 1], [0] * 9)) == []
    assert _same_bytes(ctx.poses_shortlist('summary', weights=w, k=5), first)
    # one that did not read the planes result is untouched by the planes entries
    before = _resident(ctx)
    ctx.poses_planes(x[:9])
    ctx.set_plane_atoms(pc)
    assert _same_resident(_resident(ctx), before) and before[0] == _capi.ARP_OK
    # one that read it goes with it
    ctx.poses_planes(x[:9])
    for void in (lambda: ctx.poses_planes(x[:9]), lambda: ctx.set_plane_atoms(pc)):
        ctx.poses_shortlist('summary', weights=w, k=5, tables=('atom_atom', 'atom_plane'))
        assert _resident(ctx, planes=True)[0] == _capi.ARP_OK
        void()
        rc, msg, _ = _resident(ctx)
        assert rc == _capi.ARP_E_ARG and 'no result' in msg and ctx.poses_shortlist_info()['chosen'] == 0
        ctx.poses_planes(x[:9])
    # a new poses result, a new selection, a new structure, models
    launches = ctx.poses_shortlist_info()['launches']
    ctx.poses_shortlist('summary', weights=w, k=5)
    ctx.poses_contacts(x[:9], h[:9], *params)                          # the same poses again: still a new result
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    assert ctx.poses_shortlist_info() == dict(chosen=0, atom_atom=0, atom_plane=0, plane_plane=0, group_group=0, group_plane=0, launches=launches + 1, kind=0)
    assert _same_bytes(ctx.poses_shortlist('summary', weights=w, k=5), first)
    ctx.set_selection(m)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.poses_contacts(x[:9], h[:9], *params)
    ctx.poses_shortlist('summary', weights=w, k=5)
    assert _resident(ctx)[0] == _capi.ARP_OK
    ctx.set_complex(pc)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.set_selection(m)
    ctx.poses_contacts(x[:9], h[:9], *params)
    ctx.poses_shortlist('summary', weights=w, k=5)
    ctx.set_topology(pc)
    X, H = poses.as_models(pc, idx, x[:2], h[:2])
    ctx.set_models(X, H)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.close()


@pytest.mark.gpu
def test_a_launch_reads_no_bag_and_voids_nothing():
    from test_pose_fingerprints import _fetch_everything
    ctx, pc, idx, x, h = _ring_ctx()
    counts = ctx.run_launch(5.0, 0.1, False)
    assert counts['atom_atom'] > 0 and len(ctx.residue_pairs()['res_a']) > 0
    label, net = ctx.networks(ALL15, 0x7F, True)
    ctx.poses_planes(x[:9])
    ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    f = ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    before = _fetch_everything(ctx)
    w = sl.weights(atom_atom={'hbond': 3, 'proximal': -1}, planes={'atom_plane': 2})
    for kw in (dict(kind='summary', weights=w, k=4, tables=sl.TABLES), dict(kind='tanimoto', ref=-1, skip=2, k=3, sift_mask=SCATTERED),
               dict(kind='list', pose_ids=[3, 3, 0], tables=('group_group',), ctype_mask=INTER)):
        got = ctx.poses_shortlist(kw.pop('kind'), **kw)
        assert len(got['pose']) in (3, 4)
        assert _same_bytes(_fetch_everything(ctx), before)
        assert _same_bytes(ctx.poses_fingerprints(ALL15, n_refs=2, bits=True), f) and ctx.poses_fingerprints_info()['launches'] == 1
        again = ctx.networks(ALL15, 0x7F, True)
        assert _same_bytes(again[0], label) and _same_bytes(again[1], net)
    ctx.close()


@pytest.mark.gpu
def test_null_pointers_capacity_and_a_caller_owned_stream():
    from test_gpu_paths import _hip_runtime
    ctx, pc, idx, x, h = _ring_ctx()
    table = ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    ptable = ctx.poses_planes(x[:9])
    w = sl.weights(atom_atom={'records': 1}, planes={'atom_plane': 5})
    want = ctx.poses_shortlist('summary', weights=w, k=6, tables=('atom_atom', 'atom_plane'))
    K, k, kp = 6, len(want['i']), len(want['atom_plane']['ctype'])
    assert k > 0 and kp > 0
    L, hd = ctx._L, ctx._h
    n, m = C.c_int64(0), C.c_int64(0)
    none = [None] * 10
    assert L.arp_poses_shortlist_fetch(hd, 0, 0, *none, C.byref(n), C.byref(m)) == _capi.ARP_OK and (n.value, m.value) == (K, k)
    assert L.arp_poses_shortlist_fetch(hd, 0, 0, *none, None, C.byref(m)) == _capi.ARP_E_ARG
    assert L.arp_poses_shortlist_fetch(hd, 0, 0, *none, C.byref(n), None) == _capi.ARP_E_ARG
    per_pose = dict(pose=(0, want['pose']), score=(1, want['score']), summary=(2, want['summary']), planes_summary=(3, want['planes_summary']),
                    off=(4, want['pose_off']))
    for key, (slot, ref) in per_pose.items():
        buf = np.full(ref.shape, 7, ref.dtype)
        args = list(none)
        args[slot] = _p(buf)
        n.value = m.value = 0
        assert L.arp_poses_shortlist_fetch(hd, K - 1, 0, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_CAPACITY, key
        assert (n.value, m.value) == (K, k) and (buf == 7).all() and 'too small' in L.arp_last_error(hd).decode()
        assert L.arp_poses_shortlist_fetch(hd, K, 0, *args, C.byref(n), C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, ref), key      # one array alone
    for slot, key in enumerate(poses.COLUMNS):
        buf = np.full(k, 7, want[key].dtype)
        args = list(none)
        args[5 + slot] = _p(buf)
        assert L.arp_poses_shortlist_fetch(hd, 0, k - 1, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_CAPACITY and (buf == 7).all()
        assert L.arp_poses_shortlist_fetch(hd, 0, k, *args, C.byref(n), C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, want[key]), key
    # the planes fetch: the same protocol
    tab = want['atom_plane']
    assert L.arp_poses_shortlist_planes_fetch(hd, 0, 0, 0, *none, C.byref(m)) == _capi.ARP_OK and m.value == kp
    assert L.arp_poses_shortlist_planes_fetch(hd, 0, 0, 0, *none, None) == _capi.ARP_E_ARG
    assert L.arp_poses_shortlist_planes_fetch(hd, 4, 0, 0, *none, C.byref(m)) == _capi.ARP_E_ARG
    off = np.full(K + 1, 7, np.uint64)
    assert L.arp_poses_shortlist_planes_fetch(hd, 0, K - 1, 0, _p(off), *none[1:], C.byref(m)) == _capi.ARP_E_CAPACITY and (off == 7).all()
    assert L.arp_poses_shortlist_planes_fetch(hd, 0, K, 0, _p(off), *none[1:], C.byref(m)) == _capi.ARP_OK and _same_bytes(off, tab['pose_off'])
    for slot, key in ((1, 'atom'), (2, 'ring'), (3, 'dist'), (4, 'theta'), (7, 'mask'), (8, 'ctype')):
        buf = np.full(kp, 7, tab[key].dtype)
        args = list(none)
        args[slot] = _p(buf)
        assert L.arp_poses_shortlist_planes_fetch(hd, 0, 0, kp - 1, *args, C.byref(m)) == _capi.ARP_E_CAPACITY and (buf == 7).all()
        assert L.arp_poses_shortlist_planes_fetch(hd, 0, 0, kp, *args, C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, tab[key]), key
    # a launch that did not read the planes result has no planes_summary
    ctx.poses_shortlist('summary', weights=sl.weights(atom_atom={'records': 1}), k=6)
    buf = np.zeros((6, 16), np.uint32)
    args = list(none)
    args[3] = _p(buf)
    assert L.arp_poses_shortlist_fetch(hd, 6, 0, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_ARG and 'did not read' in L.arp_last_error(hd).decode()
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    ctx.poses_summary(x[:9], h[:9], 5.0, 0.1, False)
    ctx.poses_planes_summary(x[:9])
    got = ctx.poses_shortlist('summary', weights=w, k=6, tables=('atom_atom', 'atom_plane'))
    assert _same_bytes(got, want)
    ctx.use_stream(0)                                                 # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------------------------------------------------- GPU: end to end
@pytest.mark.gpu
def test_run_pose_shortlist_end_to_end(tmp_path):
    pc, idx, x, h = hem_case()
    params = (5.0, 0.1, False)
    ic = InteractionComplex(copy.copy(pc))
    full = copy.copy(ic.run_poses(['RESNAME:HEM'], x, h, *params))
    w = mixed_weights(full)
    score = summary_scores(full, w)
    whole = ic.run_pose_shortlist(['RESNAME:HEM'], x, h, *params, k=10, weights=w)
    chunked = ic.run_pose_shortlist(np.asarray(idx), x, h, *params, k=10, weights=w, chunk=32)
    ranked = sl.order(score, 0, 10)
    want = expected(full, ranked, score)
    want['pose'] = want['pose'].astype(np.int64)                      # (the caller's numbering may pass int32)
    assert differences(whole, want) == [] and differences(chunked, want) == [] and ic.pose_shortlist is chunked
    assert len({int(p) // 32 for p in ranked}) > 1                    # the best ten come from more than one chunk
    assert whole['by'] == 'summary' and whole['n_refs'] == 0
    # a filter and a threshold
    got = ic.run_pose_shortlist(['RESNAME:HEM'], x, h, *params, k=70, weights=w, contacts=['hbond', 'hydrophobic'], interacting_entities=['INTER'],
                                min_score=score[ranked[5]], chunk=32)
    chosen = sl.order(score, 0, 70, score[ranked[5]])
    want = expected(full, chosen, score, BIT['hbond'] | BIT['hydrophobic'], INTER)
    want['pose'] = want['pose'].astype(np.int64)
    assert differences(got, want) == [] and 6 <= len(chosen) < 70
    # by Tanimoto: the references ride in front of every chunk
    rx, rh = x[:2], h[:2]
    for chunk in (None, 32):
        got = ic.run_pose_shortlist(['RESNAME:HEM'], x[2:], h[2:], *params, k=8, by='tanimoto', refs_xyz=rx, refs_h_xyz=rh, chunk=chunk)
        f = ic._ctx.poses_contacts(x, h, *params)
        fres = ic._ctx.poses_fingerprints(fp.planes(), n_refs=2)
        ts = sl.tanimoto_q32(fres['count'], fres['cross'], 2, -1)
        chosen = sl.order(ts, 2, 8)
        want = expected(f, chosen, ts)
        want['pose'] = chosen - 2                                     # the caller numbers its poses without the references
        assert differences(got, want) == [], chunk
        assert got['by'] == 'tanimoto' and got['n_refs'] == 2
    # a tie straddling a chunk boundary goes to the lower pose id: pose 40 repeats pose 5
    y, g = x.copy(), h.copy()
    top = int(ranked[0])
    y[5], g[5], y[40], g[40] = x[top], h[top], x[top], h[top]      # the best pose's coordinates in chunk 0 and in chunk 1
    got = ic.run_pose_shortlist(['RESNAME:HEM'], y, g, *params, k=3, weights=w, chunk=32)
    order = got['pose'].tolist()
    assert order.index(5) < order.index(40) and got['score'][order.index(5)] == got['score'][order.index(40)] == score[top]
    table = ic._ctx.poses_contacts(y, g, *params)
    ys = summary_scores(table, w)
    want = expected(table, sl.order(ys, 0, 3), ys)
    want['pose'] = want['pose'].astype(np.int64)
    assert differences(got, want) == []
    with pytest.raises(ValueError):
        ic.run_pose_shortlist(['RESNAME:HEM'], x, h, *params, k=3, by='distance')
    with pytest.raises(ValueError):
        ic.run_pose_shortlist(['RESNAME:HEM'], x, h, *params, k=0)
    # the CSV
    ic.pose_shortlist = whole
    path = ic.write_pose_shortlist(str(tmp_path))
    lines = open(path).read().splitlines()
    assert os.path.basename(path) == 'proteinlike.shortlist' and len(lines) == 1 + len(whole['i'])
    assert lines[0] == 'rank,pose,score,atom_bgn,atom_end,distance,contacts,interacting_entities'
    assert lines[1].startswith(f'0,{int(whole["pose"][0])},{int(whole["score"][0])},')
    ic._ctx.close()
