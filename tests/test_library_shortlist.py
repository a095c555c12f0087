"""Library shortlist (arp_library_shortlist_launch / _fetch / _planes_fetch / _info, Context.library_shortlist,
arpeggio_amd.library_shortlist, InteractionComplex.run_library_shortlist).

The yardstick is never the code under test: Python integers and NumPy over what ``Context.library_contacts``, ``library_planes``
and ``library_fingerprints`` fetch in full (tests/test_ligand_library.py, test_library_planes.py and test_library_fingerprints.py
pin those three to the pose route and the oracle).  ``pose_scores``, ``best_per_ligand``, ``ranked`` and ``expected`` below are this
file's own mirror of score, best-per-ligand, order and record slicing; ``library_shortlist.py`` is checked against it as well.
Every comparison is exact: integers as integers, floats as bytes, dtypes and shapes included.  No tolerance and no time anywhere."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_library_planes as tp
import test_ligand_library as tl
from arpeggio_amd import _capi, synth
from arpeggio_amd import library_fingerprints as lfp
from arpeggio_amd import library_shortlist as lsl
from arpeggio_amd import ligand_library as ll
from arpeggio_amd import pose_shortlist as sl
from arpeggio_amd import poses
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex
from helpers import tiny_complex

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
ALL15 = (1 << 15) - 1
SCATTERED = BIT['vdw'] | BIT['hbond'] | BIT['hydrophobic'] | BIT['weak_polar']
INTER = 1 << CT['INTER']
ONE = 1 << 32
I64_MIN = -(1 << 63)
PARAMS = tl.PARAMS[0]
ENTRIES = ('arp_library_shortlist_launch', 'arp_library_shortlist_fetch', 'arp_library_shortlist_planes_fetch', 'arp_library_shortlist_info')
LIST, SUMMARY, TANIMOTO = 0, 1, 2
POSES, LIGANDS = 0, 1


# ------------------------------------------------------------------------------------------------------------- yardstick
def pose_scores(kind, table=None, w=None, ptable=None, fpr=None, ref=0):
    """The int64 score of every global pose as Python integers: the weighted summary slots of both results, or the Tanimoto
    similarity in 32 fractional bits of row Q + t of a fully fetched library fingerprint."""
    if kind == 'summary':
        s = np.asarray(table['summary']).tolist()
        p = None if ptable is None else np.asarray(ptable['summary']).tolist()
        ww = [int(v) for v in w]
        return [sum(ww[q] * s[t][q] for q in range(16)) + (0 if p is None else sum(ww[16 + q] * p[t][q] for q in range(16))) for t in range(len(s))]
    count, cross = np.asarray(fpr['count']).tolist(), np.asarray(fpr['cross']).tolist()
    Q = int(fpr['n_refs'])
    out = []
    for row in range(Q, len(count)):
        per = []
        for q in (range(Q) if ref < 0 else [ref]):
            x = cross[row][q]
            u = count[row] + count[q] - x
            per.append(ONE if u == 0 else (x << 32) // u)
        out.append(max(per))
    return out


def best_per_ligand(score, lig_off):
    """Per ligand with a pose its best global pose: the highest score, the first of equals."""
    out = []
    for l in range(len(lig_off) - 1):
        best = None
        for t in range(int(lig_off[l]), int(lig_off[l + 1])):
            if best is None or score[t] > score[best]:      # (ascending t: the lower pose keeps a tie)
                best = t
        if best is not None:
            out.append(best)
    return out


def ranked(score, lig_off, unit, k=None, min_score=None):
    cand = best_per_ligand(score, lig_off) if unit == 'ligands' else list(range(len(score)))
    order = sorted(cand, key=lambda t: (-score[t], t))
    if k is not None:
        order = order[:k]
    return [t for t in order if min_score is None or score[t] >= min_score]


def _kept(off, chosen, keep):
    off = np.asarray(off).astype(np.int64).tolist()
    rows, lens = [], []
    for t in chosen:
        r = [q for q in range(off[t], off[t + 1]) if keep(q)]
        rows += r
        lens.append(len(r))
    return np.asarray(rows, np.int64).reshape(-1), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def expected(table, chosen, score, sift_mask=0, ctype_mask=0x7F, ptable=None, tables=('atom_atom',)):
    """What a shortlist of the global poses ``chosen`` (in that order) must hold, from fully fetched tables."""
    chosen = [int(t) for t in chosen]
    idx = np.asarray(chosen, np.int64).reshape(-1)
    want = dict(ligand=ll.ligand_of(table)[idx].astype(np.int32), pose=idx.astype(np.int32),
                score=np.array([int(score[t]) for t in chosen], np.int64).reshape(-1), summary=np.asarray(table['summary'], np.uint32)[idx],
                ligand_pose_off=np.arange(len(chosen) + 1, dtype=np.int64))
    if 'atom_atom' in tables:
        ct, sf = table['ctype'].tolist(), table['sift'].tolist()
        rows, off = _kept(table['pose_off'], chosen, lambda q: (ctype_mask >> ct[q]) & 1 and (sift_mask == 0 or sf[q] & sift_mask))
        want.update({c: np.asarray(table[c])[rows].astype(ll.DTYPES[c]) for c in ll.COLUMNS})
        want['pose_off'] = off
    if ptable is not None:
        want['planes_summary'] = np.asarray(ptable['summary'], np.uint32)[idx]
        for name in tables:
            if name == 'atom_atom':
                continue
            ct = ptable[name]['ctype'].tolist()
            rows, off = _kept(ptable[name]['pose_off'], chosen, lambda q: (ctype_mask >> ct[q]) & 1)
            want[name] = {c: np.asarray(ptable[name][c])[rows].astype(dt) for c, dt in poses.plane_columns(name)}
            want[name]['pose_off'] = off
    return want


def _same_bytes(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bytes(u, v) for u, v in zip(a, b))
    if isinstance(a, (str, int, bool)) or a is None:
        return a == b
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differences(got, want):
    """The keys of ``want`` that ``got`` lacks or holds with another dtype, shape or bytes (sub-tables: 'table.column')."""
    bad = []
    for k, v in want.items():
        if isinstance(v, dict):
            bad += [f'{k}.{c}' for c in differences(got.get(k, {}), v)]
        elif k not in got or not _same_bytes(got[k], v):
            bad.append(k)
    return bad


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def mixed_weights():
    """Weights of both signs on slots that occur."""
    return lsl.weights(atom_atom={'hydrophobic': 50, 'vdw': 30, 'hbond': 400, 'weak_polar': 20, 'proximal': 10, 'records': -15})


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_table():
    """Four ligands with 3, 0, 1 and 2 poses.  Records per global pose: 2, 1, 3, 0, 2, 2.
        pose  record  i  a   sift                 ctype
        0     0       0  0   hbond|proximal       INTER
              1       1  1   hydrophobic|vdw      INTER
        1     2       0  0   hbond|proximal       INTER
        2     3       0  0   proximal             INTER
              4       0  2   hydrophobic|vdw      NON_SELECTION_WATER
              5       1  1   vdw                  INTER
        3     (none)
        4     6       0  3   proximal             NON_SELECTION_WATER
              7       1  4   proximal             NON_SELECTION_WATER
        5     8       0  0   hbond|proximal       INTER
              9       1  1   hydrophobic|vdw      INTER"""
    hp, hv, p_, v_ = BIT['hbond'] | BIT['proximal'], BIT['hydrophobic'] | BIT['vdw'], BIT['proximal'], BIT['vdw']
    other = CT['NON_SELECTION_WATER']
    t = dict(i=np.array([0, 1, 0, 0, 0, 1, 0, 1, 0, 1], np.int32), a=np.array([0, 1, 0, 0, 2, 1, 3, 4, 0, 1], np.int32),
             dist=np.array([2.9, 3.8, 3.0, 4.6, 3.9, 3.7, 4.8, 4.9, 2.9, 3.8], np.float32),
             sift=np.array([hp, hv, hp, p_, hv, v_, p_, p_, hp, hv], np.uint16),
             ctype=np.array([CT['INTER']] * 4 + [other, CT['INTER'], other, other, CT['INTER'], CT['INTER']], np.uint8),
             pose_off=np.array([0, 2, 3, 6, 6, 8, 10], np.uint64), ligand_pose_off=np.array([0, 3, 3, 4, 6], np.int64))
    t['summary'] = np.stack([poses.summarise(s) for s in np.split(t['sift'], t['pose_off'][1:-1].astype(np.int64))])
    return t


def test_the_header_and_the_binding_name_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    for s in ENTRIES:
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    assert '#define ARP_LIBRARY_SHORTLIST_POSES 0' in hdr and '#define ARP_LIBRARY_SHORTLIST_LIGANDS 1' in hdr
    assert (_capi.LIBRARY_SHORTLIST_POSES, _capi.LIBRARY_SHORTLIST_LIGANDS) == (POSES, LIGANDS) and lsl.UNITS == ('poses', 'ligands')
    assert all(hasattr(_capi.Context, m) for m in ('library_shortlist', 'library_shortlist_info'))
    assert all(hasattr(InteractionComplex, m) for m in ('run_library_shortlist', 'write_library_shortlist'))
    # re-exported, not re-implemented
    assert lsl.weights is sl.weights and lsl.tanimoto_q32 is sl.tanimoto_q32 and lsl.take_planes is sl.take_planes and lsl.shift is sl.shift
    assert lsl.KINDS == sl.KINDS and lsl.TABLES == sl.TABLES


def test_ligand_best_with_a_tie_a_ligand_without_poses_and_a_one_pose_ligand():
    lo = [0, 3, 3, 4, 6]
    score = [5, 7, 7, -2, 1, 1]                       # ligand 0: poses 1 and 2 tie; ligand 1 has no pose; ligand 2 has one
    best, best_score = lsl.ligand_best(score, lo)
    assert best.tolist() == [1, -1, 3, 4] and best.dtype == np.int64 and best_score == [7, None, -2, 1]
    assert [t for t in best.tolist() if t >= 0] == best_per_ligand(score, lo)
    big = [1 << 60, (1 << 60) + 1, -(1 << 60), 0, 0, 0]      # Python integers, not floats
    assert lsl.ligand_best(big, lo)[0].tolist() == [1, -1, 3, 4] and lsl.ligand_best(big, lo)[1][0] == (1 << 60) + 1


def test_scores_and_order_for_both_units_with_ties_k_and_min_score():
    t = hand_table()
    lo = t['ligand_pose_off']
    w = lsl.weights(atom_atom={'hbond': 10, 'vdw': -3, 'records': 1})
    score = lsl.scores('summary', t['summary'], None, w)
    assert score == pose_scores('summary', t, w) == [9, 11, -3, 0, 2, 9]
    assert lsl.order(score, lo, 'poses').tolist() == ranked(score, lo, 'poses') == [1, 0, 5, 4, 3, 2]      # 0 and 5 tie across ligands
    assert lsl.order(score, lo, 'ligands').tolist() == ranked(score, lo, 'ligands') == [1, 5, 3]
    assert lsl.order(score, lo, 'ligands').dtype == np.int64
    # k beyond the candidates; min_score equal to a score keeps it
    assert lsl.order(score, lo, 'ligands', k=1000).tolist() == [1, 5, 3] and lsl.order(score, lo, 'poses', k=2).tolist() == [1, 0]
    assert lsl.order(score, lo, 'poses', min_score=9).tolist() == [1, 0, 5] and lsl.order(score, lo, 'poses', min_score=10).tolist() == [1]
    assert lsl.order(score, lo, 'ligands', k=2, min_score=10).tolist() == [1] and lsl.order(score, lo, 'ligands', min_score=12).tolist() == []
    for unit in lsl.UNITS:
        for k in (None, 1, 2, 3, 6, 1000):
            for ms in (None, -3, 0, 9, 10, 11, 12):
                assert lsl.order(score, lo, unit, k, ms).tolist() == ranked(score, lo, unit, k, ms), (unit, k, ms)
    # equal scores everywhere: pure tie order
    assert lsl.order([0] * 6, lo, 'ligands').tolist() == [0, 3, 4] and lsl.order([0] * 6, lo, 'poses').tolist() == list(range(6))
    # Tanimoto: the reference rows are no poses
    fpr = dict(count=np.array([4, 0, 2, 2, 5, 0], np.uint32), cross=np.array([[4, 0], [0, 0], [2, 0], [2, 0], [3, 0], [0, 0]], np.uint32), n_refs=2)
    for ref, want in ((0, [ONE // 2, ONE // 2, ONE // 2, 0]), (1, [0, 0, 0, ONE]), (-1, [ONE // 2, ONE // 2, ONE // 2, ONE])):
        assert lsl.scores('tanimoto', count=fpr['count'], cross=fpr['cross'], n_refs=2, ref=ref) == pose_scores('tanimoto', fpr=fpr, ref=ref) == want
    with pytest.raises(ValueError):
        lsl.order(score, lo, 'molecules')


def test_take_and_take_planes_with_both_masks_and_an_entry_that_keeps_nothing():
    t = hand_table()
    score = [0] * 6
    for ids in ((5, 0, 3, 2), (2, 2), (3,)):
        for sift_mask, ctype_mask in ((0, 0x7F), (BIT['hbond'] | BIT['vdw'], 0x7F), (0, INTER), (BIT['vdw'], 1 << CT['NON_SELECTION_WATER']), (BIT['ionic'], 0x7F)):
            got, want = lsl.take(t, ids, sift_mask, ctype_mask), expected(t, ids, score, sift_mask, ctype_mask)
            del want['score']
            assert differences(got, want) == [], (ids, sift_mask, ctype_mask)
    got = lsl.take(t, (5, 0, 3, 2), BIT['vdw'], 1 << CT['NON_SELECTION_WATER'])
    assert got['pose_off'].tolist() == [0, 0, 0, 0, 1] and got['a'].tolist() == [2] and got['ligand'].tolist() == [3, 0, 2, 0]
    assert got['ligand'].dtype == np.int32 and got['pose'].dtype == np.int32 and np.array_equal(got['summary'], t['summary'][[5, 0, 3, 2]])
    assert [len(per) for per in ll.split(got)] == [1, 1, 1, 1] and ll.split(got)[3][0]['a'].tolist() == [2]      # a library table of K entries
    # planes: the hand-made tables of three poses, one record given another type by hand
    _, pt = tp.hand_planes()
    pt['atom_plane']['ctype'] = np.array([CT['INTER'], CT['INTER'], CT['NON_SELECTION_WATER']], np.uint8)
    T = len(pt['summary'])
    ids = list(range(T - 1, -1, -1)) + [0]
    for ctype_mask in (0x7F, INTER, 1 << CT['NON_SELECTION_WATER'], 1 << CT['INTRA_SELECTION']):
        got = lsl.take_planes(pt, ids, ctype_mask)
        lo = dict(pt, ligand_pose_off=np.arange(T + 1))
        want = expected(dict(summary=pt['summary'], ligand_pose_off=np.arange(T + 1)), ids, [0] * T, 0, ctype_mask, lo, tables=poses.PLANE_TABLES)
        assert differences(got, {n: want[n] for n in poses.PLANE_TABLES}) == [] and np.array_equal(got['summary'], want['planes_summary'])


def _short_of(t, ids, score, base=0):
    s = lsl.take(t, ids)
    s['score'] = np.array([score[p] for p in ids], np.int64)
    return lsl.shift(s, base)


def test_merge_for_ligands_cut_between_chunks_and_k_beyond_what_there_is():
    t = hand_table()
    score = [9, 11, -3, 0, 2, 9]
    # chunk A holds global poses 0 ... 1, chunk B poses 2 ... 5: ligand 0 is cut, its better pose (1) is in ... A; then turned round
    a, b = _short_of(t, [1], score), _short_of(t, [5, 3, 2], score)
    m = lsl.merge([a, b], 3, 'ligands')
    assert m['pose'].tolist() == [1, 5, 3] and m['ligand'].tolist() == [0, 3, 2] and m['score'].tolist() == [11, 9, 0]
    want = expected(t, [1, 5, 3], score)
    want['pose'] = want['pose'].astype(np.int64)
    assert differences(m, want) == []
    # the better pose of the cut ligand is in the SECOND chunk
    score2 = [9, 3, 11, 0, 2, 9]
    m = lsl.merge([_short_of(t, [0], score2), _short_of(t, [2, 5, 3], score2)], 2, 'ligands')
    assert m['pose'].tolist() == [2, 5] and m['ligand'].tolist() == [0, 3] and m['pose_off'].tolist() == [0, 3, 5]
    # an equal score in both: the lower global pose wins, BEFORE the best k are taken (k = 1 must not see ligand 0 twice)
    score3 = [9, 3, 9, 0, 2, 9]
    m = lsl.merge([_short_of(t, [0], score3), _short_of(t, [2, 5, 3], score3)], 2, 'ligands')
    assert m['pose'].tolist() == [0, 5] and m['ligand'].tolist() == [0, 3]
    # unit poses keeps both entries of the ligand
    m = lsl.merge([_short_of(t, [0], score3), _short_of(t, [2, 5, 3], score3)], 3, 'poses')
    assert m['pose'].tolist() == [0, 2, 5] and m['ligand'].tolist() == [0, 0, 3]
    # k beyond what there is; chunk-local ids shifted to global ones
    m = lsl.merge([_short_of(t, [0], score3), _short_of(dict(t), [2, 5, 3], score3)], 1000, 'ligands')
    assert m['pose'].tolist() == [0, 5, 3] and m['ligand_pose_off'].tolist() == [0, 1, 2, 3]
    assert lsl.shift(a, 40)['pose'].tolist() == [41] and lsl.shift(a, 40)['ligand'].tolist() == [0]
    with pytest.raises(ValueError):
        lsl.merge([a], 1, 'molecules')


def test_records_and_the_csv_text(tmp_path):
    rec, ligs, _ = tl.case_main()
    t = hand_table()
    short = _short_of(t, [5, 3, 0], [9, 11, -3, 0, 2, 7])
    assert short['ligand'].tolist() == [3, 2, 0]
    four = [ligs[2], ligs[3], ligs[4], ligs[5]]       # ligands of at least five atoms
    recs = lsl.to_records(short, rec, four)
    assert [(r['rank'], r['ligand'], r['pose'], r['score']) for r in recs] == [(0, 3, 5, 7), (0, 3, 5, 7), (2, 0, 0, 9), (2, 0, 0, 9)]
    plain = ll.to_records(t, rec, four)
    assert [r['bgn'] for r in recs] == [plain[q]['bgn'] for q in (8, 9, 0, 1)] and [r['end'] for r in recs] == [plain[q]['end'] for q in (8, 9, 0, 1)]
    assert recs[0]['contact'] == ['proximal', 'hbond'] and recs[0]['interacting_entities'] == 'INTER' and recs[0]['type'] == 'atom-atom'
    path = lsl.write_library_shortlist(str(tmp_path), 'x', short, rec, four)
    assert path.endswith('x.libraryshortlist')
    lines = open(path).read().splitlines()
    assert lines[0] == 'rank,ligand,pose,score,atom_bgn,atom_end,distance,contacts,interacting_entities' and len(lines) == 5
    ll.write_csv(str(tmp_path / 'full.csv'), t, rec, four)
    full = open(tmp_path / 'full.csv').read().splitlines()
    assert lines[1] == '0,3,5,7,' + full[9].split(',', 2)[2] and lines[3] == '2,0,0,9,' + full[1].split(',', 2)[2]
    assert lines[1].endswith('proximal|hbond,INTER')


# ------------------------------------------------------------------------------------------------------------- GPU: contents
def _ctx(pc):
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    return ctx


def main_launch():
    rec, ligs, ps = tl.case_main()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    return rec, ligs, ps, lib, ctx, tl.launch(ctx, lib, ps)


@pytest.mark.gpu
def test_main_case_both_units_by_summary_against_the_mirror_and_library_best():
    rec, ligs, ps, lib, ctx, table = main_launch()
    lo = table['ligand_pose_off']
    assert np.diff(lo).tolist() == list(tl.MAIN_P)
    for w in (mixed_weights(), np.zeros(32, np.int32)):      # both signs; all zero: pure tie order
        score = pose_scores('summary', table, w)
        assert lsl.scores('summary', table['summary'], None, w) == score
        assert not any(w) or (min(score) < 0 < max(score))
        for unit in lsl.UNITS:
            for k in (1, 5, 6, 7, 1000):
                chosen = ranked(score, lo, unit, k)
                assert lsl.order(score, lo, unit, k).tolist() == chosen
                got = ctx.library_shortlist('summary', unit=unit, weights=w, k=k)
                assert differences(got, expected(table, chosen, score)) == [], (unit, k)
                assert len(chosen) == (min(k, 6) if unit == 'ligands' else min(k, 82))      # the pose-less ligand never counts
                assert 3 not in got['ligand'].tolist() and got['unit'] == unit and got['kind'] == 'summary'
                info = ctx.library_shortlist_info()
                assert (info['chosen'], info['atom_atom'], info['kind'], info['unit']) == (len(chosen), len(got['i']), SUMMARY, lsl.UNITS.index(unit))
        # unit ligands with first-half weights: what library_best gives, from another kernel
        best = ctx.library_best(w[:16])
        got = ctx.library_shortlist('summary', unit='ligands', weights=w, k=1000, tables=('atom_atom',))
        assert np.array_equal(got['pose'], best['best_pose'][got['ligand']]) and np.array_equal(got['score'], best['score'][got['ligand']])
        assert sorted(got['ligand'].tolist()) == [0, 1, 2, 4, 5, 6]
    # a library table of K entries: split gives one pose per entry
    got = ctx.library_shortlist('summary', unit='ligands', weights=mixed_weights(), k=3)
    per = ll.split(got)
    off = table['pose_off'].astype(np.int64)
    assert [len(x) for x in per] == [1, 1, 1] and all(np.array_equal(per[r][0]['a'], table['a'][off[t]:off[t + 1]]) for r, t in enumerate(got['pose'].tolist()))
    assert len(lsl.to_records(got, rec, ligs)) == len(got['i'])
    ctx.close()


def one_atom_receptor():
    """A receptor of one 10-atom cluster on a 4 A sphere about the origin (and an atom far away): a one-atom ligand at the origin
    has ten records, one 100 A away none."""
    k = np.arange(10) + 0.5
    phi, th = np.arccos(1.0 - 2.0 * k / 10), np.pi * (1.0 + 5.0 ** 0.5) * k
    atoms = 4.0 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    return tiny_complex(np.concatenate([atoms, [[0.0, -200.0, 0.0]]]))


def _one_atom_poses(points):
    return np.asarray(points, np.float32).reshape(-1, 1, 3), np.zeros((len(points), 0, 3))


@functools.lru_cache(maxsize=None)
def argmax_case():
    """One-atom ligands of 0, 1, 63, 0, 64, 65, 130 and 0 poses: pose-less ligands first, in the middle and last.  A pose at
    the origin has ten records, one far away none.  Ligand 2 (63): random near poses.  Ligand 4 (64): all
    far but a few near ones.  Ligand 5 (65): every pose far away but the LAST — its unique best is the second pose of lane 0.
    Ligand 6 (130): IDENTICAL poses, a tie across all lanes and across a lane's stride of three."""
    rng = np.random.default_rng(5)
    far = np.array([0.0, 100.0, 0.0])
    near = lambda n: rng.normal(size=(n, 3)) * 1.2      # (off the centre: other atoms within the cutoff, other contacts)
    l4 = np.tile(far, (64, 1))
    l4[[7, 40, 63]] = near(3)
    l5 = np.tile(far, (65, 1))
    l5[64] = [0.1, 0.0, 0.0]
    pts = [None, near(1), near(63), None, l4, l5, np.tile([0.2, 0.1, 0.0], (130, 1)), None]
    ligs = tuple(synth.ligand('ion', 10 + q) for q in range(len(pts)))
    return one_atom_receptor(), ligs, [None if p is None else _one_atom_poses(p) for p in pts]


@pytest.mark.gpu
def test_the_segmented_arg_max_on_its_seams():
    rec, ligs, ps = argmax_case()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    table = tl.launch(ctx, lib, ps)
    lo = table['ligand_pose_off']
    assert np.diff(lo).tolist() == [0, 1, 63, 0, 64, 65, 130, 0]
    n = np.diff(table['pose_off'].astype(np.int64))
    assert n[int(lo[5]):int(lo[6])].tolist() == [0] * 64 + [10] and len(set(n[int(lo[6]):].tolist())) == 1 and n[-1] == 10      # the conditions, on the yardstick
    for w in (lsl.weights(atom_atom={'records': 1}), lsl.weights(atom_atom={'records': -1}), lsl.weights(atom_atom={'proximal': 3, 'vdw': -2, 'records': 1})):
        score = pose_scores('summary', table, w)
        for unit, k in (('ligands', 1000), ('ligands', 3), ('ligands', 5), ('poses', 1000), ('poses', 64), ('poses', 65)):
            chosen = ranked(score, lo, unit, k)
            got = ctx.library_shortlist('summary', unit=unit, weights=w, k=k)
            assert differences(got, expected(table, chosen, score)) == [], (unit, k)
        got = ctx.library_shortlist('summary', unit='ligands', weights=w, k=1000)
        assert sorted(got['ligand'].tolist()) == [1, 2, 4, 5, 6] and len(got['pose']) == 5
        entry = dict(zip(got['ligand'].tolist(), got['pose'].tolist()))
        assert entry[6] == int(lo[6])                                # identical poses: the first
        assert w[15] < 0 or entry[5] == int(lo[6]) - 1               # the unique best is the last pose
    ctx.close()


@pytest.mark.gpu
def test_more_ligands_than_a_block_has_waves_and_than_one_scan_round():
    rec = tl.receptor()
    L = 1030
    ligs = synth.ligands(L, seed=3, kinds=('ion',))
    assert all(lig.n_atoms == 1 for lig in ligs)
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    rng = np.random.default_rng(11)
    ps = [_one_atom_poses(centre + rng.normal(size=(1, 3)) * 6.0) for _ in range(L)]
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    table = tl.launch(ctx, lib, ps)
    lo = table['ligand_pose_off']
    w = lsl.weights(atom_atom={'records': 1, 'vdw': 7})
    score = pose_scores('summary', table, w)
    assert len(set(score)) < L                                        # ties among the 1 030
    for k in (1030, 3):
        for unit in lsl.UNITS:
            chosen = ranked(score, lo, unit, k)
            got = ctx.library_shortlist('summary', unit=unit, weights=w, k=k, sift_mask=SCATTERED)
            assert differences(got, expected(table, chosen, score, SCATTERED)) == [], (unit, k)
            assert len(got['pose']) == k and np.array_equal(got['ligand'], got['pose'])      # one pose each: ligand l is pose l
    ctx.close()


@pytest.mark.gpu
def test_tanimoto_with_one_reference_all_and_an_empty_one():
    rec, ligs, ps = argmax_case()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    table = tl.launch(ctx, lib, ps)
    lo = table['ligand_pose_off']
    near = int(lo[6])
    refs = lfp.references([lfp.reference_from_pose(table, near, level='atom'), {}])
    fpr = ctx.library_fingerprints(refs, ALL15, by_residue=False)
    assert fpr['count'][1] == 0 and fpr['count'][0] > 0
    for ref in (0, 1, -1):
        score = pose_scores('tanimoto', fpr=fpr, ref=ref)
        assert lsl.scores('tanimoto', count=fpr['count'], cross=fpr['cross'], n_refs=2, ref=ref) == score
        for unit, k in (('poses', 1000), ('poses', 70), ('ligands', 1000), ('ligands', 2)):
            chosen = ranked(score, lo, unit, k)
            got = ctx.library_shortlist('tanimoto', unit=unit, ref=ref, k=k)
            assert differences(got, expected(table, chosen, score)) == [], (ref, unit, k)
        if ref == 1:      # a pose without features against the empty reference: 0 / 0 ranks first with 2^32
            got = ctx.library_shortlist('tanimoto', unit='poses', ref=ref, k=1)
            assert got['score'].tolist() == [ONE] and got['pose'].tolist() == [int(lo[4])] and len(got['i']) == 0
        if ref == -1:     # ... and ties there with the poses that have exactly the first reference's features
            ones = [t for t in range(len(score)) if score[t] == ONE]
            assert int(lo[4]) in ones and near in ones and ranked(score, lo, 'poses', 1) == [ones[0]]
    # the scores are taken at launch: a later fingerprint launch leaves the shortlist as it is
    before = _resident(ctx)
    ctx.library_fingerprints(lfp.references([{}]), BIT['hbond'], by_residue=False)
    assert before[0] == _capi.ARP_OK and _same_resident(_resident(ctx), before)
    ctx.close()


@pytest.mark.gpu
def test_tanimoto_on_the_main_case_equals_library_fingerprints_best():
    rec, ligs, ps, lib, ctx, table = main_launch()
    lo = table['ligand_pose_off']
    refs = lfp.references([lfp.reference_from_pose(table, int(lo[2]), rec.res_id)])
    planes = ALL15 & ~BIT['proximal']
    fpr = ctx.library_fingerprints(refs, planes)
    best = ctx.library_fingerprints_best()
    score = pose_scores('tanimoto', fpr=fpr, ref=0)
    got = ctx.library_shortlist('tanimoto', unit='ligands', ref=0, k=1000)
    assert differences(got, expected(table, ranked(score, lo, 'ligands'), score)) == []
    assert np.array_equal(got['pose'], best['best_pose'][got['ligand'], 0]) and np.array_equal(got['score'], best['tanimoto_q32'][got['ligand'], 0])
    assert got['pose'][0] == int(lo[2]) and got['score'][0] == ONE
    for ref in (0, -1):
        got = ctx.library_shortlist('tanimoto', unit='poses', ref=ref, k=9, sift_mask=SCATTERED, ctype_mask=INTER)
        assert differences(got, expected(table, ranked(score, lo, 'poses', 9), score, SCATTERED, INTER)) == []
    ctx.close()


@pytest.mark.gpu
def test_min_score_between_two_scores_equal_to_one_and_above_the_best():
    rec, ligs, ps, lib, ctx, table = main_launch()
    lo = table['ligand_pose_off']
    w = mixed_weights()
    score = pose_scores('summary', table, w)
    for unit in lsl.UNITS:
        cand = ranked(score, lo, unit)
        s = [score[t] for t in cand]
        distinct = sorted(set(s), reverse=True)
        assert len(distinct) >= 3
        for ms, kept in ((distinct[1], sum(v >= distinct[1] for v in s)), (distinct[1] + 1, sum(v > distinct[1] for v in s)),
                         ((distinct[1] + distinct[2]) // 2 if distinct[1] - distinct[2] > 1 else distinct[1], None), (distinct[0] + 1, 0)):
            for k in (1000, 4):
                chosen = ranked(score, lo, unit, k, ms)
                got = ctx.library_shortlist('summary', unit=unit, weights=w, k=k, min_score=ms)
                assert differences(got, expected(table, chosen, score)) == [], (unit, ms, k)
                assert kept is None or len(chosen) == min(kept, k)
    # above the best: K = 0, fetched with cap_entries = 0
    got = ctx.library_shortlist('summary', unit='ligands', weights=w, k=5, min_score=max(score) + 1)
    assert len(got['pose']) == 0 and got['pose_off'].tolist() == [0] and ctx.library_shortlist_info()['chosen'] == 0
    n, m = C.c_int64(-1), C.c_int64(-1)
    off = np.full(1, 7, np.uint64)
    empty = np.zeros(0, np.int32)
    assert ctx._L.arp_library_shortlist_fetch(ctx._h, 0, 0, _p(empty), _p(empty), None, None, None, _p(off), None, None, None, None, None,
                                              C.byref(n), C.byref(m)) == _capi.ARP_OK and (n.value, m.value, off.tolist()) == (0, 0, [0])
    ctx.close()


@functools.lru_cache(maxsize=None)
def seam_case():
    """Three clusters of 63, 64 and 65 receptor atoms on 4 A spheres about centres 40 A apart; four one-atom ligands with poses
    at the centres and 100 A away: record segments of 63, 64, 65 and 0."""
    def sphere(n):
        k = np.arange(n) + 0.5
        phi, th = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
        return 4.0 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    centres = np.array([[0.0, 0.0, 0.0], [40.0, 0.0, 0.0], [80.0, 0.0, 0.0]])
    atoms = np.concatenate([centres[c] + sphere(n) for c, n in enumerate((63, 64, 65))])
    pc = tiny_complex(np.concatenate([atoms, [[0.0, -200.0, 0.0]]]))
    ligs = tuple(synth.ligand('ion', 20 + q) for q in range(3))
    ps = [_one_atom_poses(centres[:2]), _one_atom_poses([centres[2], [0.0, 100.0, 0.0]]), None]
    return pc, ligs, ps


@pytest.mark.gpu
def test_lists_and_segment_lengths_on_the_wave_seam():
    pc, ligs, ps = seam_case()
    lib = ll.pack(ligs)
    ctx = _ctx(pc)
    ctx.set_ligand_library(lib)
    table = tl.launch(ctx, lib, ps)
    assert np.diff(table['pose_off'].astype(np.int64)).tolist() == [63, 64, 65, 0]      # the condition, on the yardstick
    for ids in ((2, 0, 3, 1), (3,), (1, 1, 2)):
        got = ctx.library_shortlist('list', pose_ids=ids)
        assert differences(got, expected(table, ids, [0] * 4)) == [], ids
        assert got['pose'].tolist() == list(ids) and not got['score'].any() and got['unit'] == 'poses'
        assert got['ligand'].tolist() == [[0, 0, 1, 1][t] for t in ids] and ctx.library_shortlist_info()['kind'] == LIST
    w = lsl.weights(atom_atom={'records': 1})
    score = pose_scores('summary', table, w)
    got = ctx.library_shortlist('summary', unit='poses', weights=w, k=4)
    assert got['pose'].tolist() == [2, 1, 0, 3] and got['pose_off'].tolist() == [0, 65, 129, 192, 192]
    assert differences(got, expected(table, [2, 1, 0, 3], score)) == []
    got = ctx.library_shortlist('summary', unit='ligands', weights=w, k=4)
    assert got['pose'].tolist() == [2, 1] and got['ligand'].tolist() == [1, 0] and got['pose_off'].tolist() == [0, 65, 129]
    # a filter that keeps everything takes the counting path over the same seams; one that keeps nothing leaves empty entries
    every = int(np.bitwise_and.reduce(table['sift']))
    assert every != 0
    for sift_mask, ctype_mask in ((ALL15, 0x7F), (every, 0x7F), (every, INTER), (0, INTER)):
        got = ctx.library_shortlist('list', pose_ids=(1, 2, 0, 3), sift_mask=sift_mask, ctype_mask=ctype_mask)
        want = expected(table, (1, 2, 0, 3), [0] * 4, sift_mask, ctype_mask)
        assert differences(got, want) == [] and want['pose_off'].tolist() == [0, 64, 129, 192, 192], (sift_mask, ctype_mask)
    none = ALL15 & ~int(np.bitwise_or.reduce(table['sift']))
    got = ctx.library_shortlist('list', pose_ids=(1, 2), sift_mask=none)
    assert differences(got, expected(table, (1, 2), [0] * 4, none)) == [] and got['pose_off'].tolist() == [0, 0, 0]
    ctx.close()


@pytest.mark.gpu
def test_the_record_filter_on_the_main_case():
    rec, ligs, ps, lib, ctx, table = main_launch()
    lo = table['ligand_pose_off']
    w = mixed_weights()
    score = pose_scores('summary', table, w)
    water = 1 << CT['SELECTION_WATER']
    assert ((table['ctype'] == CT['SELECTION_WATER']).any() and (table['ctype'] == CT['INTER']).any())
    nothing = 0
    for sift_mask, ctype_mask in ((SCATTERED, 0x7F), (0, INTER), (SCATTERED, INTER), (0, water), (BIT['hbond'], water)):
        for unit, k in (('ligands', 6), ('poses', 20)):
            chosen = ranked(score, lo, unit, k)
            want = expected(table, chosen, score, sift_mask, ctype_mask)
            got = ctx.library_shortlist('summary', unit=unit, weights=w, k=k, sift_mask=sift_mask, ctype_mask=ctype_mask)
            assert differences(got, want) == [], (sift_mask, ctype_mask, unit)
            assert len(want['i']) < int(sum(int(table['pose_off'][t + 1]) - int(table['pose_off'][t]) for t in chosen))      # the filter drops records
            assert np.array_equal(got['summary'], table['summary'][chosen])                                             # the rows stay the unfiltered ones
            nothing += int((np.diff(want['pose_off'].astype(np.int64)) == 0).sum())
    assert nothing > 0                                                                                                   # an entry that keeps nothing
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: planes
def planes_launch(case):
    rec, ligs, ps = case()
    ctx, lib = tp.library_ctx(tp.device_planes(rec), ligs)
    table = tl.launch(ctx, lib, ps)
    return rec, ligs, ps, lib, ctx, table, tp.launch(ctx, lib, ps)


@pytest.mark.gpu
@pytest.mark.parametrize('case', (tp.case_main, tp.case_docked), ids=('main', 'docked'))
def test_the_planes_tables_weights_and_summary_rows(case):
    rec, ligs, ps, lib, ctx, table, ptable = planes_launch(case)
    lo = table['ligand_pose_off']
    assert sum(len(ptable[n]['ctype']) for n in poses.PLANE_TABLES) > 0 and len(ptable['group_group']['ctype']) + len(ptable['atom_plane']['ctype']) > 0
    w = lsl.weights(atom_atom={'records': 1, 'hbond': -40}, planes={'atom_plane': 100, 'plane_plane': -250, 'group_plane': 30})
    alone = lsl.weights(planes={'atom_plane': 1})                      # a weight on a planes slot alone
    for ww in (w, alone):
        score = pose_scores('summary', table, ww, ptable)
        assert lsl.scores('summary', table['summary'], ptable['summary'], ww) == score and any(score)
        for unit in lsl.UNITS:
            for ctype_mask in (0x7F, INTER):                            # (INTER alone is a partial mask: water and intra records go)
                chosen = ranked(score, lo, unit, 6)
                got = ctx.library_shortlist('summary', unit=unit, weights=ww, k=6, tables=lsl.TABLES, ctype_mask=ctype_mask)
                want = expected(table, chosen, score, 0, ctype_mask, ptable, lsl.TABLES)
                assert differences(got, want) == [], (unit, ctype_mask)
                assert got['group_group']['dist'].dtype == np.float32 and got['group_group']['dist'].tobytes() == want['group_group']['dist'].tobytes()
    # tables without bit 0: no atom-atom column, the ring / amide tables alone
    score = pose_scores('summary', table, w, ptable)
    chosen = ranked(score, lo, 'poses', 4)
    got = ctx.library_shortlist('summary', unit='poses', weights=w, k=4, tables=('plane_plane', 'group_group'))
    want = expected(table, chosen, score, 0, 0x7F, ptable, ('plane_plane', 'group_group'))
    assert differences(got, want) == [] and 'i' not in got and 'pose_off' not in got and 'atom_plane' not in got
    assert np.array_equal(got['planes_summary'], ptable['summary'][chosen])
    n, m = C.c_int64(0), C.c_int64(0)
    off = np.zeros(5, np.uint64)
    assert ctx._L.arp_library_shortlist_fetch(ctx._h, 4, 0, None, None, None, None, None, _p(off), None, None, None, None, None, C.byref(n),
                                              C.byref(m)) == _capi.ARP_E_ARG and 'was not requested' in ctx._L.arp_last_error(ctx._h).decode()
    # the weight on a planes slot alone reads the planes result although only the atom-atom table is fetched
    got = ctx.library_shortlist('summary', unit='ligands', weights=alone, k=3)
    sc = pose_scores('summary', table, alone, ptable)
    assert differences(got, dict(expected(table, ranked(sc, lo, 'ligands', 3), sc), planes_summary=ptable['summary'][ranked(sc, lo, 'ligands', 3)])) == []
    # a list over all five tables
    ids = [int(lo[-1]) - 1, 0, 0]
    got = ctx.library_shortlist('list', pose_ids=ids, tables=lsl.TABLES, ctype_mask=INTER)
    assert differences(got, expected(table, ids, [0] * int(lo[-1]), 0, INTER, ptable, lsl.TABLES)) == []
    assert differences(lsl.take_planes(ptable, ids, INTER), {n: expected(table, ids, [0] * int(lo[-1]), 0, INTER, ptable, lsl.TABLES)[n] for n in poses.PLANE_TABLES}) == []
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: protocol
def _launch(ctx, kind=SUMMARY, unit=LIGANDS, weights=None, ref=0, ids=None, k=5, min_score=I64_MIN, tables=1, sift_mask=0, ctype_mask=0x7F, n_ids=None):
    info = np.zeros(8, np.int64)
    w = None if weights is None else np.ascontiguousarray(weights, np.int32)
    i = None if ids is None else np.ascontiguousarray(ids, np.int32)
    rc = ctx._L.arp_library_shortlist_launch(ctx._h, kind, unit, _p(w), ref, _p(i), (0 if i is None else len(i)) if n_ids is None else n_ids, k, min_score,
                                             tables, sift_mask, ctype_mask, _p(info))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), info


def _same_resident(a, b):
    return a[0] == b[0] and _same_bytes(a[2], b[2])


def _resident(ctx, planes=False):
    """The resident library shortlist, fetched without a launch: (rc, message, arrays)."""
    info = ctx.library_shortlist_info()
    K, k = info['chosen'], info['atom_atom']
    out = dict(ligand=np.empty(K, np.int32), pose=np.empty(K, np.int32), score=np.empty(K, np.int64), summary=np.empty((K, 16), np.uint32),
               off=np.empty(K + 1, np.uint64), i=np.empty(k, np.int32), a=np.empty(k, np.int32), dist=np.empty(k, np.float32), sift=np.empty(k, np.uint16),
               ctype=np.empty(k, np.uint8))
    if planes:
        out['planes_summary'] = np.empty((K, 16), np.uint32)
    n, m = C.c_int64(-1), C.c_int64(-1)
    rc = ctx._L.arp_library_shortlist_fetch(ctx._h, K, k, _p(out['ligand']), _p(out['pose']), _p(out['score']), _p(out['summary']), _p(out.get('planes_summary')),
                                            _p(out['off']), _p(out['i']), _p(out['a']), _p(out['dist']), _p(out['sift']), _p(out['ctype']), C.byref(n), C.byref(m))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), out


def _moved_pose(ps):
    """The poses of ``tp.case_main`` with the last pose of ligand 0 handed to ligand 1 (both one atom, no hydrogen rows in xyz): T and
    the coordinate count stay, the per-ligand pose ranges do not."""
    out = list(ps)
    x0, x1 = ps[0][0], ps[1][0]
    out[0] = (x0[:-1], ps[0][1][:-1])
    out[1] = (np.concatenate([x0[-1:], x1]), None)
    return out


@pytest.mark.gpu
def test_every_refusal_names_its_cause_in_order_and_touches_nothing():
    rec, ligs, ps = tp.case_main()
    ctx, lib = tp.library_ctx(tp.device_planes(rec), ligs)
    w = mixed_weights()
    rc, msg, _ = _launch(ctx, weights=w)
    assert rc == _capi.ARP_E_ARG and 'no library result' in msg
    table = tl.launch(ctx, lib, ps)
    T = int(table['ligand_pose_off'][-1])
    good = ctx.library_shortlist('summary', weights=w, k=5, sift_mask=SCATTERED)
    launches = ctx.library_shortlist_info()
    before = _resident(ctx)
    assert before[0] == _capi.ARP_OK and np.array_equal(before[2]['pose'], good['pose']) and len(before[2]['i']) > 0
    wp = w.copy()
    wp[16] = 1
    big = w.copy()
    big[3] = (1 << 24) + 1
    bad = dict(kind=dict(kind=3), unit=dict(unit=2), tables=dict(tables=0), ids=dict(kind=LIST, unit=POSES, k=0), k=dict(k=0), weights=dict(weights=None),
               tanimoto=dict(kind=TANIMOTO), planes=dict(tables=3))

    def refused(word, code=_capi.ARP_E_ARG, **kw):
        kw.setdefault('weights', w)
        rc, msg, _ = _launch(ctx, **kw)
        assert rc == code and word in msg, (word, rc, msg)
    refused('unknown kind', kind=3)
    refused('unknown kind', kind=-1)
    refused('unknown unit', unit=2)
    refused('unknown unit', unit=-1)
    refused('tables must be', tables=0)
    refused('tables must be', tables=32)
    refused('sift_mask has bits beyond', sift_mask=1 << 15)
    refused('ctype_mask has bits beyond', ctype_mask=0x80)
    refused('ctype_mask of 0', ctype_mask=0)
    refused('pose_ids missing', kind=LIST, unit=POSES, k=0)
    refused('n_ids', kind=LIST, unit=POSES, k=0, ids=[0], n_ids=0)
    refused('n_ids', kind=LIST, unit=POSES, k=0, ids=[0], n_ids=(1 << 20) + 1)
    refused('pose_ids has an id outside', kind=LIST, unit=POSES, k=0, ids=[0, T])
    refused('pose_ids has an id outside', kind=LIST, unit=POSES, k=0, ids=[-1])
    refused('ARP_SHORTLIST_LIST takes unit', kind=LIST, unit=LIGANDS, k=0, ids=[0])
    refused('ARP_SHORTLIST_LIST takes unit', kind=LIST, unit=POSES, k=1, ids=[0])
    refused('ARP_SHORTLIST_LIST takes unit', kind=LIST, unit=POSES, k=0, min_score=0, ids=[0])
    refused('k must be at least 1', k=0)
    refused('weights missing', weights=None)
    refused('weights has an entry beyond', weights=big)
    refused('weights has an entry beyond', weights=-big)
    refused('no library fingerprint', kind=TANIMOTO)
    refused('no library-planes result', tables=3)
    refused('no library-planes result', weights=wp)
    # the documented order: of two causes the earlier one is named
    order = ('kind', 'unit', 'tables', 'ids', 'k', 'weights', 'tanimoto', 'planes')
    words = dict(kind='unknown kind', unit='unknown unit', tables='tables must be', ids='pose_ids missing', k='k must be at least 1',
                 weights='weights missing', tanimoto='no library fingerprint', planes='no library-planes result')
    for a, first in enumerate(order):
        for second in order[a + 1:]:
            if (first, second) == ('weights', 'tanimoto'):
                continue                                            # (two causes that need different kinds cannot be combined)
            kw = dict(bad[second])
            kw.update(bad[first])
            refused(words[first], **kw)
    ctx.run_enqueue(5.0, 0.1, False)
    refused('not been waited for', kind=3)                          # before everything else
    ctx.run_wait()
    ctx.library_fingerprints(None, ALL15)
    refused('no references', kind=TANIMOTO)
    ctx.library_fingerprints(lfp.references([{}, {}]), ALL15)
    refused('ref must be', kind=TANIMOTO, ref=2)
    refused('ref must be', kind=TANIMOTO, ref=-2)
    refused('no library-planes result', kind=TANIMOTO, ref=1, tables=2)
    # the same-poses refusals: other ligands' pose ranges with the same T and the same number of coordinates
    moved = _moved_pose(ps)
    off_m, x_m, _ = ll.flatten_poses(lib, moved)
    off, x, _ = ll.flatten_poses(lib, ps)
    assert off_m[-1] == off[-1] and len(x_m) == len(x) and off_m.tolist() != off.tolist()
    ctx.library_planes_summary(off_m, x_m)
    refused('differ in ligands, poses or pose ranges', tables=2)
    refused('differ in ligands, poses or pose ranges', weights=wp)
    fewer = [p if q != 4 else (p[0][:-1], p[1][:-1]) for q, p in enumerate(ps)]
    off_f, x_f, _ = ll.flatten_poses(lib, fewer)
    ctx.library_planes_summary(off_f, x_f)
    refused('differ in ligands, poses or pose ranges', tables=2)
    # none of them touched the resident shortlist
    assert ctx.library_shortlist_info() == launches and _same_resident(_resident(ctx), before)
    assert ctx._L.arp_library_shortlist_launch(None, 1, 1, _p(w), 0, None, 0, 5, I64_MIN, 1, 0, 0x7F, _p(np.zeros(8, np.int64))) == _capi.ARP_E_ARG
    assert ctx._L.arp_library_shortlist_launch(ctx._h, 1, 1, _p(w), 0, None, 0, 5, I64_MIN, 1, 0, 0x7F, None) == _capi.ARP_E_ARG
    assert ctx.library_shortlist_info() == launches and _same_resident(_resident(ctx), before)
    # made from different poses — one float, one ulp —: found on the device, no shortlist is left
    other = x.copy()
    other[len(other) // 2] = np.nextafter(other[len(other) // 2], np.float32(np.inf))
    assert int((other.view(np.uint32) != x.view(np.uint32)).sum()) == 1
    ctx.library_planes_summary(off, other)
    rc, msg, _ = _launch(ctx, weights=w, tables=3)
    assert rc == _capi.ARP_E_ARG and 'made from different poses' in msg
    rc, msg, _ = _resident(ctx)
    assert rc == _capi.ARP_E_ARG and 'no result' in msg and ctx.library_shortlist_info()['chosen'] == 0
    # ... and the same poses are accepted
    ctx.library_planes_summary(off, x)
    assert _launch(ctx, weights=w, tables=3)[0] == _capi.ARP_OK and _resident(ctx, planes=True)[0] == _capi.ARP_OK
    ctx.close()


@pytest.mark.gpu
def test_the_shortlist_goes_with_its_sources_and_with_nothing_else():
    rec, ligs, ps = tp.case_main()
    rec_gpu = tp.device_planes(rec)
    ctx, lib = tp.library_ctx(rec_gpu, ligs)
    w = mixed_weights()
    off, x, h = ll.flatten_poses(lib, ps)
    none = dict(chosen=0, atom_atom=0, atom_plane=0, plane_plane=0, group_group=0, group_plane=0, launches=0, kind=0, unit=0)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and 'no result' in _resident(ctx)[1] and ctx.library_shortlist_info() == none
    table = ctx.library_contacts(off, x, h, *PARAMS)
    first = ctx.library_shortlist('summary', weights=w, k=5)
    second = ctx.library_shortlist('list', pose_ids=[8, 1])          # a repeated launch with other arguments remakes the result
    assert ctx.library_shortlist_info()['launches'] == 2 and differences(second, expected(table, [8, 1], [0] * 16)) == []
    assert _same_bytes(ctx.library_shortlist('summary', weights=w, k=5), first)
    # not with set_selection, not with a later fingerprint launch; one that did not read the planes result not with the planes entries
    before = _resident(ctx)
    sel = np.zeros(rec.n_atoms, np.uint8)
    sel[:5] = 1
    ctx.set_selection(sel)
    ctx.library_fingerprints(lfp.references([{}]), ALL15)
    ctx.library_planes_summary(off, x)
    ctx.set_ligand_library_planes(lib)
    assert before[0] == _capi.ARP_OK and _same_resident(_resident(ctx), before)
    # one that read the planes result goes with it
    for void in (lambda: ctx.library_planes_summary(off, x), lambda: ctx.set_ligand_library_planes(lib)):
        ctx.library_planes_summary(off, x)
        ctx.library_shortlist('summary', weights=w, k=5, tables=('atom_atom', 'atom_plane'))
        assert _resident(ctx, planes=True)[0] == _capi.ARP_OK
        ctx.set_selection(sel)
        assert _resident(ctx, planes=True)[0] == _capi.ARP_OK
        void()
        rc, msg, _ = _resident(ctx)
        assert rc == _capi.ARP_E_ARG and 'no result' in msg and ctx.library_shortlist_info()['chosen'] == 0
    # a new library launch, a new library, a new structure, models, a batch
    launches = ctx.library_shortlist_info()['launches']

    def made():
        ctx.library_summary(off, x, h, *PARAMS)
        ctx.library_shortlist('summary', weights=w, k=5)
        return _resident(ctx)[0] == _capi.ARP_OK
    assert made()
    ctx.library_summary(off, x, h, *PARAMS)                           # the same poses again: still a new result
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and ctx.library_shortlist_info() == dict(none, launches=launches + 1)
    assert _same_bytes(ctx.library_shortlist('summary', weights=w, k=5), first)
    ctx.set_ligand_library(lib)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and made()
    ctx.set_complex(rec_gpu)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and made()
    ctx.set_topology(rec_gpu)
    assert _resident(ctx)[0] == _capi.ARP_OK                          # (the kept topology is not the resident structure)
    ctx.set_models(np.stack([rec_gpu.xyz, rec_gpu.xyz]), np.stack([rec_gpu.h_xyz, rec_gpu.h_xyz]))
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.set_complex(rec_gpu)
    assert made()
    ctx.set_batch([rec_gpu, rec_gpu], [sel, sel])
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.close()


def _fetch_everything(ctx):
    packed, _ = ctx.fetch_packed()
    return {name: {k: np.array(v) for k, v in bag.items()} for name, bag in packed.items()}      # (copies: the buffer is the context's)


def _library_planes_fetch(ctx, T):
    """The resident library-planes result, fetched without a launch."""
    out = {}
    n = C.c_int64(0)
    info = ctx.library_planes_info()
    summary = np.empty((T, 16), np.uint32)
    for t, name in enumerate(poses.PLANE_TABLES):
        tab, args = ctx._plane_table_buffers(name, info[name], T + 1)
        ctx._check(ctx._L.arp_library_planes_fetch(ctx._h, t, info[name], _p(tab['pose_off']), *args, _p(summary) if t == 0 else None, C.byref(n)), 'fetch')
        out[name] = tab
    out['summary'] = summary
    return out


def _library_fetch(ctx, T):
    k = ctx.library_info()['records']
    return ctx._pose_records_fetch('arp_library_contacts_fetch', 'a', T, k)


def _library_best_fetch(ctx, L):
    out = dict(n_poses=np.empty(L, np.int64), best_pose=np.empty(L, np.int32), score=np.empty(L, np.int64))
    n = C.c_int64(0)
    ctx._check(ctx._L.arp_library_best_fetch(ctx._h, L, _p(out['n_poses']), _p(out['best_pose']), _p(out['score']), C.byref(n)), 'fetch')
    return out


def _library_fp_fetch(ctx, L):
    info = ctx.library_fingerprints_info()
    P, Q, U, NP = info['rows'], info['n_refs'], info['nodes'], info['planes']
    out = dict(ids=np.empty(U, np.int32), count=np.empty(P, np.uint32), cross=np.empty((P, Q), np.uint32), occupancy=np.empty((U, NP), np.uint32),
               bits=np.empty((P, NP, (U + 63) // 64), np.uint64))
    n, q = C.c_int64(0), C.c_int64(0)
    ctx._check(ctx._L.arp_library_fingerprints_fetch(ctx._h, U, _p(out['ids']), _p(out['count']), _p(out['cross']), _p(out['occupancy']), _p(out['bits']),
                                                     C.byref(n)), 'fetch')
    best = dict(n_poses=np.empty(L, np.int64), best_pose=np.empty((L, Q), np.int32), tanimoto_q32=np.empty((L, Q), np.int64))
    ctx._check(ctx._L.arp_library_fingerprints_best_fetch(ctx._h, L, _p(best['n_poses']), _p(best['best_pose']), _p(best['tanimoto_q32']), None, None,
                                                          C.byref(n), C.byref(q)), 'fetch')
    return out, best


@pytest.mark.gpu
def test_a_launch_voids_nothing():
    from test_pose_shortlist import _resident as pose_resident
    rec, ligs, ps = tp.case_main()
    rec_gpu = tp.device_planes(rec)
    ctx, lib = tp.library_ctx(rec_gpu, ligs)
    hem = np.nonzero(rec.res_id == int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]))[0]
    sel = np.zeros(rec.n_atoms, np.uint8)
    sel[hem] = 1
    ctx.set_selection(sel)
    counts = ctx.run_launch(5.0, 0.1, False)
    px, ph = synth.poses_of(rec, hem, 4, seed=11, shift=2.0)
    ctx.poses_contacts(px, ph, 5.0, 0.1, False)
    ctx.poses_shortlist('summary', weights=sl.weights(atom_atom={'records': 1}), k=3)
    off, x, h = ll.flatten_poses(lib, ps)
    T, L = int(off[-1]), len(ligs)
    ctx.library_contacts(off, x, h, *PARAMS)
    ctx.library_planes(off, x)
    ctx.library_best(np.ones(16, np.int32))
    ctx.library_fingerprints(lfp.references([{3: 0x7FFF}, {}]), ALL15)
    ctx.library_fingerprints_best()

    def everything():
        return (_fetch_everything(ctx), _library_fetch(ctx, T), _library_best_fetch(ctx, L), _library_planes_fetch(ctx, T), _library_fp_fetch(ctx, L),
                pose_resident(ctx)[2])
    before = everything()
    assert counts['atom_atom'] > 0 and len(before[1]['i']) > 0 and len(before[5]['pose']) == 3 and pose_resident(ctx)[0] == _capi.ARP_OK
    fp_launches = ctx.library_fingerprints_info()['launches']
    w = lsl.weights(atom_atom={'hbond': 3, 'proximal': -1}, planes={'atom_plane': 2})
    for kw in (dict(kind='summary', weights=w, k=4, tables=lsl.TABLES), dict(kind='tanimoto', unit='poses', ref=-1, k=3, sift_mask=SCATTERED),
               dict(kind='list', pose_ids=[3, 3, 0], tables=('group_group',), ctype_mask=INTER)):
        got = ctx.library_shortlist(kw.pop('kind'), **kw)
        assert len(got['pose']) in (3, 4)
        assert _same_bytes(everything(), before)
        assert ctx.library_fingerprints_info()['launches'] == fp_launches and ctx.library_info()['best']
    ctx.close()


@pytest.mark.gpu
def test_null_pointers_capacity_and_a_caller_owned_stream():
    from test_gpu_paths import _hip_runtime
    rec, ligs, ps = tp.case_main()
    ctx, lib = tp.library_ctx(tp.device_planes(rec), ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    ctx.library_contacts(off, x, h, *PARAMS)
    ctx.library_planes(off, x)
    w = lsl.weights(atom_atom={'records': 1}, planes={'atom_plane': 5})
    want = ctx.library_shortlist('summary', weights=w, k=6, tables=('atom_atom', 'atom_plane'))
    K, k, kp = 6, len(want['i']), len(want['atom_plane']['ctype'])
    assert len(want['pose']) == K and k > 0 and kp > 0
    L, hd = ctx._L, ctx._h
    n, m = C.c_int64(0), C.c_int64(0)
    none = [None] * 11
    assert L.arp_library_shortlist_fetch(hd, 0, 0, *none, C.byref(n), C.byref(m)) == _capi.ARP_OK and (n.value, m.value) == (K, k)
    assert L.arp_library_shortlist_fetch(hd, 0, 0, *none, None, C.byref(m)) == _capi.ARP_E_ARG
    assert L.arp_library_shortlist_fetch(hd, 0, 0, *none, C.byref(n), None) == _capi.ARP_E_ARG
    per_entry = dict(ligand=(0, want['ligand']), pose=(1, want['pose']), score=(2, want['score']), summary=(3, want['summary']),
                     planes_summary=(4, want['planes_summary']), off=(5, want['pose_off']))
    for key, (slot, ref) in per_entry.items():
        buf = np.full(ref.shape, 7, ref.dtype)
        args = list(none)
        args[slot] = _p(buf)
        n.value = m.value = 0
        assert L.arp_library_shortlist_fetch(hd, K - 1, 0, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_CAPACITY, key
        assert (n.value, m.value) == (K, k) and (buf == 7).all() and 'cap_entries' in L.arp_last_error(hd).decode()
        assert L.arp_library_shortlist_fetch(hd, K, 0, *args, C.byref(n), C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, ref), key      # one array alone
    for slot, key in enumerate(ll.COLUMNS):
        buf = np.full(k, 7, want[key].dtype)
        args = list(none)
        args[6 + slot] = _p(buf)
        assert L.arp_library_shortlist_fetch(hd, 0, k - 1, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_CAPACITY and (buf == 7).all()
        assert L.arp_library_shortlist_fetch(hd, 0, k, *args, C.byref(n), C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, want[key]), key
    # the planes fetch: the same protocol
    tab = want['atom_plane']
    pnone = [None] * 10
    assert L.arp_library_shortlist_planes_fetch(hd, 0, 0, 0, *pnone, C.byref(m)) == _capi.ARP_OK and m.value == kp
    assert L.arp_library_shortlist_planes_fetch(hd, 0, 0, 0, *pnone, None) == _capi.ARP_E_ARG
    assert L.arp_library_shortlist_planes_fetch(hd, 4, 0, 0, *pnone, C.byref(m)) == _capi.ARP_E_ARG
    assert L.arp_library_shortlist_planes_fetch(hd, 1, 0, 0, *pnone, C.byref(m)) == _capi.ARP_E_ARG and 'was not requested' in L.arp_last_error(hd).decode()
    offs = np.full(K + 1, 7, np.uint64)
    assert L.arp_library_shortlist_planes_fetch(hd, 0, K - 1, 0, _p(offs), *pnone[1:], C.byref(m)) == _capi.ARP_E_CAPACITY and (offs == 7).all()
    assert L.arp_library_shortlist_planes_fetch(hd, 0, K, 0, _p(offs), *pnone[1:], C.byref(m)) == _capi.ARP_OK and _same_bytes(offs, tab['pose_off'])
    for slot, key in ((1, 'atom'), (2, 'ring'), (3, 'dist'), (4, 'theta'), (7, 'mask'), (8, 'ctype')):
        buf = np.full(kp, 7, tab[key].dtype)
        args = list(pnone)
        args[slot] = _p(buf)
        assert L.arp_library_shortlist_planes_fetch(hd, 0, 0, kp - 1, *args, C.byref(m)) == _capi.ARP_E_CAPACITY and (buf == 7).all()
        assert L.arp_library_shortlist_planes_fetch(hd, 0, 0, kp, *args, C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, tab[key]), key
    buf = np.zeros(kp, np.float64)
    args = list(pnone)
    args[5] = _p(buf)                                                 # atom_plane has two value columns: no third
    assert L.arp_library_shortlist_planes_fetch(hd, 0, 0, kp, *args, C.byref(m)) == _capi.ARP_E_ARG and 'no such value column' in L.arp_last_error(hd).decode()
    # a launch that did not read the planes result has no planes_summary
    ctx.library_shortlist('summary', weights=lsl.weights(atom_atom={'records': 1}), k=6)
    buf = np.zeros((6, 16), np.uint32)
    args = list(none)
    args[4] = _p(buf)
    assert L.arp_library_shortlist_fetch(hd, 6, 0, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_ARG and 'did not read' in L.arp_last_error(hd).decode()
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    ctx.library_summary(off, x, h, *PARAMS)
    ctx.library_planes_summary(off, x)
    got = ctx.library_shortlist('summary', weights=w, k=6, tables=('atom_atom', 'atom_plane'))
    assert _same_bytes(got, want)
    ctx.use_stream(0)                                                 # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------------------------------------------------- GPU: end to end
@pytest.mark.gpu
def test_run_library_shortlist_in_chunks_equals_one_chunk_and_the_full_route(tmp_path):
    rec, ligs, ps = tl.case_main()
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    ic = InteractionComplex(copy.copy(rec))
    full = ic.run_ligand_library(ligs, ps, *PARAMS)
    lo = full['ligand_pose_off']
    # a weighting that puts the best pose of the water (70 poses, cut at 32 and 64) behind the first cut
    cands = [lsl.weights(atom_atom={n: s, 'records': r}) for n in ('vdw', 'hbond', 'hydrophobic', 'proximal') for s in (5, -5) for r in (1, -1)]
    w = next(c for c in cands if best_per_ligand(pose_scores('summary', full, c), lo)[0] >= 32)
    zero = np.zeros(32, np.int32)                                     # every score 0: ties straddle every boundary, the lower pose wins
    for ww in (w, zero):
        score = pose_scores('summary', full, ww)
        for unit in lsl.UNITS:
            for k in (4, 40):
                chosen = ranked(score, lo, unit, k)
                want = expected(full, chosen, score, SCATTERED, 0x7F)
                want['pose'] = want['pose'].astype(np.int64)
                one = ic.run_library_shortlist(lib, off, x, h, k, unit=unit, weights=ww, contacts=[n for n in config.SIFT_NAMES if BIT[n] & SCATTERED])
                cut = ic.run_library_shortlist(lib, off, x, h, k, unit=unit, weights=ww, contacts=[n for n in config.SIFT_NAMES if BIT[n] & SCATTERED], chunk=32)
                assert differences(one, want) == [] and differences(cut, want) == [], (unit, k)
                assert _same_bytes({c: cut[c] for c in want}, {c: one[c] for c in want}) and ic.library_shortlist is cut
                took = lsl.take(full, chosen, SCATTERED)
                assert all(_same_bytes(cut[c], took[c]) for c in ll.COLUMNS + ('pose_off', 'summary', 'ligand', 'ligand_pose_off'))
    # by Tanimoto, the reference a pose of the haem
    ref = lfp.reference_from_pose(full, int(lo[2]) + 1, rec.res_id)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    ctx.library_summary(off, x, h, *PARAMS)
    fpr = ctx.library_fingerprints(lfp.references([ref]), lfp.planes(None))
    ctx.close()
    score = pose_scores('tanimoto', fpr=fpr, ref=0)
    for unit in lsl.UNITS:
        chosen = ranked(score, lo, unit, 7)
        want = expected(full, chosen, score)
        want['pose'] = want['pose'].astype(np.int64)
        for chunk in (None, 32):
            got = ic.run_library_shortlist(ligs, off, x, h, 7, by='tanimoto', unit=unit, refs=[ref], chunk=chunk)
            assert differences(got, want) == [], (unit, chunk)
    assert got['by'] == 'tanimoto' and got['unit'] == 'ligands'
    path = ic.write_library_shortlist(str(tmp_path))
    lines = open(path).read().splitlines()
    assert path.endswith('.libraryshortlist') and len(lines) == 1 + len(got['i']) and lines[1].split(',')[:3] == ['0', str(got['ligand'][0]), str(got['pose'][0])]
    with pytest.raises(ValueError, match='by must be'):
        ic.run_library_shortlist(lib, off, x, h, 3, by='rmsd')
    with pytest.raises(ValueError, match='unit must be'):
        ic.run_library_shortlist(lib, off, x, h, 3, unit='molecules')
    with pytest.raises(ValueError, match='k must be'):
        ic.run_library_shortlist(lib, off, x, h, 0)
