"""Water-bridge persistence over the models of an ensemble, reduced on the device
(arp_models_water_bridge_persistence_launch / _fetch, Context.models_water_bridge_persistence,
EnsembleComplex.run_water_bridge_persistence, arpeggio_amd.bridge_persistence).

The yardstick is never the device table and never ``bridge_persistence.fold``: it is ``loop_fold`` below, plain Python loops
over per-model bridge tables with topology ids — made by ``test_water_bridges._join`` (loops as well) from the ORACLE's
per-model atom-atom bags.  Every column is compared as bytes, ``dist_sum`` included: its order is the contract.  No tolerance
anywhere."""
import copy
import csv
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

from arpeggio_amd import _capi, bridge_persistence as bp, contact_filter, synth, tables, water_bridges as wb
from arpeggio_amd.core import config
from helpers import tiny_complex
from test_persistence import PARAMS, _ctx_with_models, _mask, _oracle_bags
from test_water_bridges import ALL, BIT, COLS, CT, DTYPES, HP, SAME, SPECIFIC, _join, _shell, _two_interleaved_residues, seam_shells
from test_water_bridges import _same_table as _same_bridges

BYRES = 2
LEVELS = ('atom', 'residue')
F_HUB = 8


def loop_fold(per_model, res=None):
    """The yardstick: per-model bridge tables (topology ids) folded by loops, models in ascending order.  ``res``: the residue
    of every topology atom for the residue level, ``None`` for the atom level."""
    rows = {}
    for f, t in enumerate(per_model):
        model = {}
        for r in range(len(t['water'])):
            a, b = int(t['a'][r]), int(t['b'][r])
            legs = [(int(t['sift_a'][r]), int(t['ctype_a'][r])), (int(t['sift_b'][r]), int(t['ctype_b'][r]))]
            if res is None:
                pair = (a, b)
            else:
                ra, rb = int(res[a]), int(res[b])
                pair = (min(ra, rb), max(ra, rb))
                if ra > rb:
                    legs.reverse()
            path = np.float32(np.float32(t['dist_a'][r]) + np.float32(t['dist_b'][r]))
            assert path.dtype == np.float32
            m = model.setdefault(pair, dict(waters=set(), n=0, dmin=np.float32(np.inf), s=[0, 0], c=[0, 0]))
            m['waters'].add(int(t['water'][r]))
            m['n'] += 1
            m['dmin'] = min(m['dmin'], path)
            for q in (0, 1):
                m['s'][q] |= legs[q][0] & 0x7FFF
                m['c'][q] |= 1 << legs[q][1]
        for pair, m in model.items():      # one model closes: what it adds to each of its pairs
            R = rows.setdefault(pair, dict(nm=0, first=f, last=f, nw=0, nb=0, dmin=np.float32(np.inf), dmax=np.float32(-np.inf),
                                           dsum=0.0, bits=[[0] * 15, [0] * 15], c=[0, 0]))
            R['nm'] += 1
            R['last'] = f
            R['nw'] += len(m['waters'])
            R['nb'] += m['n']
            R['dmin'] = min(R['dmin'], m['dmin'])
            R['dmax'] = max(R['dmax'], m['dmin'])
            R['dsum'] = R['dsum'] + float(np.float64(m['dmin']))
            for q in (0, 1):
                for k in range(15):
                    R['bits'][q][k] += (m['s'][q] >> k) & 1
                R['c'][q] |= m['c'][q]
    pairs = sorted(rows)
    ka, kb = ('a', 'b') if res is None else ('res_a', 'res_b')
    g = lambda f, dt: np.array([f(rows[p]) for p in pairs], dt)
    out = {ka: np.array([p[0] for p in pairs], np.int32), kb: np.array([p[1] for p in pairs], np.int32),
           'n_models': g(lambda R: R['nm'], np.uint16), 'first': g(lambda R: R['first'], np.int32), 'last': g(lambda R: R['last'], np.int32),
           'n_waters': g(lambda R: R['nw'], np.uint32), 'n_bridges': g(lambda R: R['nb'], np.uint32),
           'dist_min': g(lambda R: R['dmin'], np.float32), 'dist_max': g(lambda R: R['dmax'], np.float32),
           'dist_sum': g(lambda R: R['dsum'], np.float64),
           'bit_models_a': np.array([rows[p]['bits'][0] for p in pairs], np.uint16).reshape(-1, 15),
           'bit_models_b': np.array([rows[p]['bits'][1] for p in pairs], np.uint16).reshape(-1, 15),
           'ctype_mask_a': g(lambda R: R['c'][0], np.uint8), 'ctype_mask_b': g(lambda R: R['c'][1], np.uint8)}
    return out


def _same(got, want, what):
    level = 'residue' if 'res_a' in want else 'atom'
    assert list(got) == [k for k, _ in bp.COLUMNS[level]] == list(want), what
    for k, dt in bp.COLUMNS[level]:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == dt and w.dtype == dt and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


def _resident(per_model, n):
    """Per-model bridge tables with topology ids -> the one table with resident ids that the device holds."""
    out = {}
    for k, dt in zip(COLS, DTYPES):
        parts = [(np.asarray(t[k]).astype(np.int64) + f * n).astype(dt) if k in ('water', 'a', 'b') else np.asarray(t[k], dt)
                 for f, t in enumerate(per_model)]
        out[k] = np.concatenate(parts) if parts else np.zeros(0, dt)
    return out


def _bridge_table(rows):
    return {k: np.array([r[q] for r in rows], dt) for q, (k, dt) in enumerate(zip(COLS, DTYPES))}


def _hdr():
    return open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()


# ---- the parity structure: proteinlike40 with 20 waters, 8 models, by the oracle
@functools.lru_cache(maxsize=None)
def _hub():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    pc.ensure_labels()
    return pc


@functools.lru_cache(maxsize=None)
def _hub_models(F=F_HUB):
    pc = _hub()
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    return pc, xyz, h_xyz


HUB_CASES = {'whole': (None, PARAMS[0]), '508': ('/A/508/', PARAMS[2])}


@functools.lru_cache(maxsize=None)
def _hub_bags(case):
    pc, xyz, h_xyz = _hub_models()
    sel, params = HUB_CASES[case]
    bags = _oracle_bags(pc, xyz, h_xyz, params, None if sel is None else _mask(pc, [sel]))
    assert all(b.get('err', 0) == 0 for b in bags)
    return bags


@functools.lru_cache(maxsize=None)
def _hub_per_model(case, sift_any, same):
    pc = _hub()
    return tuple(_join(b, pc.flags, pc.res_id, sift_any, same) for b in _hub_bags(case))


@functools.lru_cache(maxsize=None)
def _hub_want(case, sift_any, same, level):
    return loop_fold(_hub_per_model(case, sift_any, same), _hub().res_id if level == 'residue' else None)


def _runs(t):
    """(start, end) of every row's run among the sorted records: the rows ascend by the pair and n_bridges are their records."""
    end = np.cumsum(t['n_bridges'].astype(np.int64))
    return end - t['n_bridges'], end


# ------------------------------------------------------------------------------------------------------------- CPU
def _hand_made():
    """Topology of 8 atoms: 0, 1 residue 0; 2, 3 residue 1; 4 residue 2; waters 5, 6, 7 (residues 3, 4, 5).  Three models."""
    H, P, V = BIT['hbond'], BIT['polar'], BIT['vdw']
    SW, NW = CT['SELECTION_WATER'], CT['NON_SELECTION_WATER']
    res = np.array([0, 0, 1, 1, 2, 3, 4, 5], np.int32)
    m0 = _bridge_table([(5, 0, 2, 2.5, 3.0, H, P, SW, NW),          # (0, 2) through two waters in model 0
                        (5, 0, 3, 2.5, 3.5, H, V, SW, NW),          # water 5 bridges residues (0, 1) through two atom pairs
                        (6, 0, 2, 2.0, 2.25, P, H | V, SW, NW),
                        (6, 1, 3, 1.5, 1.0, P, V, SW, NW)])
    m1 = _bridge_table([])
    m2 = _bridge_table([(7, 0, 2, 3.0, 3.0, V, V, NW, NW),
                        (7, 2, 4, 3.0, 2.0, V, H, NW, SW),
                        (7, 0, 1, 3.0, 1.0, V, P, NW, NW)])         # one residue: SAME_RESIDUE only
    return [m0, m1, m2], res


def test_fold_on_a_hand_made_bridge_table():
    per, res = _hand_made()
    H, P, V = BIT['hbond'], BIT['polar'], BIT['vdw']
    SW, NW = 1 << CT['SELECTION_WATER'], 1 << CT['NON_SELECTION_WATER']
    t = loop_fold(per)
    assert list(zip(t['a'].tolist(), t['b'].tolist())) == [(0, 1), (0, 2), (0, 3), (1, 3), (2, 4)]
    assert t['n_models'].tolist() == [1, 2, 1, 1, 1] and t['first'].tolist() == [2, 0, 0, 0, 2] and t['last'].tolist() == [2, 2, 0, 0, 2]
    assert t['n_waters'].tolist() == [1, 3, 1, 1, 1] == t['n_bridges'].tolist()
    assert t['dist_min'].tolist() == [4.0, 4.25, 6.0, 2.5, 5.0] and t['dist_max'].tolist() == [4.0, 6.0, 6.0, 2.5, 5.0]
    assert t['dist_sum'].tolist() == [4.0, 10.25, 6.0, 2.5, 5.0]
    bits = lambda *names: [1 if config.SIFT_NAMES[k] in names else 0 for k in range(15)]
    assert t['bit_models_a'][1].tolist() == [a + b for a, b in zip(bits('hbond', 'polar'), bits('vdw'))]      # model 0: H | P, model 2: V
    assert t['bit_models_b'][1].tolist() == [a + b for a, b in zip(bits('polar', 'hbond', 'vdw'), bits('vdw'))]
    assert t['ctype_mask_a'].tolist() == [NW, SW | NW, SW, SW, NW] and t['ctype_mask_b'].tolist() == [NW, NW, NW, NW, SW]
    r = loop_fold(per, res)
    assert list(zip(r['res_a'].tolist(), r['res_b'].tolist())) == [(0, 0), (0, 1), (1, 2)]
    assert r['n_models'].tolist() == [1, 2, 1] and r['n_waters'].tolist() == [1, 3, 1] and r['n_bridges'].tolist() == [1, 5, 1]
    assert r['dist_min'].tolist() == [4.0, 2.5, 5.0] and r['dist_max'].tolist() == [4.0, 6.0, 5.0] and r['dist_sum'].tolist() == [4.0, 8.5, 5.0]
    assert r['bit_models_a'][1].tolist() == [a + b for a, b in zip(bits('hbond', 'polar'), bits('vdw'))]
    assert r['ctype_mask_a'].tolist() == [NW, SW | NW, NW] and r['ctype_mask_b'].tolist() == [NW, NW, SW]
    # partners met in either residue order: leg a is the one in res_a
    flip = [_bridge_table([(7, 0, 2, 1.0, 2.0, H, P, 3, 4), (7, 3, 4, 1.0, 2.0, H, P, 3, 4)])]
    other = np.array([1, 0, 0, 2, 0, 0, 0, 0], np.int32)      # atom 0 in residue 1, atom 2 in residue 0: swapped; 3 in 2, 4 in 0: swapped
    u = loop_fold(flip, other)
    assert list(zip(u['res_a'].tolist(), u['res_b'].tolist())) == [(0, 1), (0, 2)]
    assert u['bit_models_a'][0].tolist() == bits('polar') and u['bit_models_b'][0].tolist() == bits('hbond')
    assert u['ctype_mask_a'].tolist() == [1 << 4, 1 << 4] and u['ctype_mask_b'].tolist() == [1 << 3, 1 << 3]
    # the twin
    for rs, what in ((None, 'atom'), (res, 'residue')):
        _same(bp.fold(_resident(per, 8), 8, rs), loop_fold(per, rs), what)
    _same(bp.fold(_resident(flip, 8), 8, other), u, 'flip')
    for level in LEVELS:
        _same(bp.fold(wb.empty(), 8, None if level == 'atom' else res), bp.empty(level), level)
        _same(bp.empty(level), loop_fold([], None if level == 'atom' else res), level)
        assert tuple(bp.COLUMNS[level]) == tuple(bp.LEVELS[level].columns)
    with pytest.raises(ValueError):
        bp.fold(wb.empty(), 0)
    with pytest.raises(ValueError):
        bp.empty('chain')
    # the order of dist_sum: float32 paths whose float64 sum depends on the order
    big = np.float32(2.0 ** 60)
    order = [_bridge_table([(2, 0, 1, big, 0.0, 1, 1, 0, 0)]), _bridge_table([(2, 0, 1, 1.0, 0.0, 1, 1, 0, 0)]), _bridge_table([(2, 0, 1, -big, 0.0, 1, 1, 0, 0)])]
    assert loop_fold(order)['dist_sum'].tolist() == [0.0] == bp.fold(_resident(order, 3), 3)['dist_sum'].tolist()      # (any other order gives 1.0)


def _random_models(rs, F, same, n=30, n_waters=6, n_res=7, empty=()):
    """Per-model bridge tables in (water, a, b) order over ``n`` atoms, the last ``n_waters`` of them waters, with the
    residues of the partners; without ``same`` no row has both partners in one residue."""
    res = np.r_[rs.randint(0, n_res, n - n_waters), n_res + np.arange(n_waters)].astype(np.int32)
    per = []
    for f in range(F):
        rows = []
        for w in range(n - n_waters, n):
            if f in empty or rs.rand() < 0.2:
                continue
            ps = np.sort(rs.choice(n - n_waters, rs.randint(2, 7), replace=False))
            leg = {int(p): (np.float32(rs.rand() * 3 + 1.5), int(rs.randint(1, 1 << 15)), int(rs.randint(0, 7))) for p in ps}
            for x in range(len(ps)):
                for y in range(x + 1, len(ps)):
                    a, b = int(ps[x]), int(ps[y])
                    if same or res[a] != res[b]:
                        rows.append((w, a, b, leg[a][0], leg[b][0], leg[a][1], leg[b][1], leg[a][2], leg[b][2]))
        per.append(_bridge_table(rows))
    return per, res


def test_fold_on_random_bridge_tables_equals_the_loops():
    for seed, same in ((3, False), (5, True), (8, False), (13, True)):
        rs = np.random.RandomState(seed)
        F, n = 9, 30
        per, res = _random_models(rs, F, same, empty=(4,))
        at, rt = loop_fold(per), loop_fold(per, res)
        assert len(at['a']) > 100 and len(rt['res_a']) > 10
        assert (at['n_waters'] > at['n_models']).any()             # several waters for one pair in one model
        assert (at['n_waters'] == at['n_bridges']).all()
        assert (rt['n_bridges'] > rt['n_waters']).any()            # a water bridges a residue pair through several atom pairs
        assert (rt['n_models'] == F - 1).any() and (at['n_models'] == 1).any() and (at['first'] > 0).any() and (at['last'] < F - 1).any()
        assert bool((rt['res_a'] == rt['res_b']).any()) == same    # equal residues under SAME_RESIDUE only
        assert int(at['n_bridges'].sum()) == int(rt['n_bridges'].sum()) == sum(len(t['water']) for t in per)
        whole = _resident(per, n)
        _same(bp.fold(whole, n), at, (seed, 'atom'))
        _same(bp.fold(whole, n, res), rt, (seed, 'residue'))
        # the table is a function of the bridge table as a set of rows
        p = rs.permutation(len(whole['water']))
        shuffled = {k: whole[k][p] for k in COLS}
        _same(bp.fold(shuffled, n), at, (seed, 'atom, shuffled'))
        _same(bp.fold(shuffled, n, res), rt, (seed, 'residue, shuffled'))


def test_merge_of_two_chunks_equals_the_whole_at_every_boundary():
    rs = np.random.RandomState(17)
    F, n = 8, 30
    per, res = _random_models(rs, F, True, empty=(3,))
    for level, rid in (('atom', None), ('residue', res)):
        ka, kb = [k for k, _ in bp.COLUMNS[level]][:2]
        whole = loop_fold(per, rid)
        exact = [k for k, _ in bp.COLUMNS[level] if k != 'dist_sum']
        stride = int(whole[kb].max()) + 1
        key = lambda t: t[ka].astype(np.int64) * stride + t[kb]
        assert len(whole[ka]) > 15 and whole['n_models'].max() > 1
        for c in range(1, F):
            t1, t2 = loop_fold(per[:c], rid), loop_fold(per[c:], rid)
            m = bp.merge(t1, t2, c)
            assert list(m) == [k for k, _ in bp.COLUMNS[level]]
            for k in exact:
                assert m[k].dtype == whole[k].dtype and m[k].tobytes() == whole[k].tobytes(), (level, c, k)
            # dist_sum: t1's sum + t2's sum, in that order, to the bit (a pair of one chunk alone: the other's sum is 0.0)
            s1, s2 = np.zeros(len(m[ka])), np.zeros(len(m[ka]))
            s1[np.searchsorted(key(m), key(t1))] = t1['dist_sum']
            s2[np.searchsorted(key(m), key(t2))] = t2['dist_sum']
            assert m['dist_sum'].tobytes() == (s1 + s2).tobytes(), (level, c)
            assert np.allclose(m['dist_sum'], whole['dist_sum'], rtol=1e-14, atol=0)
        m = bp.merge(bp.merge(loop_fold(per[:2], rid), loop_fold(per[2:5], rid), 2), loop_fold(per[5:], rid), 5)
        for k in exact:
            assert m[k].tobytes() == whole[k].tobytes(), (level, 'three', k)
        for m in (bp.merge(bp.empty(level), whole, 0), bp.merge(whole, bp.empty(level), F)):
            _same(m, whole, (level, 'empty side'))
        for k, top in (('n_models', 40000), ('n_waters', 0xC0000000), ('n_bridges', 0xC0000000), ('bit_models_a', 40000), ('bit_models_b', 40000)):
            hi = dict(whole)
            hi[k] = np.full(whole[k].shape, top, whole[k].dtype)
            with pytest.raises(OverflowError, match=k):
                bp.merge(hi, hi, F)
    with pytest.raises(ValueError):
        bp.merge(loop_fold(per), loop_fold(per, res), F)
    with pytest.raises(ValueError):
        bp.merge(loop_fold(per), loop_fold(per), -1)


def _small_table():
    per, res = _hand_made()
    return loop_fold(per), loop_fold(per, res)


def test_frequency_ligand_rows_records_and_csv_text_of_a_hand_made_table(tmp_path):
    pc = _hub()
    at, rt = _small_table()
    fr = bp.frequency(at, 4)
    assert fr['bridge'].tolist() == [0.25, 0.5, 0.25, 0.25, 0.25] and fr['bridge'].dtype == np.float64
    assert fr['bits_a'].shape == fr['bits_b'].shape == (5, 15) and fr['bits_a'][1, 5] == 0.25 and fr['bits_b'][1, 3] == 0.5
    with pytest.raises(ValueError):
        bp.frequency(at, 0)
    lig = bp.ligand_rows(at)
    assert list(zip(lig['a'].tolist(), lig['b'].tolist())) == [(0, 2), (0, 3), (1, 3), (2, 4)] and list(lig) == list(at)
    assert lig['dist_sum'].tolist() == [10.25, 6.0, 2.5, 5.0] and lig['bit_models_a'].shape == (4, 15)
    lig = bp.ligand_rows(rt)
    assert list(zip(lig['res_a'].tolist(), lig['res_b'].tolist())) == [(0, 1), (1, 2)]
    assert len(bp.ligand_rows(bp.empty())['a']) == 0
    from arpeggio_amd.core import export
    lab = export.Labels(pc, pc.component_types)
    rec = bp.to_records(at, pc)
    assert len(rec) == 5 and rec[1]['type'] == 'water-bridge-persistence' and rec[1]['level'] == 'atom'
    assert {k: rec[1]['bgn'][k] for k in lab.atom_dict(0)} == lab.atom_dict(0) and {k: rec[1]['end'][k] for k in lab.atom_dict(2)} == lab.atom_dict(2)
    assert rec[1]['n_models'] == 2 and rec[1]['first_model'] == 0 and rec[1]['last_model'] == 2 and rec[1]['n_waters'] == 3 == rec[1]['n_bridges']
    assert rec[1]['distance_min'] == 4.25 and rec[1]['distance_max'] == 6.0 and rec[1]['distance_sum'] == 10.25 and rec[1]['distance_mean'] == 5.125
    assert rec[1]['bgn']['contact'] == {'vdw': 1, 'hbond': 1, 'polar': 1} and rec[1]['end']['contact'] == {'vdw': 2, 'hbond': 1, 'polar': 1}
    assert rec[1]['bgn']['interacting_entities'] == ['SELECTION_WATER', 'NON_SELECTION_WATER'] and rec[1]['end']['interacting_entities'] == ['NON_SELECTION_WATER']
    assert json.loads(json.dumps(rec)) == rec
    rr = bp.to_records(rt, pc)
    assert len(rr) == 3 and rr[1]['level'] == 'residue' and rr[1]['n_bridges'] == 5 and rr[1]['n_waters'] == 3
    path = tmp_path / 'x.bridgepersist'
    bp.write_csv(str(path), at, pc)
    lines = path.read_text().splitlines()
    names = list(config.SIFT_NAMES[:15])
    assert lines[0] == ','.join(['atom_bgn', 'atom_end', 'n_models', 'first_model', 'last_model', 'n_waters', 'n_bridges', 'distance_min',
                                 'distance_max', 'distance_sum'] + [x + '_bgn' for x in names] + [x + '_end' for x in names] +
                                ['interacting_entities_bgn', 'interacting_entities_end']) == ','.join(bp.csv_header('atom'))
    assert lines[2] == ','.join([lab.atom_macro(0), lab.atom_macro(2), '2', '0', '2', '3', '3', '4.25', '6.0', '10.25'] +
                                [str(x) for x in at['bit_models_a'][1].tolist() + at['bit_models_b'][1].tolist()] +
                                ['SELECTION_WATER|NON_SELECTION_WATER', 'NON_SELECTION_WATER']) and len(lines) == 6
    assert bp.write_bridge_persistence(str(tmp_path), 'abc', rt, pc) == os.path.join(str(tmp_path), 'abc.bridgepersist')
    lines = (tmp_path / 'abc.bridgepersist').read_text().splitlines()
    assert lines[0].startswith('residue_bgn,residue_end,n_models') and lines[2].startswith(','.join([lab.res_macro[0], lab.res_macro[1], '2', '0', '2', '3', '5', '2.5', '6.0', '8.5']))
    _same(_parse_csv(str(path), pc, 'atom'), at, 'csv, atom')
    _same(_parse_csv(str(tmp_path / 'abc.bridgepersist'), pc, 'residue'), rt, 'csv, residue')


def _parse_csv(path, pc, level):
    from arpeggio_amd.core import export
    lab = export.Labels(pc, pc.component_types)
    ids = {lab.atom_macro(i): i for i in range(pc.n_atoms)} if level == 'atom' else {lab.res_macro[r]: r for r in range(pc.n_residues)}
    with open(path, newline='') as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == bp.csv_header(level)
    ct = lambda s: sum(1 << CT[x] for x in s.split('|')) if s else 0
    ka, kb = ('a', 'b') if level == 'atom' else ('res_a', 'res_b')
    body = rows[1:]
    col = lambda f, dt: np.array([f(r) for r in body], dt)
    return {ka: col(lambda r: ids[r[0]], np.int32), kb: col(lambda r: ids[r[1]], np.int32), 'n_models': col(lambda r: int(r[2]), np.uint16),
            'first': col(lambda r: int(r[3]), np.int32), 'last': col(lambda r: int(r[4]), np.int32), 'n_waters': col(lambda r: int(r[5]), np.uint32),
            'n_bridges': col(lambda r: int(r[6]), np.uint32), 'dist_min': col(lambda r: np.float32(r[7]), np.float32),
            'dist_max': col(lambda r: np.float32(r[8]), np.float32), 'dist_sum': col(lambda r: float(r[9]), np.float64),
            'bit_models_a': np.array([[int(x) for x in r[10:25]] for r in body], np.uint16).reshape(-1, 15),
            'bit_models_b': np.array([[int(x) for x in r[25:40]] for r in body], np.uint16).reshape(-1, 15),
            'ctype_mask_a': col(lambda r: ct(r[40]), np.uint8), 'ctype_mask_b': col(lambda r: ct(r[41]), np.uint8)}


def test_header_constants_match_the_binding():
    hdr = _hdr()
    assert int(re.search(r'#define\s+ARP_WBP_BY_RESIDUE\s+\(1u << (\d+)\)', hdr).group(1)) == 1 and _capi.WBP_BY_RESIDUE == bp.BY_RESIDUE == BYRES == 2
    assert int(re.search(r'#define\s+ARP_WBP_BITS\s+(\d+)', hdr).group(1)) == _capi.WBP_BITS == bp.N_BITS == tables.N_BITS == 15
    assert wb.SAME_RESIDUE == SAME == 1 and not (wb.SAME_RESIDUE & _capi.WBP_BY_RESIDUE)
    for s in ('arp_models_water_bridge_persistence_launch', 'arp_models_water_bridge_persistence_fetch'):
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    want = (np.int32, np.int32, np.uint16, np.int32, np.int32, np.uint32, np.uint32, np.float32, np.float32, np.float64, np.uint16, np.uint16, np.uint8, np.uint8)
    for spec, names in ((tables.BRIDGEPERSIST_ATOM, ('a', 'b')), (tables.BRIDGEPERSIST_RESIDUE, ('res_a', 'res_b'))):
        assert tuple(k for k, _ in spec.columns) == names + ('n_models', 'first', 'last', 'n_waters', 'n_bridges', 'dist_min', 'dist_max', 'dist_sum',
                                                             'bit_models_a', 'bit_models_b', 'ctype_mask_a', 'ctype_mask_b')
        assert tuple(dt for _, dt in spec.columns) == want and spec.width == {'bit_models_a': 15, 'bit_models_b': 15}
    # the fetch's arguments in the header are the columns, in this order
    proto = re.search(r'int arp_models_water_bridge_persistence_fetch\(([^;]*)\);', hdr).group(1)
    args = re.findall(r'(\w+)\s*(?:/\*[^*]*\*/)?\s*(?:,|$)', re.sub(r'\s+', ' ', proto))
    assert args == ['ctx', 'cap', 'a', 'b'] + [k for k, _ in tables.BRIDGEPERSIST_ATOM.columns][2:] + ['count']


# (mask) -> bridge rows over the 8 models, rows keyed by atom pair, by residue pair, longest residue-pair run
HUB_FIGURES = {HP: (104, 60, 25, 17), SPECIFIC: (804, 390, 37, 146), ALL: (4875, 1666, 94, 409)}


def test_the_parity_structure_is_what_it_claims():
    """proteinlike40 with 20 waters, F = 8, whole structure, 5.0 A, by the oracle and the loops: the figures the GPU cases
    lean on — rows in every model and in one only, residue-pair runs over several 64-steps, pairs with several waters in one
    model, and a run that lies across record 2048 (the second tile of the run kernels)."""
    pc = _hub()
    assert pc.n_atoms == 532 and pc.n_residues == 61
    assert sum(len(b['i']) for b in _hub_bags('whole')) == 9016
    for sa, (rows, atom_rows, res_rows, longest) in HUB_FIGURES.items():
        at, rt = _hub_want('whole', sa, False, 'atom'), _hub_want('whole', sa, False, 'residue')
        assert sum(len(t['water']) for t in _hub_per_model('whole', sa, False)) == rows == int(at['n_bridges'].sum()) == int(rt['n_bridges'].sum())
        assert (len(at['a']), len(rt['res_a']), int(rt['n_bridges'].max())) == (atom_rows, res_rows, longest), hex(sa)
    at, rt = _hub_want('whole', ALL, False, 'atom'), _hub_want('whole', ALL, False, 'residue')
    assert int((at['n_models'] == F_HUB).sum()) == 47 and int((at['n_models'] == 1).sum()) == 710
    assert int((at['n_waters'] > at['n_models']).sum()) == 83          # a model is a segment of a run at the atom level too
    assert int((rt['n_bridges'] > 64).sum()) == 22 and int((rt['n_bridges'] > 128).sum()) == 13
    assert (rt['n_bridges'] > rt['n_waters']).any() and (rt['n_models'] == F_HUB).any() and (rt['n_models'] < F_HUB).any()
    at, rt = _hub_want('whole', ALL, True, 'atom'), _hub_want('whole', ALL, True, 'residue')
    assert (int(at['n_bridges'].sum()), len(at['a']), len(rt['res_a']), int(rt['n_bridges'].max())) == (7066, 2254, 127, 666)
    assert (rt['res_a'] == rt['res_b']).any()
    for same in (False, True):
        s, e = _runs(_hub_want('whole', ALL, same, 'residue'))
        assert ((s < 2048) & (e > 2048)).any(), same
    # the twin on the same rows
    n = pc.n_atoms
    for same in (False, True):
        whole = _resident(_hub_per_model('whole', ALL, same), n)
        _same(bp.fold(whole, n), _hub_want('whole', ALL, same, 'atom'), same)
        _same(bp.fold(whole, n, pc.res_id), _hub_want('whole', ALL, same, 'residue'), same)


# ------------------------------------------------------------------------------------------------------------- GPU
def _flags(same, level):
    return (SAME if same else 0) | (BYRES if level == 'residue' else 0)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(HUB_CASES))
def test_parity_with_the_loops_on_the_oracles_bags(case):
    pc, xyz, h_xyz = _hub_models()
    sel, params = HUB_CASES[case]
    ctx = _ctx_with_models(pc, xyz, h_xyz, sort_after=False)
    if sel is not None:
        ctx.set_selection(np.tile(_mask(pc, [sel]), F_HUB))
    ctx.run_launch(*params)
    for sa in (HP, SPECIFIC, ALL):
        for same in (False, True):
            for level in LEVELS:
                want = _hub_want(case, sa, same, level)
                got = ctx.models_water_bridge_persistence(sa, _flags(same, level))
                print(case, hex(sa), same, level, 'rows', len(got['n_models']), 'bridges', int(want['n_bridges'].sum()), 'longest run', int(want['n_bridges'].max(initial=0)))
                _same(got, want, (case, hex(sa), same, level))
    # every bit, residue level: runs over several 64-steps, one of them across record 2048
    for same in (False, True):
        want = _hub_want(case, ALL, same, 'residue')
        s, e = _runs(want)
        assert ((s < 2048) & (e > 2048)).any() and int(want['n_bridges'].max()) > 128, (case, same)
    if sel is not None:      # a ligand: bridges from the selection to the rest
        for level in LEVELS:
            lig = bp.ligand_rows(ctx.models_water_bridge_persistence(ALL, _flags(False, level)))
            assert 0 < len(lig['n_models']) < len(_hub_want(case, ALL, False, level)['n_models']), level
    ctx.close()


def _seam_check(pc, xyz, what, sift_any=ALL, expect=None):
    """Both levels, both flag values, against the loops on the oracle's bag of every model; returns the tables without
    ARP_WB_SAME_RESIDUE."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    F = len(xyz)
    h_xyz = np.zeros((F, 0, 3))
    bags = _oracle_bags(pc, xyz, h_xyz, PARAMS[2])
    ctx = _ctx_with_models(pc, xyz, h_xyz, sort_after=False)
    ctx.run_launch(*PARAMS[2])
    out = {}
    for same in (False, True):
        per = [_join(b, pc.flags, pc.res_id, sift_any, same) for b in bags]
        for level in LEVELS:
            want = loop_fold(per, pc.res_id if level == 'residue' else None)
            _same(ctx.models_water_bridge_persistence(sift_any, _flags(same, level)), want, (what, same, level))
            if not same:
                out[level] = want
    ctx.close()
    return out


def _one_water_two_partners():
    """water 0 (residue 0) at the origin, partners 1 and 2 (residues 1, 2) at 3 A on either side"""
    return tiny_complex([[0, 0, 0], [3, 0, 0], [-3, 0, 0]], flags=np.array([config.F_WATER, 0, 0], np.uint16), res_id=[0, 1, 2])


def _three_waters_two_partners():
    """partners 0 and 1 at (+-3, 0, 0); waters 2, 3, 4 on a ring of 2 A round the axis between them"""
    ring = [[0.0, 2.0 * np.cos(t), 2.0 * np.sin(t)] for t in (0.0, 2.1, 4.2)]
    return tiny_complex([[3, 0, 0], [-3, 0, 0]] + ring, flags=np.array([0, 0] + [config.F_WATER] * 3, np.uint16), res_id=[0, 1, 2, 3, 4])


def _models(pc, F, away=None):
    """F copies of the topology's coordinates, each scaled a little differently so that no two models have the same
    distances; away(f) -> the atoms moved 50 A off in model f."""
    xyz = np.stack([np.asarray(pc.xyz, np.float32) * np.float32(1.0 + 0.001 * (f % 7)) for f in range(F)])
    for f in range(F):
        for atom in (away(f) if away else ()):
            xyz[f, atom] += np.float32(50.0)
    return xyz


@pytest.mark.gpu
@pytest.mark.parametrize('F', [1, 63, 64, 65, 129])
def test_seam_one_row_whose_run_is_exactly_F_records(F):
    pc = _one_water_two_partners()
    t = _seam_check(pc, np.repeat(np.asarray(pc.xyz, np.float32)[None], F, axis=0), F)
    for level in LEVELS:
        assert len(t[level]['n_models']) == 1 and t[level]['n_models'].tolist() == [F] and t[level]['n_bridges'].tolist() == [F]
        assert t[level]['first'].tolist() == [0] and t[level]['last'].tolist() == [F - 1]


@pytest.mark.gpu
@pytest.mark.parametrize('F', [22, 43])
def test_seam_segments_of_three_waters_straddle_the_steps(F):
    pc = _three_waters_two_partners()
    t = _seam_check(pc, _models(pc, F), F)
    for level in LEVELS:
        assert t[level]['n_waters'].tolist() == [3 * F] == t[level]['n_bridges'].tolist() and t[level]['n_models'].tolist() == [F]
    assert 3 * 21 < 64 < 3 * 22 and 3 * 42 < 128 < 3 * 43      # the model open at records 63 | 64 and at 127 | 128 has records on both sides
    # one of the three waters 50 A away in every third model
    t = _seam_check(pc, _models(pc, F, lambda f: (3,) if f % 3 == 1 else ()), (F, 'a water away'))
    gone = len([f for f in range(F) if f % 3 == 1])
    for level in LEVELS:
        assert t[level]['n_waters'].tolist() == [3 * F - gone] and t[level]['n_models'].tolist() == [F]


@pytest.mark.gpu
def test_seam_models_without_the_bridge_first_last_and_in_the_middle():
    pc = _one_water_two_partners()
    F = 70
    missing = (0, 1, 33, 64, 68, 69)
    t = _seam_check(pc, _models(pc, F, lambda f: (0,) if f in missing else ()), 'missing models')
    for level in LEVELS:
        assert t[level]['n_models'].tolist() == [F - len(missing)] and t[level]['first'].tolist() == [2] and t[level]['last'].tolist() == [67]
        assert t[level]['dist_min'][0] < t[level]['dist_max'][0]


@pytest.mark.gpu
def test_seam_every_model_boundary_on_a_step_boundary():
    """One water, 16 partners in two interleaved residues: the residue pair (1, 2) has 8 x 8 = 64 rows in each of 3 models."""
    pc = seam_shells((16,), _two_interleaved_residues)
    t = _seam_check(pc, _models(pc, 3), 'interleaved')
    r = t['residue']
    assert list(zip(r['res_a'].tolist(), r['res_b'].tolist())) == [(1, 2)] and r['n_bridges'].tolist() == [192]
    assert r['n_models'].tolist() == [3] and r['n_waters'].tolist() == [3]
    assert len(t['atom']['a']) == 64 and set(t['atom']['n_models'].tolist()) == {3}


@pytest.mark.gpu
def test_seam_no_water_and_only_waters():
    for flags, what in ((0, 'no water'), (config.F_WATER, 'only waters')):
        pc = tiny_complex(_shell(12), flags=flags)
        xyz = _models(pc, 3)
        ctx = _ctx_with_models(pc, xyz, np.zeros((3, 0, 3)))
        assert ctx.run_launch(*PARAMS[2])['atom_atom'] > 0
        cnt = C.c_int64(-1)
        for fl in (0, SAME, BYRES, SAME | BYRES):
            _same(ctx.models_water_bridge_persistence(ALL, fl), bp.empty('residue' if fl & BYRES else 'atom'), (what, fl))
            assert ctx._L.arp_models_water_bridge_persistence_launch(ctx._h, ALL, fl, C.byref(cnt)) == _capi.ARP_OK and cnt.value == 0
            assert ctx._L.arp_models_water_bridge_persistence_fetch(ctx._h, 0, *([None] * 14), C.byref(cnt)) == _capi.ARP_OK and cnt.value == 0
        ctx.close()


@pytest.mark.gpu
def test_one_model_is_the_bridge_table_grouped_by_pair():
    pc, xyz, h_xyz = _hub_models()
    ctx = _ctx_with_models(pc, xyz[:1], h_xyz[:1], sort_after=False)
    ctx.run_launch(*PARAMS[0])
    for sa in (HP, ALL):
        bridges = ctx.water_bridges(sa)
        got = ctx.models_water_bridge_persistence(sa)
        _same(got, loop_fold([bridges]), hex(sa))
        U = len(got['a'])
        assert U > 0 and (got['n_models'] == 1).all() and not got['first'].any() and not got['last'].any()
        assert got['n_waters'].tobytes() == got['n_bridges'].tobytes() and int(got['n_bridges'].sum()) == len(bridges['water'])
        assert got['dist_min'].tobytes() == got['dist_max'].tobytes() and got['dist_sum'].tobytes() == got['dist_min'].astype(np.float64).tobytes()
        pairs, counts = np.unique(bridges['a'].astype(np.int64) * pc.n_atoms + bridges['b'], return_counts=True)
        assert (got['a'].astype(np.int64) * pc.n_atoms + got['b']).tolist() == pairs.tolist() and got['n_bridges'].tolist() == counts.tolist()
        _same(got, loop_fold([_join(_hub_bags('whole')[0], pc.flags, pc.res_id, sa)]), (hex(sa), 'oracle'))
    ctx.close()


def _bridge_fetch(ctx):
    """arp_water_bridges_fetch alone: (status, table)."""
    cnt = C.c_int64(-1)
    cols = {k: np.zeros(1 << 16, dt) for k, dt in zip(COLS, DTYPES)}
    rc = ctx._L.arp_water_bridges_fetch(ctx._h, 1 << 16, *(_capi._p(cols[k]) for k in COLS), C.byref(cnt))
    return rc, {k: cols[k][:max(cnt.value, 0)] for k in COLS}


@pytest.mark.gpu
def test_nothing_else_notices_a_launch():
    pc, xyz, h_xyz = _hub_models()
    F = 4
    ctx = _ctx_with_models(pc, xyz[:F], h_xyz[:F], sort_after=False)
    ctx.run_launch(*PARAMS[0])

    def everything():
        out = [{k: np.asarray(v).tobytes() for k, v in t.items()} for t in (ctx.residue_pairs(), ctx.models_persistence(), ctx.models_residue_persistence())]
        for rows in (False, True):
            ctx.set_packed_layout(rows)
            for bags in (ctx.fetch_packed()[0], ctx.fetch_packed_filtered(*contact_filter.SPECIFIC)[0]):
                out.append({name: {k: np.asarray(v).tobytes() for k, v in b.items()} for name, b in bags.items() if isinstance(b, dict)})
        ctx.set_packed_layout(False)
        return out

    before = everything()
    bridges = ctx.water_bridges(SPECIFIC)
    assert everything() == before
    ctx.run_launch(*PARAMS[0])
    assert _bridge_fetch(ctx)[0] == _capi.ARP_E_ARG
    got = {fl: ctx.models_water_bridge_persistence(SPECIFIC, fl) for fl in (0, BYRES)}
    assert len(got[0]['a']) > len(got[BYRES]['res_a']) > 0
    # the bridge table is resident as if the caller had launched it: fetchable at once, and a launch with the arguments is no work
    rc, t = _bridge_fetch(ctx)
    assert rc == _capi.ARP_OK
    _same_bridges(t, bridges, 'the bridge table after the launch')
    assert everything() == before
    _same_bridges(ctx.water_bridges(SPECIFIC), bridges, 'again')
    for fl in (0, BYRES):
        _same(ctx.models_water_bridge_persistence(SPECIFIC, fl), got[fl], ('after the others', fl))
    per = wb.split_models(bridges, pc.n_atoms)
    _same(got[0], loop_fold(per), 'atom')
    _same(got[BYRES], loop_fold(per, pc.res_id), 'residue')
    assert everything() == before
    ctx.close()


@pytest.mark.gpu
def test_contract():
    pc, xyz, h_xyz = _hub_models()
    F = 3
    xyz, h_xyz = xyz[:F], h_xyz[:F]
    L = _capi.load()
    ctx = _capi.Context(0)
    h = ctx._h
    n = C.c_int64(-1)
    launch = lambda sa=SPECIFIC, fl=0: L.arp_models_water_bridge_persistence_launch(h, sa, fl, C.byref(n))
    spec = tables.BRIDGEPERSIST_ATOM
    names = [k for k, _ in spec.columns]
    cols = tables.alloc(spec, 1 << 14, np.zeros)

    def fetch(cap=1 << 14, skip=()):
        return L.arp_models_water_bridge_persistence_fetch(h, cap, *(None if k in skip else _capi._p(cols[k]) for k in names), C.byref(n))

    def table(rows, rename=False):
        t = {k: cols[k][:rows].copy() for k in names}
        return {{'a': 'res_a', 'b': 'res_b'}.get(k, k): v for k, v in t.items()} if rename else t

    err = lambda: L.arp_last_error(h)
    # no structure; a structure that is no ensemble, before and after its pass
    assert launch() == _capi.ARP_E_ARG and fetch() == _capi.ARP_E_ARG
    ctx.set_complex(pc)
    assert launch() == _capi.ARP_E_ARG and b'no models resident' in err()
    ctx.run_launch(*PARAMS[0])
    assert launch() == _capi.ARP_E_ARG and b'no models resident' in err() and fetch() == _capi.ARP_E_ARG
    # models, but no pass
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    assert launch() == _capi.ARP_E_ARG and b'no atom-contact results' in err() and fetch() == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    # a fetch without a launch; masks and flags out of range; NULL arguments
    assert fetch() == _capi.ARP_E_ARG
    assert launch(0x8000) == _capi.ARP_E_ARG and launch(0x17FFF) == _capi.ARP_E_ARG
    assert launch(0) == _capi.ARP_E_ARG and b'no record a leg' in err()
    assert launch(SPECIFIC, 4) == _capi.ARP_E_ARG and launch(SPECIFIC, 0x80000000) == _capi.ARP_E_ARG and b'unknown flag' in err()
    assert L.arp_models_water_bridge_persistence_launch(h, SPECIFIC, 0, None) == _capi.ARP_E_ARG
    assert L.arp_models_water_bridge_persistence_launch(None, SPECIFIC, 0, C.byref(n)) == _capi.ARP_E_ARG
    assert fetch() == _capi.ARP_E_ARG and _bridge_fetch(ctx)[0] == _capi.ARP_E_ARG      # (a refused launch makes no bridge table either)
    with pytest.raises(ValueError):
        ctx.models_water_bridge_persistence(0)
    # the yardstick: the loops on the oracle's bags of these models
    bags = _hub_bags('whole')[:F]
    want = {(sa, same, level): loop_fold([_join(b, pc.flags, pc.res_id, sa, same) for b in bags], pc.res_id if level == 'residue' else None)
            for sa in (SPECIFIC, HP) for same in (False, True) for level in LEVELS}
    rows = {k: len(v['n_models']) for k, v in want.items()}
    # a launch; the second one with the same arguments returns the stored count
    assert launch() == _capi.ARP_OK and n.value == rows[SPECIFIC, False, 'atom'] > 0
    n.value = -1
    assert launch() == _capi.ARP_OK and n.value == rows[SPECIFIC, False, 'atom']
    # cap too small: ARP_E_CAPACITY with the count; then the fetch; NULL columns are skipped
    U = n.value
    n.value = -1
    assert fetch(U - 1) == _capi.ARP_E_CAPACITY and n.value == U
    assert fetch(0) == _capi.ARP_E_CAPACITY and n.value == U
    n.value = -1
    assert fetch(U) == _capi.ARP_OK and n.value == U
    _same(table(U), want[SPECIFIC, False, 'atom'], 'fetch')
    for k in names:
        cols[k][...] = 0
    skipped = ('b', 'n_waters', 'dist_sum', 'bit_models_a', 'ctype_mask_b')
    assert fetch(skip=skipped) == _capi.ARP_OK
    for k in names:
        w = want[SPECIFIC, False, 'atom'][k]
        assert cols[k][:U].tobytes() == (np.zeros_like(w) if k in skipped else w).tobytes(), k
    assert fetch(skip=names) == _capi.ARP_OK and n.value == U
    # a fetch of one column alone returns the bytes of the full fetch: the slab is laid out in the order of the arguments
    for k in names:
        cols[k].view(np.uint8)[...] = 0xA5
        assert fetch(skip=[x for x in names if x != k]) == _capi.ARP_OK
        assert cols[k][:U].tobytes() == want[SPECIFIC, False, 'atom'][k].tobytes(), k
    # other arguments remake it: every flag, the mask
    for sa, same, level in ((SPECIFIC, False, 'residue'), (SPECIFIC, True, 'residue'), (SPECIFIC, True, 'atom'), (HP, False, 'atom'), (SPECIFIC, False, 'atom')):
        assert launch(sa, _flags(same, level)) == _capi.ARP_OK and n.value == rows[sa, same, level], (sa, same, level)
        assert fetch() == _capi.ARP_OK
        _same(table(n.value, level == 'residue'), want[sa, same, level], (sa, same, level))
        rc, t = _bridge_fetch(ctx)      # ... and the bridge table is the one of the launch's arguments
        assert rc == _capi.ARP_OK and len(t['water']) == int(want[sa, same, level]['n_bridges'].sum())
    # the bridge table relaunched with another mask: the table is void, and made again from a new bridge table
    assert len(ctx.water_bridges(SPECIFIC)['water']) > 0 and fetch() == _capi.ARP_OK      # (the same table: nothing is remade)
    assert len(ctx.water_bridges(HP)['water']) > 0
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and n.value == U and fetch() == _capi.ARP_OK
    _same(table(U), want[SPECIFIC, False, 'atom'], 'after another bridge table')
    assert len(_bridge_fetch(ctx)[1]['water']) == int(want[SPECIFIC, False, 'atom']['n_bridges'].sum())
    assert len(ctx.water_bridges(SPECIFIC, SAME)['water']) > 0 and fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and n.value == U
    # voided by a new pass
    ctx.run_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and n.value == U and fetch() == _capi.ARP_OK
    # ... by the atom-atom launch alone; not by the re-run of a ring bag or a change of layout
    ctx.atom_contacts_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and n.value == U
    ctx.launch_bag('plane_plane')
    ctx.set_packed_layout(True)
    assert fetch() == _capi.ARP_OK and n.value == U
    ctx.set_packed_layout(False)
    # ... by a selection, and by new models (fewer of them: another table)
    ctx.set_selection(np.ones(pc.n_atoms * F, np.uint8))
    assert fetch() == _capi.ARP_E_ARG and launch() == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    assert launch() == _capi.ARP_OK and n.value == U
    ctx.set_models(xyz[:2], h_xyz[:2])
    assert fetch() == _capi.ARP_E_ARG and launch() == _capi.ARP_E_ARG and _bridge_fetch(ctx)[0] == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    assert launch() == _capi.ARP_OK and fetch() == _capi.ARP_OK
    _same(table(n.value), loop_fold([_join(b, pc.flags, pc.res_id, SPECIFIC) for b in bags[:2]]), 'two models')
    # a shard
    ctx.set_ownership(np.ones(pc.n_atoms * 2, np.uint8), np.arange(pc.n_atoms * 2, dtype=np.int32))
    assert launch() == _capi.ARP_E_ARG and b'shard' in err()
    ctx.close()


@pytest.mark.gpu
def test_more_models_than_the_uint16_columns_count_are_refused():
    pc = _one_water_two_partners()
    F = 65536
    ctx = _capi.Context(0)
    ctx.set_topology(pc)
    ctx.set_models(np.ascontiguousarray(np.repeat(np.asarray(pc.xyz, np.float32)[None], F, axis=0)), np.zeros((F, 0, 3)))
    cnt = C.c_int64(-1)
    assert ctx._L.arp_models_water_bridge_persistence_launch(ctx._h, ALL, 0, C.byref(cnt)) == _capi.ARP_E_ARG
    assert b'65 535' in ctx._L.arp_last_error(ctx._h)
    ctx.close()


@pytest.mark.gpu
def test_ensemble_complex_run_water_bridge_persistence(tmp_path):
    from arpeggio_amd.core import EnsembleComplex
    pc, xyz, h_xyz = _hub_models(24)
    ens = EnsembleComplex((copy.copy(pc), xyz[:8], h_xyz[:8]))
    with pytest.raises(AttributeError):
        ens.write_bridge_persistence(str(tmp_path))
    # both levels equal the Context table, and the loops on the oracle's bags (the first 8 models are the parity structure's)
    for level in LEVELS:
        for same, contacts, sa in ((False, ('hbond', 'polar'), HP), (True, None, ALL)):
            t = ens.run_water_bridge_persistence([], *PARAMS[0], contacts=contacts, same_residue=same, level=level)
            assert ens.bridge_persistence is t and ens.bridge_persistence_models == 8 and ens._results is None
            _same(t, ens._ctx.models_water_bridge_persistence(sa, _flags(same, level)), (level, same, 'context'))
            _same(t, _hub_want('whole', sa, same, level), (level, same, 'oracle'))
    t = ens.run_water_bridge_persistence([], *PARAMS[0])
    _same(t, _hub_want('whole', HP, False, 'atom'), 'defaults')
    with pytest.raises(ValueError, match='level'):
        ens.run_water_bridge_persistence([], *PARAMS[0], level='chain')
    with pytest.raises(ValueError, match='nothing_like_it'):
        ens.run_water_bridge_persistence([], *PARAMS[0], contacts=['nothing_like_it'])
    # 24 models in chunks of 8: the merge of the chunk tables
    for level in LEVELS:
        chunks = []
        for c in range(3):
            ens.set_coordinates(xyz[8 * c:8 * c + 8], h_xyz[8 * c:8 * c + 8])
            acc = ens.run_water_bridge_persistence([], *PARAMS[0], contacts=None, level=level, accumulate=c > 0)
            chunks.append(ens._ctx.models_water_bridge_persistence(ALL, _flags(False, level)))
            assert ens.bridge_persistence_models == 8 * (c + 1) and ens.bridge_persistence is acc
        _same(acc, bp.merge(bp.merge(chunks[0], chunks[1], 8), chunks[2], 16), (level, 'chunks'))
        assert int(acc['n_models'].max()) == 24 and int(acc['last'].max()) == 23
        # ... which is the one-pass table of the 24 models but for the rounding of dist_sum
        whole = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
        one = whole.run_water_bridge_persistence([], *PARAMS[0], contacts=None, level=level)
        whole._ctx.close()
        for k, _ in bp.COLUMNS[level]:
            if k != 'dist_sum':
                assert acc[k].tobytes() == one[k].tobytes(), (level, k)
        assert np.allclose(acc['dist_sum'], one['dist_sum'], rtol=1e-14, atol=0)
        # another mask, flag or level than the accumulated table's
        for kw in (dict(contacts=('hbond',), level=level), dict(contacts=None, level=level, same_residue=True),
                   dict(contacts=None, level='residue' if level == 'atom' else 'atom')):
            with pytest.raises(ValueError, match='accumulate'):
                ens.run_water_bridge_persistence([], *PARAMS[0], accumulate=True, **kw)
        assert ens.bridge_persistence is acc and ens.bridge_persistence_models == 24
        # '<id>.bridgepersist' parses back to the table
        path = ens.write_bridge_persistence(str(tmp_path))
        assert path == os.path.join(str(tmp_path), ens.id + '.bridgepersist')
        _same(_parse_csv(path, pc, level), acc, (level, 'csv'))
    ens._ctx.close()
