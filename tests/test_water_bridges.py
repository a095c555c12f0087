"""Water-mediated contacts: the atom-atom bag joined with itself on its water atoms, on the device
(arp_water_bridges_launch / arp_water_bridges_fetch, Context.water_bridges, arpeggio_amd.water_bridges,
InteractionComplex.water_bridges / write_water_bridges, EnsembleComplex.run_water_bridges).

The yardstick is never the device join: it is ``_join`` below, plain loops over a canonical atom-atom bag — the oracle's, and
the one ``fetch_packed()`` returns once that has been held against the oracle's.  Every column is compared as bytes.  No
tolerance anywhere."""
import copy
import csv
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, contact_filter, synth, water_bridges as wb
from arpeggio_amd.core import config
from helpers import tiny_complex
from test_persistence import PARAMS
from test_residue_pairs import _mask

AA = ('i', 'j', 'dist', 'sift', 'ctype')
COLS = ('water', 'a', 'b', 'dist_a', 'dist_b', 'sift_a', 'sift_b', 'ctype_a', 'ctype_b')
DTYPES = (np.int32, np.int32, np.int32, np.float32, np.float32, np.uint16, np.uint16, np.uint8, np.uint8)
BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
HP = BIT['hbond'] | BIT['polar']
ALL = 0x7FFF
SPECIFIC = 0x7FFF & ~BIT['proximal']
SAME = 1


def _join(bag, flags, res_id, sift_any, same=False):
    """The yardstick: legs by a loop over the records, bridges by a double loop over each water's sorted partners."""
    i, j = np.asarray(bag['i']).tolist(), np.asarray(bag['j']).tolist()
    sift = np.asarray(bag['sift']).tolist()
    water = ((np.asarray(flags).astype(np.int64) & config.F_WATER) != 0).tolist()
    res = np.asarray(res_id).tolist()
    legs = {}
    for r in range(len(i)):
        if (sift[r] & sift_any) == 0 or water[i[r]] == water[j[r]]:
            continue
        w, p = (i[r], j[r]) if water[i[r]] else (j[r], i[r])
        legs.setdefault(w, []).append((p, r))
    rows = []
    for w in sorted(legs):
        ps = sorted(legs[w])
        for x in range(len(ps)):
            for y in range(x + 1, len(ps)):
                if same or res[ps[x][0]] != res[ps[y][0]]:
                    rows.append((w, ps[x][0], ps[y][0], ps[x][1], ps[y][1]))
    rows = np.asarray(rows, np.int64).reshape(-1, 5)
    ra, rb = rows[:, 3], rows[:, 4]
    dist, sf, ct = np.asarray(bag['dist']), np.asarray(bag['sift']), np.asarray(bag['ctype'])
    t = {'water': rows[:, 0].astype(np.int32), 'a': rows[:, 1].astype(np.int32), 'b': rows[:, 2].astype(np.int32),
         'dist_a': dist[ra].astype(np.float32), 'dist_b': dist[rb].astype(np.float32), 'sift_a': sf[ra].astype(np.uint16),
         'sift_b': sf[rb].astype(np.uint16), 'ctype_a': ct[ra].astype(np.uint8), 'ctype_b': ct[rb].astype(np.uint8)}
    t['_runs'] = sorted(len(v) for v in legs.values())
    return t


def _bytes(t, keys=COLS):
    return {k: np.asarray(t[k]).tobytes() for k in keys}


def _same_table(got, want, what):
    assert list(got)[:9] == list(COLS), what
    for k, dt in zip(COLS, DTYPES):
        assert np.asarray(got[k]).dtype == dt and np.asarray(got[k]).shape == np.asarray(want[k]).shape, (what, k)
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (what, k)


def _hdr():
    return open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()


@functools.lru_cache(maxsize=None)
def _protein():
    pc = synth.proteinlike()
    pc.ensure_labels()
    return pc


@functools.lru_cache(maxsize=None)
def _config3():
    return synth.config3(20000)


@functools.lru_cache(maxsize=None)
def _hub():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    pc.ensure_labels()
    return pc


def _selection(pc, sel):
    return np.ones(pc.n_atoms, np.uint8) if sel is None else _mask(pc, [sel])


def _oracle_bag(pc, params=PARAMS[0], sel=None):
    """The oracle's atom-atom bag of a pass, sorted by (i, j)."""
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None if sel is None else _selection(pc, sel))
    aa = oc.atom_contacts(*params)
    assert aa.get('err', 0) == 0
    order = np.lexsort((aa['j'], aa['i']))
    return {k: np.asarray(aa[k])[order] for k in AA}


# (name) -> structure, selection, parameters, {mask: bridges without ARP_WB_SAME_RESIDUE}
PARITY = {
    'proteinlike': (_protein, None, PARAMS[0], {HP: 225, SPECIFIC: 1458, ALL: 10308}),
    'proteinlike_508': (_protein, '/A/508/', PARAMS[2], {ALL: 2884}),
    'config3_20000': (_config3, None, PARAMS[0], {HP: 3103, ALL: 234221}),
}


@functools.lru_cache(maxsize=None)
def _parity_oracle(name):
    make, sel, params, _ = PARITY[name]
    return _oracle_bag(make(), params, sel)


# ---- the seam structures: one atom flagged water at the centre of a shell of m partners at 4 A, every atom a residue of its own
def _shell(m, radius=4.0):
    k = np.arange(m) + 0.5
    phi = np.arccos(1.0 - 2.0 * k / m)
    theta = np.pi * (1.0 + 5.0 ** 0.5) * k
    return radius * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)


def seam_shells(ms, res_of_partner=None):
    """One shell of ms[c] partners around a water per cluster, clusters 30 A apart; in each cluster the water sits in the
    middle of the atom ids, so that it is i of some of its records and j of the others."""
    xyz, flags = [], []
    for c, m in enumerate(ms):
        pts = _shell(m) + np.array([30.0 * c, 0.0, 0.0])
        at = m // 2
        xyz += [pts[:at], np.array([[30.0 * c, 0.0, 0.0]]), pts[at:]]
        flags += [0] * at + [config.F_WATER] + [0] * (m - at)
    xyz = np.concatenate(xyz)
    res = np.arange(len(xyz), dtype=np.int32) if res_of_partner is None else np.asarray(res_of_partner(np.asarray(flags)), np.int32)
    return tiny_complex(xyz, flags=np.asarray(flags, np.uint16), res_id=res)


def _two_interleaved_residues(flags):
    """the water residue 0, the partners residues 1 and 2 in turn"""
    res = np.zeros(len(flags), np.int32)
    res[flags == 0] = 1 + (np.arange(int((flags == 0).sum())) & 1)
    return res


STRADDLE = (40,) + (64,) * 64      # 4136 legs: the runs of two waters lie across legs 2048 and 4096, tile boundaries of the run kernels


# ------------------------------------------------------------------------------------------------------------- CPU
def _hand_made():
    """atoms 0-2 residue 0, 3-4 residue 1, 5 residue 2; waters 6 (residue 3), 7 (residue 4), 8 (residue 5)"""
    flags = np.array([0, 0, 0, 0, 0, 0, 4, 4, 4], np.uint16)
    res_id = np.array([0, 0, 0, 1, 1, 2, 3, 4, 5], np.int32)
    H, P, V = BIT['hbond'], BIT['polar'], BIT['vdw']
    rec = [(0, 6, 2.5, H | V, 3),      # water 6: partners 0, 1 (one residue), 3, 5
           (1, 6, 3.0, P, 3),
           (3, 6, 3.5, H | P, 4),
           (5, 6, 4.5, BIT['proximal'], 4),      # no wanted bit under hbond | polar
           (6, 7, 2.75, H, 5),         # water-water: no leg
           (2, 7, 3.25, H, 4),         # water 7: one partner
           (0, 3, 4.0, H, 2),          # no water
           (4, 8, 2.0, H, 4),          # water 8: partners 4 and 5, the water is j of one record ...
           (8, 5, 2.25, P, 3)]         # ... and i of the other (a bag need not have i < j for this join)
    order = [4, 0, 8, 2, 6, 1, 7, 3, 5]                  # records in no particular order
    bag = {k: np.array([rec[r][q] for r in order], dt) for q, (k, dt) in enumerate(zip(AA, (np.int32, np.int32, np.float32, np.uint16, np.uint8)))}
    return bag, flags, res_id


def test_join_on_hand_made_bags():
    bag, flags, res_id = _hand_made()
    t = wb.join(bag, flags, res_id, HP)
    assert t['water'].tolist() == [6, 6, 8] and t['a'].tolist() == [0, 1, 4] and t['b'].tolist() == [3, 3, 5]
    assert t['dist_a'].tolist() == [2.5, 3.0, 2.0] and t['dist_b'].tolist() == [3.5, 3.5, 2.25]
    assert t['sift_a'].tolist() == [BIT['hbond'] | BIT['vdw'], BIT['polar'], BIT['hbond']]      # (whole, not masked)
    assert t['ctype_a'].tolist() == [3, 3, 4] and t['ctype_b'].tolist() == [4, 4, 3]
    s = wb.join(bag, flags, res_id, HP, same_residue=True)
    assert list(zip(s['water'].tolist(), s['a'].tolist(), s['b'].tolist())) == [(6, 0, 1), (6, 0, 3), (6, 1, 3), (8, 4, 5)]
    everything = wb.join(bag, flags, res_id, ALL)
    assert list(zip(everything['a'].tolist(), everything['b'].tolist())) == [(0, 3), (0, 5), (1, 3), (1, 5), (3, 5), (4, 5)]
    for sa in (HP, ALL, BIT['hbond'], BIT['polar'], BIT['vdw'], BIT['xbond']):
        for same in (False, True):
            _same_table(wb.join(bag, flags, res_id, sa, same_residue=same), _join(bag, flags, res_id, sa, same), (hex(sa), same))
    assert len(wb.join(bag, flags, res_id, BIT['xbond'])['water']) == 0
    _same_table(wb.empty(), _join({k: bag[k][:0] for k in AA}, flags, res_id, ALL), 'empty')
    for bad in (0, 0x8000, 0x17FFF):
        with pytest.raises(ValueError):
            wb.join(bag, flags, res_id, bad)
    assert tuple(k for k, _ in wb.COLUMNS) == COLS and tuple(dt for _, dt in wb.COLUMNS) == DTYPES


def test_join_on_random_bags_equals_the_loops():
    rs = np.random.RandomState(7)
    n = 60
    flags = np.where(rs.rand(n) < 0.25, config.F_WATER | 8, 8).astype(np.uint16)
    res_id = rs.randint(0, 12, n).astype(np.int32)
    pairs = np.array([(a, b) for a in range(n) for b in range(a + 1, n)])
    pairs = pairs[rs.rand(len(pairs)) < 0.3]
    rs.shuffle(pairs)
    bag = dict(i=pairs[:, 0].astype(np.int32), j=pairs[:, 1].astype(np.int32), dist=rs.rand(len(pairs)).astype(np.float32) * 5,
               sift=rs.randint(0, 1 << 15, len(pairs)).astype(np.uint16), ctype=rs.randint(0, 6, len(pairs)).astype(np.uint8))
    for sa in (HP, ALL, 1 << 3):
        for same in (False, True):
            want = _join(bag, flags, res_id, sa, same)
            assert len(want['water']) > 50
            _same_table(wb.join(bag, flags, res_id, sa, same_residue=same), want, (hex(sa), same))


def test_mask_names_unknown_and_empty():
    hdr = _hdr()
    for k, name in enumerate(config.SIFT_NAMES):
        assert wb.mask([name]) == wb.mask(name) == 1 << k == contact_filter.masks([name])[0]
    assert wb.mask() == wb.mask(('hbond', 'polar')) == (1 << 5) | (1 << 13) == HP
    assert wb.mask(None) == 0x7FFF == wb.SIFT_ALL
    with pytest.raises(ValueError, match='hbonds'):
        wb.mask(['hbond', 'hbonds'])
    with pytest.raises(ValueError, match='empty'):
        wb.mask([])
    assert int(re.search(r'#define\s+ARP_WB_SAME_RESIDUE\s+\(1u << (\d+)\)', hdr).group(1)) == 0 and wb.SAME_RESIDUE == 1
    assert int(re.search(r'#define\s+ARP_F_WATER\s+\(1u << (\d+)\)', hdr).group(1)) == 2 and config.F_WATER == 4
    assert 'arp_water_bridges_launch' in _capi.SYMBOLS and 'arp_water_bridges_fetch' in _capi.SYMBOLS
    assert 'int arp_water_bridges_launch(' in hdr and 'int arp_water_bridges_fetch(' in hdr


def _table(rows):
    return {k: np.array([r[q] for r in rows], dt) for q, (k, dt) in enumerate(zip(COLS, DTYPES))}


def test_splitters_ligand_bridges_and_by_residue_on_a_hand_made_table():
    SW, NW = CT['SELECTION_WATER'], CT['NON_SELECTION_WATER']
    H, P = BIT['hbond'], BIT['polar']
    # two structures / models of 10 atoms: water 9 of the first, waters 17 and 19 of the second
    t = _table([(9, 0, 4, 2.5, 3.0, H, P, SW, NW), (9, 0, 7, 2.5, 3.5, H, H | P, SW, SW), (9, 4, 7, 3.0, 3.5, P, H | P, NW, SW),
                (17, 10, 14, 2.0, 2.25, H, H, NW, NW), (19, 10, 14, 3.0, 2.0, P, H, NW, SW), (19, 10, 16, 3.0, 4.0, P, P, NW, NW)])
    for parts in (wb.split_models(t, 10), wb.split_structures(t, [0, 10, 20])):
        assert len(parts) == 2
        _same_table(parts[0], {k: t[k][:3] for k in COLS}, 'first')
        assert parts[1]['water'].tolist() == [7, 9, 9] and parts[1]['a'].tolist() == [0, 0, 0] and parts[1]['b'].tolist() == [4, 4, 6]
        assert _bytes(parts[1], COLS[3:]) == _bytes({k: t[k][3:] for k in COLS}, COLS[3:])
    three = wb.split_structures(t, [0, 10, 10, 20])
    assert [len(p['water']) for p in three] == [3, 0, 3]
    assert [len(p['water']) for p in wb.split_structures(t, [0, 10, 20, 25])] == [3, 3, 0]
    assert wb.split_models(wb.empty(), 10) == []
    with pytest.raises(ValueError):
        wb.split_structures(t, [0, 5, 20])          # water 9's partners 0 and 4 lie below 5
    with pytest.raises(ValueError):
        wb.split_structures(t, [0, 20, 10])
    lig = wb.ligand_bridges(t)
    assert list(zip(lig['water'].tolist(), lig['a'].tolist(), lig['b'].tolist())) == [(9, 0, 4), (9, 4, 7), (19, 10, 14)]
    assert lig['ctype_a'].tolist() == [SW, NW, NW] and lig['dist_b'].dtype == np.float32
    res_id = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 5, 5, 6, 7, 7, 8], np.int32)
    r = wb.by_residue(t, res_id)
    assert list(zip(r['res_a'].tolist(), r['res_b'].tolist())) == [(0, 1), (0, 2), (1, 2), (4, 5), (4, 6)]
    assert r['n_bridges'].tolist() == [1, 1, 1, 2, 1] and r['n_waters'].tolist() == [1, 1, 1, 2, 1]
    assert r['dist_min'].tolist() == [5.5, 6.0, 6.5, 4.25, 7.0] and r['dist_min'].dtype == np.float32
    assert [len(v) for v in wb.by_residue(wb.empty(), res_id).values()] == [0] * 5
    # a residue pair met in either atom order is one row
    u = _table([(9, 0, 4, 1.0, 1.0, H, H, NW, NW), (9, 5, 3, 2.0, 2.0, H, H, NW, NW)])
    assert wb.by_residue(u, res_id)['n_bridges'].tolist() == [2]


def test_csv_text_and_records_of_a_hand_made_table(tmp_path):
    pc = _hub()
    water = int(np.nonzero(pc.flags & config.F_WATER)[0][0])
    t = _table([(water, 0, 9, 2.5, np.float32(3.1), BIT['hbond'] | BIT['polar'], BIT['proximal'], CT['SELECTION_WATER'], CT['NON_SELECTION_WATER'])])
    path = tmp_path / 'x.waterbridges'
    wb.write_csv(str(path), t, pc)
    from arpeggio_amd.core import export
    lab = export.Labels(pc, pc.component_types)
    lines = path.read_text().splitlines()
    assert lines[0] == 'water,atom_bgn,atom_end,distance_bgn,distance_end,contacts_bgn,contacts_end,interacting_entities_bgn,interacting_entities_end'
    assert lines[1] == ','.join([lab.atom_macro(water), lab.atom_macro(0), lab.atom_macro(9), '2.5', '3.1', 'hbond|polar', 'proximal',
                                 'SELECTION_WATER', 'NON_SELECTION_WATER']) and len(lines) == 2
    assert wb.write_water_bridges(str(tmp_path), 'abc', t, pc) == os.path.join(str(tmp_path), 'abc.waterbridges')
    rec = wb.to_records(t, pc)
    assert len(rec) == 1 and rec[0]['type'] == 'water-bridge' and rec[0]['water'] == lab.atom_dict(water)
    assert rec[0]['bgn']['contact'] == ['hbond', 'polar'] and rec[0]['end']['interacting_entities'] == 'NON_SELECTION_WATER'
    assert rec[0]['bgn']['distance'] == 2.5 and rec[0]['end']['auth_atom_id'] == lab.atom_dict(9)['auth_atom_id']


def test_the_parity_structures_are_what_they_claim():
    """By the oracle, on the CPU: the bridges of every parity case and the longest run of legs of a water."""
    pc = _protein()
    aa = _parity_oracle('proteinlike')
    t = _join(aa, pc.flags, pc.res_id, HP)
    assert len(aa['i']) == 17938 and len(t['water']) == 225 and len(t['_runs']) == 69 and sum(t['_runs']) == 184 and t['_runs'][-1] == 11
    assert len(_join(aa, pc.flags, pc.res_id, HP, True)['water']) == 225 + 50
    assert len(_join(aa, pc.flags, pc.res_id, SPECIFIC)['water']) == 1458 and len(_join(aa, pc.flags, pc.res_id, ALL)['water']) == 10308
    t = _join(_parity_oracle('proteinlike_508'), pc.flags, pc.res_id, ALL)
    assert len(t['water']) == 2884 and t['_runs'][-1] == 65          # one full 64-step and one lane
    pc = _config3()
    aa = _parity_oracle('config3_20000')
    t = _join(aa, pc.flags, pc.res_id, ALL)
    assert len(aa['i']) == 240949 and len(t['water']) == 234221 and sum(t['_runs']) == 19987 and t['_runs'][-1] == 47
    assert (19987 + 2047) // 2048 == 10 and 19987 > 4096            # ten leg tiles, more than one tile of the radix passes
    t = _join(aa, pc.flags, pc.res_id, HP)
    assert len(t['water']) == 3103 and sum(t['_runs']) == 2273


def test_the_seam_structures_are_what_they_claim():
    for m in (1, 2, 63, 64, 65, 128, 129):
        pc = seam_shells((m,))
        t = _join(_oracle_bag(pc, PARAMS[2]), pc.flags, pc.res_id, ALL)
        assert t['_runs'] == [m] and len(t['water']) == m * (m - 1) // 2, m
    pc = seam_shells((65,), _two_interleaved_residues)
    t = _join(_oracle_bag(pc, PARAMS[2]), pc.flags, pc.res_id, ALL)
    assert t['_runs'] == [65] and len(t['water']) == 33 * 32
    pc = seam_shells(STRADDLE)
    t = _join(_oracle_bag(pc, PARAMS[2]), pc.flags, pc.res_id, ALL)
    assert t['_runs'] == sorted(STRADDLE) and sum(STRADDLE[:32]) < 2048 < sum(STRADDLE[:33]) and sum(STRADDLE[:64]) < 4096 < sum(STRADDLE) == 4136


# ------------------------------------------------------------------------------------------------------------- GPU
def _ctx(pc, params=PARAMS[0], sel=None):
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(False)
    ctx.set_complex(pc)
    if sel is not None:
        ctx.set_selection(sel)
    ctx.run_launch(*params)
    return ctx


def _full(ctx):
    """fetch_packed() in the records layout, copied out of its buffer."""
    ctx.set_packed_layout(False)
    bags, _ = ctx.fetch_packed()
    return {name: {k: np.array(v) for k, v in b.items()} for name, b in bags.items()}


def _check(ctx, bag, pc, sift_any, what):
    """Both flag values against the yardstick; returns the rows without ARP_WB_SAME_RESIDUE."""
    rows = []
    for same in (False, True):
        want = _join(bag, pc.flags, pc.res_id, sift_any, same)
        got = ctx.water_bridges(sift_any, SAME if same else 0)
        _same_table(got, want, (what, hex(sift_any), same))
        rows.append(len(want['water']))
    assert rows[0] <= rows[1]
    return rows[0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(PARITY))
def test_parity_with_the_join_of_the_canonical_bag(name):
    make, sel, params, expect = PARITY[name]
    pc = make()
    ctx = _ctx(pc, params, None if sel is None else _selection(pc, sel))
    aa = _full(ctx)['atom_atom']
    orc = _parity_oracle(name)
    assert {k: aa[k].tobytes() for k in AA} == {k: orc[k].tobytes() for k in AA}, name      # the yardstick's input, against the oracle
    for sift_any, rows in expect.items():
        assert _check(ctx, aa, pc, sift_any, name) == rows, (name, hex(sift_any))
        _same_table(ctx.water_bridges(sift_any), _join(orc, pc.flags, pc.res_id, sift_any), (name, 'oracle'))
    if sel is not None:      # a ligand: bridges from the selection to the rest
        lig = wb.ligand_bridges(ctx.water_bridges(ALL))
        assert 0 < len(lig['water']) < expect[ALL]
    ctx.close()


def _seam(pc, rows, what):
    ctx = _ctx(pc, PARAMS[2])
    aa = _full(ctx)['atom_atom']
    orc = _oracle_bag(pc, PARAMS[2])
    assert {k: aa[k].tobytes() for k in AA} == {k: orc[k].tobytes() for k in AA}, what
    assert _check(ctx, aa, pc, ALL, what) == rows, what
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('m', [1, 2, 63, 64, 65, 128, 129])
def test_seam_one_run_of_m_legs(m):
    _seam(seam_shells((m,)), m * (m - 1) // 2, m)


@pytest.mark.gpu
def test_seam_rank_skips_same_residue_pairs_across_the_carry():
    _seam(seam_shells((65,), _two_interleaved_residues), 33 * 32, 'interleaved')


@pytest.mark.gpu
def test_seam_runs_across_a_tile_boundary_of_the_legs():
    _seam(seam_shells(STRADDLE), sum(m * (m - 1) // 2 for m in STRADDLE), 'straddle')


@pytest.mark.gpu
def test_seam_no_leg_and_no_water():
    # waters, but every record with one is bare proximity: no leg under hbond
    pc = seam_shells((5, 3))
    ctx = _ctx(pc, PARAMS[2])
    aa = _full(ctx)['atom_atom']
    assert not (aa['sift'] & BIT['hbond']).any() and len(aa['i']) > 0
    assert len(_join(aa, pc.flags, pc.res_id, BIT['hbond'])['water']) == 0
    _same_table(ctx.water_bridges(BIT['hbond']), wb.empty(), 'no leg')
    _same_table(ctx.water_bridges(BIT['hbond'], SAME), wb.empty(), 'no leg, same')
    assert len(ctx.water_bridges(ALL)['water']) == 10 + 3
    ctx.close()
    # no water at all
    pc = tiny_complex(_shell(12))
    ctx = _ctx(pc, PARAMS[2])
    assert len(_full(ctx)['atom_atom']['i']) > 0
    _same_table(ctx.water_bridges(ALL, SAME), wb.empty(), 'no water')
    ctx.close()
    # only waters: every record water-water
    pc = tiny_complex(_shell(12), flags=config.F_WATER)
    ctx = _ctx(pc, PARAMS[2])
    assert (_full(ctx)['atom_atom']['ctype'] == CT['WATER_WATER']).all()
    _same_table(ctx.water_bridges(ALL, SAME), wb.empty(), 'only waters')
    ctx.close()


@pytest.mark.gpu
def test_a_batch_splits_into_the_single_runs_tables():
    pcs = [synth.proteinlike(), synth.proteinlike(seed=5, id='variant5'), synth.proteinlike(seed=9, id='variant9')]
    singles = []
    for pc in pcs:
        ctx = _ctx(pc)
        singles.append({(sa, fl): ctx.water_bridges(sa, fl) for sa in (HP, SPECIFIC) for fl in (0, SAME)})
        ctx.close()
    ctx = _capi.Context(0)
    off = ctx.set_batch(pcs)
    ctx.run_launch(*PARAMS[0])
    for (sa, fl), _ in singles[0].items():
        parts = wb.split_structures(ctx.water_bridges(sa, fl), off['atom'])
        assert len(parts) == 3
        for s in range(3):
            assert len(singles[s][(sa, fl)]['water']) > 0
            _same_table(parts[s], singles[s][(sa, fl)], (hex(sa), fl, s))
    ctx.close()


def _models(F=8):
    pc = copy.copy(_hub())
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    return pc, xyz, h_xyz


def _model_pack(pc, xyz, h_xyz, f):
    from arpeggio_amd.core import EnsembleComplex
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    packs = [ens.model_pack(k) for k in f]
    ens._ctx.close()
    return packs


@pytest.mark.gpu
def test_models_split_into_the_single_runs_tables():
    F = 8
    pc, xyz, h_xyz = _models(F)
    ctx = _capi.Context(0)
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    ctx.run_launch(*PARAMS[0])
    whole = _capi.split_models(_full(ctx), ctx._models)
    got = {sa: wb.split_models(ctx.water_bridges(sa), pc.n_atoms) for sa in (HP, SPECIFIC)}
    ctx.close()
    total = 0
    for sa, per in got.items():
        assert len(per) == F
        for f in range(F):
            _same_table(per[f], _join(whole[f]['atom_atom'], pc.flags, pc.res_id, sa), (hex(sa), f))
            total += len(per[f]['water'])
    assert total > 0
    # ... and the table of a model run alone
    for f, q in zip((0, 5), _model_pack(pc, xyz, h_xyz, (0, 5))):
        one = _ctx(q)
        _same_table(one.water_bridges(SPECIFIC), got[SPECIFIC][f], ('alone', f))
        one.close()


@pytest.mark.gpu
def test_nothing_else_notices_a_bridges_launch():
    pc, xyz, h_xyz = _models(4)
    ctx = _capi.Context(0)
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
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
    t = ctx.water_bridges(SPECIFIC)
    assert len(t['water']) > 0
    assert everything() == before
    _same_table(ctx.water_bridges(SPECIFIC), t, 'again, after the others')
    # the bridges first after a new pass, everything else after them
    ctx.run_launch(*PARAMS[0])
    _same_table(ctx.water_bridges(SPECIFIC), t, 'first after a pass')
    assert everything() == before
    ctx.close()


@pytest.mark.gpu
def test_contract():
    pc = _hub()
    L = _capi.load()
    ctx = _capi.Context(0)
    h = ctx._h
    n = C.c_int64(-1)
    launch = lambda sa=SPECIFIC, fl=0: L.arp_water_bridges_launch(h, sa, fl, C.byref(n))
    cols = {k: np.zeros(1 << 16, dt) for k, dt in zip(COLS, DTYPES)}

    def fetch(cap=1 << 16, skip=()):
        return L.arp_water_bridges_fetch(h, cap, *(None if k in skip else _capi._p(cols[k]) for k in COLS), C.byref(n))

    # no results
    assert launch() == _capi.ARP_E_ARG and fetch() == _capi.ARP_E_ARG
    ctx.set_complex(pc)
    assert launch() == _capi.ARP_E_ARG and fetch() == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    # a fetch without a launch; a mask with bits out of range; a zero mask; an unknown flag; NULL arguments
    assert fetch() == _capi.ARP_E_ARG
    assert launch(0x8000) == _capi.ARP_E_ARG and launch(0x17FFF) == _capi.ARP_E_ARG
    assert launch(0) == _capi.ARP_E_ARG and b'no record a leg' in L.arp_last_error(h)
    assert launch(SPECIFIC, 2) == _capi.ARP_E_ARG and launch(SPECIFIC, 0x80000000) == _capi.ARP_E_ARG
    assert L.arp_water_bridges_launch(h, SPECIFIC, 0, None) == _capi.ARP_E_ARG
    assert fetch() == _capi.ARP_E_ARG
    with pytest.raises(ValueError):
        ctx.water_bridges(0)
    # a launch; the second one with the same arguments returns the stored count
    aa = _full(ctx)['atom_atom']
    want = _join(aa, pc.flags, pc.res_id, SPECIFIC)
    rows = len(want['water'])
    assert launch() == _capi.ARP_OK and n.value == rows > 0
    n.value = -1
    assert launch() == _capi.ARP_OK and n.value == rows
    # other arguments remake it
    both = _join(aa, pc.flags, pc.res_id, SPECIFIC, True)
    assert launch(SPECIFIC, SAME) == _capi.ARP_OK and n.value == len(both['water']) > rows
    assert launch(HP) == _capi.ARP_OK and n.value == len(_join(aa, pc.flags, pc.res_id, HP)['water'])
    assert launch() == _capi.ARP_OK and n.value == rows
    # cap too small: ARP_E_CAPACITY with the count; then the fetch; NULL columns are skipped
    n.value = -1
    assert fetch(rows - 1) == _capi.ARP_E_CAPACITY and n.value == rows
    assert fetch(0) == _capi.ARP_E_CAPACITY and n.value == rows
    n.value = -1
    assert fetch(rows) == _capi.ARP_OK and n.value == rows
    _same_table({k: cols[k][:rows] for k in COLS}, want, 'fetch')
    for k in COLS:
        cols[k][:] = 0
    skipped = ('a', 'dist_b', 'sift_a', 'ctype_b')
    assert fetch(skip=skipped) == _capi.ARP_OK
    for k in COLS:
        assert cols[k][:rows].tobytes() == (np.zeros_like(want[k]) if k in skipped else want[k]).tobytes(), k
    assert fetch(skip=COLS) == _capi.ARP_OK and n.value == rows
    # voided by a new pass
    ctx.run_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and fetch() == _capi.ARP_OK
    # ... by a selection (and made again after the pass that follows)
    ctx.set_selection(np.ones(pc.n_atoms, np.uint8))
    assert fetch() == _capi.ARP_E_ARG and launch() == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and n.value == rows and fetch() == _capi.ARP_OK
    # ... by the atom-atom launch alone, after which it is made from that bag; not by the re-run of a ring bag or a change of layout
    ctx.atom_contacts_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and n.value == rows and fetch() == _capi.ARP_OK
    ctx.run_launch(*PARAMS[0])
    assert launch() == _capi.ARP_OK
    ctx.launch_bag('plane_plane')
    ctx.set_packed_layout(True)
    assert fetch() == _capi.ARP_OK and n.value == rows
    ctx.set_packed_layout(False)
    # ... by a structure upload
    ctx.set_complex(pc)
    assert fetch() == _capi.ARP_E_ARG and launch() == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    assert launch() == _capi.ARP_OK and n.value == rows
    # a shard
    ctx.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    assert launch() == _capi.ARP_E_ARG and b'shard' in L.arp_last_error(h)
    ctx.close()


def _parse_csv(path, pc):
    from arpeggio_amd.core import export
    lab = export.Labels(pc, pc.component_types)
    atom = {lab.atom_macro(i): i for i in range(pc.n_atoms)}
    assert len(atom) == pc.n_atoms
    with open(path, newline='') as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == wb.CSV_HEADER
    bits = lambda s: sum(BIT[x] for x in s.split('|')) if s else 0
    return _table([(atom[r[0]], atom[r[1]], atom[r[2]], np.float32(r[3]), np.float32(r[4]), bits(r[5]), bits(r[6]), CT[r[7]], CT[r[8]])
                   for r in rows[1:]])


@pytest.mark.gpu
def test_interaction_complex_water_bridges(tmp_path):
    from arpeggio_amd.core import InteractionComplex
    pc = _protein()
    ic = InteractionComplex(copy.copy(pc))
    with pytest.raises(AttributeError):
        ic.water_bridges()
    ic.run_arpeggio(['/A/508/'], *PARAMS[0])
    aa = {k: np.asarray(ic._bags['atom_atom'][k]) for k in AA}
    t = ic.water_bridges()
    _same_table(t, _join(aa, pc.flags, pc.res_id, HP), 'default')
    assert len(t['water']) > 0
    _same_table(ic.water_bridges(contacts=None, same_residue=True), _join(aa, pc.flags, pc.res_id, ALL, True), 'all, same')
    _same_table(ic.water_bridges(contacts='hbond'), _join(aa, pc.flags, pc.res_id, BIT['hbond']), 'hbond')
    with pytest.raises(ValueError, match='nothing_like_it'):
        ic.water_bridges(contacts=['nothing_like_it'])
    path = ic.write_water_bridges(str(tmp_path))
    assert path == os.path.join(str(tmp_path), ic.id + '.waterbridges')
    _same_table(_parse_csv(path, pc), t, 'csv')
    _same_table(_parse_csv(ic.write_water_bridges(str(tmp_path), contacts=None), pc), _join(aa, pc.flags, pc.res_id, ALL), 'csv, all')
    # a contact filter changes the fetched records, not the resident bag the bridges are made from
    ic.set_contact_filter(contacts=['ionic'])
    ic.run_arpeggio(['/A/508/'], *PARAMS[0])
    assert len(ic._bags['atom_atom']['i']) < len(aa['i'])
    _same_table(ic.water_bridges(), t, 'with a contact filter')


@pytest.mark.gpu
def test_ensemble_complex_run_water_bridges():
    from arpeggio_amd.core import EnsembleComplex
    F = 4
    pc, xyz, h_xyz = _models(F)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    t = ens.run_water_bridges([], *PARAMS[0], contacts=None)
    assert list(t) == list(COLS) + ['model'] and t['model'].dtype == np.int32
    assert np.all(np.diff(t['model']) >= 0) and set(t['model'].tolist()) == set(range(F))
    packs = [ens.model_pack(f) for f in range(F)]
    for f in range(F):
        one = _ctx(packs[f])
        m = t['model'] == f
        _same_table({k: t[k][m] for k in COLS}, one.water_bridges(ALL), f)
        one.close()
    d = ens.run_water_bridges([], *PARAMS[0])
    assert len(d['water']) <= len(t['water']) and list(d) == list(t)
    per_model = [wb.by_residue({k: d[k][d['model'] == f] for k in COLS}, pc.res_id) for f in range(F)]
    assert len(per_model) == F
