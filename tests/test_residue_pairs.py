"""The residue-residue contact table of a pass, reduced on the device (arp_residue_pairs_launch / _fetch,
Context.residue_pairs, InteractionComplex.residue_contacts, EnsembleComplex.run_residue_contacts, arpeggio_amd.residue_pairs).

The yardstick is never the device reduction: it is ``reference_table`` below — a plain NumPy fold of bags that did not come
through the new code (the bags ``fetch_packed`` returns, and the oracle's).  Every comparison is exact: integers equal,
``dist_min`` compared as bytes.  No tolerance anywhere."""
import copy
import csv
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, batch, residue_pairs, synth
from helpers import tiny_complex
from test_models import _same
from test_persistence import PARAMS

# the two id columns of every bag and the residue table each indexes ('a' = res_id, 'r' = ring_res, 'm' = amide_res), in the
# order of plane_count
PLANE_BAGS = (('atom_plane', 'atom', 'ring', 'a', 'r'), ('plane_plane', 'bgn', 'end', 'r', 'r'),
              ('group_group', 'bgn', 'end', 'm', 'm'), ('group_plane', 'amide', 'ring', 'm', 'r'))


def reference_table(bags, res_id, ring_res, amide_res):
    """The residue-pair table of the five bags of one pass (any of them may be missing = empty): every record's two residues
    as an unordered pair, records with a residue of -1 dropped, np.unique on res_a * nres + res_b, then np.add.at /
    np.minimum.at / np.bitwise_or.at per column."""
    tab = {'a': np.asarray(res_id, np.int64), 'r': np.asarray(ring_res, np.int64), 'm': np.asarray(amide_res, np.int64)}
    nres = max([int(t.max()) + 1 for t in tab.values() if len(t)] + [1])
    aa = bags.get('atom_atom')
    parts = []      # (class, res of first id, res of second id)
    if aa is not None and len(aa['j']):
        parts.append((0, tab['a'][np.asarray(aa['i'])], tab['a'][np.asarray(aa['j'])]))
    for m, (name, ka, kb, ta, tb) in enumerate(PLANE_BAGS):
        b = bags.get(name)
        if b is not None and len(b[ka]):
            parts.append((m + 1, tab[ta][np.asarray(b[ka])], tab[tb][np.asarray(b[kb])]))
    keys = {}
    for cls, ra, rb in parts:
        keep = (ra >= 0) & (rb >= 0)
        keys[cls] = (keep, np.minimum(ra, rb)[keep] * nres + np.maximum(ra, rb)[keep])
    uk = np.unique(np.concatenate([k for _, k in keys.values()])) if keys else np.zeros(0, np.int64)
    U = len(uk)
    n = np.zeros(U, np.int64)
    dmin = np.full(U, np.inf, np.float32)
    bits = np.zeros((U, 15), np.int64)
    ct = np.zeros(U, np.uint8)
    planes = np.zeros((U, 4), np.int64)
    for cls, (keep, k) in keys.items():
        idx = np.searchsorted(uk, k)
        if cls == 0:
            np.add.at(n, idx, 1)
            np.minimum.at(dmin, idx, np.asarray(aa['dist'], np.float32)[keep])
            np.add.at(bits, idx, (np.asarray(aa['sift']).astype(np.int64)[keep][:, None] >> np.arange(15)) & 1)
            np.bitwise_or.at(ct, idx, (1 << np.asarray(aa['ctype']).astype(np.int64)[keep]).astype(np.uint8))
        else:
            np.add.at(planes[:, cls - 1], idx, 1)
    return dict(res_a=(uk // nres).astype(np.int32), res_b=(uk % nres).astype(np.int32), n_contacts=n.astype(np.uint32), dist_min=dmin,
                bit_count=bits.astype(np.uint32), ctype_mask=ct, plane_count=planes.astype(np.uint32))


def _aa(i, j, dist, sift, ctype):
    return dict(i=np.array(i, np.int32), j=np.array(j, np.int32), dist=np.array(dist, np.float32), sift=np.array(sift, np.uint16),
                ctype=np.array(ctype, np.uint8))


def _ids(ka, a, kb, b):
    return {ka: np.array(a, np.int32), kb: np.array(b, np.int32)}


def _oracle_pass(pc, params=PARAMS[0], sel=None):
    """The oracle's five bags of one pass."""
    oc = oracle.OracleComplex(pc)
    oc.make_selection(sel)
    aa = oc.atom_contacts(*params)
    assert aa.get('err', 0) == 0
    return dict(atom_atom=aa, atom_plane=oc.atom_plane(), plane_plane=oc.plane_plane(), group_group=oc.group_group(),
                group_plane=oc.group_plane())


def _ref(pc, bags):
    return reference_table(bags, pc.res_id, pc.ring_res, pc.amide_res)


def _mask(pc, sel):
    from arpeggio_amd.core import utils
    m = np.zeros(pc.n_atoms, np.uint8)
    m[utils.selection_parser(sel, pc) if sel else np.arange(pc.n_atoms)] = 1
    return m


# ---- the structures of the seam tests: non-polypeptide residues (no sequence-adjacency filter), every atom within 5 A of every other
def _cluster(n, spacing=1.2):
    g = np.array([(x, y, z) for x in range(3) for y in range(4) for z in range(2)], np.float64)[:n] * spacing
    assert n <= 24
    return g


def seam_long_run():
    """(a) two residues of 12 interleaved atoms each: 144 records in ONE row — two full 64-wide steps and a partial third."""
    return tiny_complex(_cluster(24), res_id=[k & 1 for k in range(24)])


def seam_orientation():
    """(b) res_id = [1, 0, 1, 0, ...] over 10 atoms: atom order and residue order disagree."""
    return tiny_complex(_cluster(10), res_id=[1 - (k & 1) for k in range(10)])


def seam_single_residue():
    """(c) one residue: no inter-residue pair, no record, no row."""
    return tiny_complex(_cluster(8), res_id=[0] * 8)


def seam_sentinel_tie():
    """Four residues (nres - 1 = 3 is all ones in its two bits), residue 3 with two stacked rings and an amide between them:
    an intra-residue row (3, 3) — its key all ones in the bits of a pair — with a plane-plane record and two group-plane
    records.  A second amide WITHOUT a residue is stacked on the first: its group-group records are left out, and they sit
    between the plane-plane and the group-plane records of the row when the sort begins.  A ring or amide without a residue
    is in no selection set of a pass (I:1416-1437), so the case installs its sets itself: everything selected."""
    xyz = np.array([(0, 0, 0), (1.5, 0, 0), (0, 1.5, 0), (1.5, 1.5, 0), (0.7, 0.7, 3.5), (0.7, 0.7, 7.0)], np.float64)
    rc = np.array([(0.7, 0.7, 1.0), (0.7, 0.7, 4.6)])
    rn = np.array([(0.0, 0.0, 1.0)] * 2)
    ac = np.array([(0.7, 0.7, 2.8), (0.7, 0.7, 6.0)], np.float32)
    an = np.array([(0.0, 0.0, 1.0)] * 2, np.float32)
    return tiny_complex(xyz, res_id=[0, 1, 2, 3, 3, 3], rings=(rc, rn, np.array([3, 3], np.int32)), amides=(ac, an, np.array([3, -1], np.int32)))


def _oracle_everything_selected(pc, params=PARAMS[0]):
    """The oracle's five bags with every atom, ring and amide in both selection sets (an installed selection state)."""
    one = np.ones(pc.n_atoms, np.uint8)
    oc = oracle.OracleComplex(pc, one, one)
    for m in (oc.ring_sel, oc.ring_plus, oc.amide_sel, oc.amide_plus):
        m[:] = 1
    return dict(atom_atom=oc.atom_contacts(*params), atom_plane=oc.atom_plane(), plane_plane=oc.plane_plane(), group_group=oc.group_group(),
                group_plane=oc.group_plane())


PLANES_CASES = (9, 8)


@functools.lru_cache(maxsize=None)
def planes_packs():
    """Cases of helpers.random_ring_and_amide_sets (atoms with a few hundred random rings and amides whose residues are drawn
    from the atoms' residues or -1): case 9 — by the oracle, on the CPU — fills all four ring / amide bags with hundreds of
    records, with plane-only and intra-residue rows; case 8 has 128 residues, a power of two.  {case: (pack, selection)}."""
    from helpers import random_ring_and_amide_sets
    return {case: (pc, sel) for case, pc, sel in random_ring_and_amide_sets(max(PLANES_CASES) + 1) if case in PLANES_CASES}


@functools.lru_cache(maxsize=None)
def _protein():
    return synth.proteinlike()


@functools.lru_cache(maxsize=None)
def _hub():
    return synth.proteinlike(n_res=40, seed=21, n_waters=20)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_reference_table_on_hand_made_bags():
    """Six atoms in residues [2, 0, 1, 0, 3, 1]; rings of residues [1, 1, -1, 4]; amides of residues [4, 0]."""
    H, V, P = 1 << 5, 1 << 3, 1 << 4
    res_id, ring_res, amide_res = [2, 0, 1, 0, 3, 1], [1, 1, -1, 4], [4, 0]
    bags = dict(
        # (0, 1): residues (2, 0) -> oriented pair, row (0, 2); (1, 2) and (3, 5): both (0, 1); (0, 3): (2, 0) again; (2, 4): (1, 3)
        atom_atom=_aa([0, 1, 3, 0, 2], [1, 2, 5, 3, 4], [3.0, 4.5, 2.5, 3.25, 4.0], [H | P, V, P, P, V | P], [2, 1, 2, 0, 2]),
        # atom 4 (res 3) - ring 0 (res 1): joins row (1, 3); atom 0 - ring 2 (no residue): dropped
        atom_plane=_ids('atom', [4, 0], 'ring', [0, 2]),
        # rings 0, 1 (both res 1): intra-residue row (1, 1); ring 1 - ring 3 (1, 4): plane-only row; ring 2 - ring 3: dropped
        plane_plane=_ids('bgn', [0, 1, 2], 'end', [1, 3, 3]),
        group_group=_ids('bgn', [0, 1], 'end', [1, 0]),          # amides (4, 0) and (0, 4): one row (0, 4), counted twice
        group_plane=_ids('amide', [0, 1], 'ring', [3, 2]))       # amide 0 (4) - ring 3 (4): row (4, 4); amide 1 - ring 2: dropped
    t = reference_table(bags, res_id, ring_res, amide_res)
    assert list(zip(t['res_a'].tolist(), t['res_b'].tolist())) == [(0, 1), (0, 2), (0, 4), (1, 1), (1, 3), (1, 4), (4, 4)]
    assert t['n_contacts'].tolist() == [2, 2, 0, 0, 1, 0, 0]
    assert t['dist_min'].tolist() == [2.5, 3.0, np.inf, np.inf, 4.0, np.inf, np.inf]
    assert t['bit_count'][0].tolist() == [0, 0, 0, 1, 1] + [0] * 10                   # vdw once, proximal once
    assert t['bit_count'][1].tolist() == [0, 0, 0, 0, 2, 1] + [0] * 9                 # proximal twice, hbond once
    assert t['bit_count'][4].tolist() == [0, 0, 0, 1, 1] + [0] * 10
    assert not t['bit_count'][[2, 3, 5, 6]].any()
    assert t['ctype_mask'].tolist() == [(1 << 1) | (1 << 2), (1 << 2) | (1 << 0), 0, 0, 1 << 2, 0, 0]
    assert t['plane_count'].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 2, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]
    assert [t[k].dtype for k, _ in residue_pairs.COLUMNS] == [np.dtype(dt) for _, dt in residue_pairs.COLUMNS]
    assert t['bit_count'].shape == (7, 15) and t['plane_count'].shape == (7, 4)
    # the order of the records cannot show
    rs = np.random.RandomState(3)
    o = rs.permutation(5)
    shuffled = dict(bags, atom_atom={k: v[o] for k, v in bags['atom_atom'].items()})
    _same(reference_table(shuffled, res_id, ring_res, amide_res), t, 'shuffled')
    # no record at all, and nothing but dropped records
    _same(reference_table({}, res_id, ring_res, amide_res), residue_pairs.empty(), 'no bags')
    _same(reference_table(dict(atom_plane=_ids('atom', [0], 'ring', [2])), res_id, ring_res, amide_res), residue_pairs.empty(), 'dropped')


def test_the_seam_structures_are_what_they_claim():
    """By the oracle, on the CPU: the figures the GPU seam cases lean on."""
    a = seam_long_run()
    bags = _oracle_pass(a)
    t = _ref(a, bags)
    assert t['n_contacts'].tolist() == [144] and (t['res_a'][0], t['res_b'][0]) == (0, 1)      # > 128, and 144 = 64 + 64 + 16
    b = seam_orientation()
    bags = _oracle_pass(b)
    i, j = bags['atom_atom']['i'], bags['atom_atom']['j']
    assert np.all(i < j) and int((b.res_id[i] > b.res_id[j]).sum()) == 15 and int((b.res_id[i] < b.res_id[j]).sum()) == 10
    t = _ref(b, bags)
    assert t['n_contacts'].tolist() == [25] and (t['res_a'][0], t['res_b'][0]) == (0, 1)
    c = seam_single_residue()
    bags = _oracle_pass(c)
    assert len(bags['atom_atom']['i']) == 0 and len(_ref(c, bags)['res_a']) == 0
    d = seam_sentinel_tie()
    bags = _oracle_everything_selected(d)
    t = _ref(d, bags)
    assert d.n_residues == 4
    left_out = d.amide_res[bags['group_group']['bgn']] < 0
    assert len(left_out) == 2 and np.all(left_out | (d.amide_res[bags['group_group']['end']] < 0))      # both orders of the amide pair
    row = (t['res_a'] == 3) & (t['res_b'] == 3)
    assert row.sum() == 1 and t['plane_count'][row][0].tolist() == [0, 1, 0, 2] and t['plane_count'][:, 2].sum() == 0


def test_the_parity_structure_has_runs_across_tile_boundaries():
    """proteinlike (5.9 k atoms), whole structure, 5.0 A, by the oracle: more records than one tile of the run detection (2048),
    and rows whose records straddle a multiple of 2048 in the sorted order."""
    pc = _protein()
    t = _ref(pc, _oracle_pass(pc))
    per_row = t['n_contacts'].astype(np.int64) + t['plane_count'].astype(np.int64).sum(axis=1)
    ends = np.cumsum(per_row)
    starts = ends - per_row
    assert ends[-1] > 2048
    straddle = (starts // 2048) != ((ends - 1) // 2048)
    assert int(straddle.sum()) >= 1
    print('records', int(ends[-1]), 'rows', len(per_row), 'rows across a tile boundary', int(straddle.sum()))


def test_the_planes_structure_has_plane_only_and_intra_residue_rows():
    pc, _ = planes_packs()[9]
    assert planes_packs()[8][0].n_residues == 128
    t = _ref(pc, _oracle_pass(pc))
    plane_only = (t['n_contacts'] == 0) & (t['plane_count'].sum(axis=1) > 0)
    intra = t['res_a'] == t['res_b']
    assert plane_only.any() and intra.any()
    assert np.all(t['plane_count'].sum(axis=0) > 0)      # every one of the four bags contributes
    print('rows', len(t['res_a']), 'plane-only', int(plane_only.sum()), 'intra-residue', int(intra.sum()),
          'records per bag', t['plane_count'].sum(axis=0).tolist())


def _three_tables():
    rs = np.random.RandomState(5)
    sizes = (7, 1, 5)
    tabs = []
    for nres in sizes:
        k = rs.randint(8, 30)
        bags = dict(atom_atom=_aa(rs.randint(0, nres, k), rs.randint(0, nres, k), rs.rand(k) * 5, rs.randint(0, 1 << 15, k), rs.randint(0, 7, k)),
                    plane_plane=_ids('bgn', rs.randint(0, nres, 6), 'end', rs.randint(0, nres, 6)))
        ident = np.arange(nres)
        tabs.append(reference_table(bags, ident, ident, ident))
    return sizes, tabs


def test_split_at_every_boundary_of_a_three_structure_table():
    sizes, tabs = _three_tables()
    off = np.concatenate([[0], np.cumsum(sizes)])
    big = {k: np.concatenate([t[k] + (off[s] if k in ('res_a', 'res_b') else 0) for s, t in enumerate(tabs)]).astype(dt)
           for k, dt in residue_pairs.COLUMNS}
    assert all(len(t['res_a']) > 0 for t in tabs)
    parts = residue_pairs.split(big, off)
    assert len(parts) == 3
    for s in range(3):
        _same(parts[s], tabs[s], s)
        assert list(parts[s]) == [k for k, _ in residue_pairs.COLUMNS]
    # a structure without rows, at either end and in the middle
    for drop in range(3):
        keep = ~((big['res_a'] >= off[drop]) & (big['res_a'] < off[drop + 1]))
        parts = residue_pairs.split({k: v[keep] for k, v in big.items()}, off)
        for s in range(3):
            _same(parts[s], residue_pairs.empty() if s == drop else tabs[s], (drop, s))
    # one structure: the table itself; no structure: nothing
    _same(residue_pairs.split(tabs[0], [0, sizes[0]])[0], tabs[0], 'single')
    assert residue_pairs.split(big, [0]) == []
    # offsets that do not fit the table
    with pytest.raises(ValueError):
        residue_pairs.split(big, [0, 3, off[3]])
    with pytest.raises(ValueError):
        residue_pairs.split(big, [0, 5, 2])


def test_records_and_csv_on_a_small_table(tmp_path):
    from arpeggio_amd.core import export
    pc = _hub()
    pc.ensure_labels()
    H, P = 1 << 5, 1 << 4
    a0, a1, a2 = (int(np.nonzero(pc.res_id == r)[0][0]) for r in (0, 3, 5))
    bags = dict(atom_atom=_aa([a0, a0], [a1, a1 + 1], [3.5, 3.0], [H | P, P], [2, 1]), plane_plane=_ids('bgn', [0], 'end', [0]))
    ring_res = np.array([5], np.int32)
    t = reference_table(bags, pc.res_id, ring_res, np.zeros(0, np.int32))
    assert list(zip(t['res_a'].tolist(), t['res_b'].tolist())) == [(0, 3), (5, 5)]
    lab = export.Labels(pc, pc.component_types)
    rec = residue_pairs.to_records(t, pc)
    assert len(rec) == 2
    want = lab.atom_dict(a0)
    del want['auth_atom_id']
    assert rec[0]['bgn'] == want and rec[0]['end']['auth_seq_id'] == int(pc.res_seq[3]) and rec[1]['bgn'] == rec[1]['end']
    assert rec[0]['n_contacts'] == 2 and rec[0]['distance_min'] == 3.0 and rec[0]['contact'] == {'proximal': 2, 'hbond': 1}
    assert rec[0]['interacting_entities'] == ['INTRA_SELECTION', 'INTER'] and rec[0]['planes'] == {}
    assert rec[1]['n_contacts'] == 0 and rec[1]['distance_min'] is None and rec[1]['planes'] == {'plane_plane': 1} and rec[1]['contact'] == {}
    assert json.loads(json.dumps(rec)) == rec
    path = tmp_path / 'small.csv'
    residue_pairs.write_csv(str(path), t, pc)
    with open(path, newline='') as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == residue_pairs.CSV_HEADER and len(rows[0]) == 4 + 15 + 4 + 1 and len(rows) == 3
    assert rows[1][:4] == [lab.res_macro[0], lab.res_macro[3], '2', '3.0'] and rows[1][-1] == 'INTRA_SELECTION|INTER'
    assert [int(x) for x in rows[1][4:19]] == t['bit_count'][0].tolist() and [int(x) for x in rows[2][19:23]] == [0, 1, 0, 0]
    assert rows[2][:4] == [lab.res_macro[5], lab.res_macro[5], '0', ''] and rows[2][-1] == ''
    assert os.path.basename(residue_pairs.write_residue_contacts(str(tmp_path), 'x1', t, pc)) == 'x1.rescontacts'
    assert (tmp_path / 'x1.rescontacts').read_bytes() == path.read_bytes()


def test_residue_contacts_before_a_run_raises():
    from arpeggio_amd.core import InteractionComplex
    ic = InteractionComplex(_hub())
    with pytest.raises(AttributeError, match='no results yet'):
        ic.residue_contacts()
    with pytest.raises(AttributeError, match='no results yet'):
        ic.write_residue_contacts('.')


def test_constants_and_columns_match_the_header():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert int(re.search(r'#define\s+ARP_RESPAIR_BITS\s+(\d+)', hdr).group(1)) == _capi.RESPAIR_BITS == residue_pairs.N_BITS == 15
    assert _capi.RESPAIR_COLUMNS == residue_pairs.COLUMNS
    assert tuple(b[0] for b in PLANE_BAGS) == residue_pairs.PLANE_BAGS
    assert 'arp_residue_pairs_launch' in _capi.SYMBOLS and 'arp_residue_pairs_fetch' in _capi.SYMBOLS


# ------------------------------------------------------------------------------------------------------------- GPU
def _ctx(pc, sort_after=True):
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(sort_after)
    ctx.set_complex(pc)
    return ctx


def _selections(pc):
    """Whole structure, one residue by its selector, one residue range."""
    r = pc.n_residues // 3
    rng = np.zeros(pc.n_atoms, np.uint8)
    rng[(pc.res_id >= r) & (pc.res_id < r + 12)] = 1
    one = ['/A/508/'] if any(ch == 'A' and int(sq) == 508 for ch, sq in zip(pc.res_chain, pc.res_seq)) else \
          ['/%s/%d/' % (pc.res_chain[r], int(pc.res_seq[r]))]
    return (('whole', None), (one[0], _mask(pc, one)), ('range', rng))


@pytest.mark.gpu
@pytest.mark.parametrize('make', [_hub, _protein], ids=['proteinlike40', 'proteinlike'])
def test_table_equals_the_fold_of_the_fetched_and_of_the_oracles_bags(make):
    pc = make()
    pc.ensure_labels()
    ctx = _ctx(pc)
    rows = 0
    for params in PARAMS:
        for name, sel in _selections(pc):
            what = (pc.id, params, name)
            ctx.set_selection(np.ones(pc.n_atoms, np.uint8) if sel is None else sel)
            ctx.run_launch(*params)
            got = ctx.residue_pairs()
            bags, _ = ctx.fetch_packed()
            want = _ref(pc, bags)
            print(what, 'rows', len(want['res_a']), 'records', int(want['n_contacts'].sum()), '+', want['plane_count'].sum(axis=0).tolist())
            _same(got, want, what + ('fetched',))
            _same(got, _ref(pc, _oracle_pass(pc, params, sel)), what + ('oracle',))
            _same(ctx.residue_pairs(), want, what + ('after the fetch',))
            rows += len(want['res_a'])
            if make is _protein and params == PARAMS[0] and sel is None:
                assert int(want['n_contacts'].sum()) > 2048
    assert rows > 0
    ctx.close()


@pytest.mark.gpu
def test_kernel_seams():
    for name, make, rows in (('long run', seam_long_run, 1), ('orientation', seam_orientation, 1), ('single residue', seam_single_residue, 0)):
        pc = make()
        ctx = _ctx(pc)
        ctx.run_launch(*PARAMS[0])
        got = ctx.residue_pairs()
        bags, _ = ctx.fetch_packed()
        want = _ref(pc, bags)
        _same(got, want, (name, 'fetched'))
        _same(got, _ref(pc, _oracle_pass(pc)), (name, 'oracle'))
        assert len(got['res_a']) == rows, name
        if name == 'long run':
            assert int(want['n_contacts'].max()) > 128 and int(want['n_contacts'].max()) % 64 != 0
        if name == 'orientation':
            i, j = np.asarray(bags['atom_atom']['i']), np.asarray(bags['atom_atom']['j'])
            assert int((pc.res_id[i] > pc.res_id[j]).sum()) > 0 and int((pc.res_id[i] < pc.res_id[j]).sum()) > 0
        if name == 'single residue':
            cnt = C.c_int64(-1)
            assert ctx._L.arp_residue_pairs_launch(ctx._h, C.byref(cnt)) == _capi.ARP_OK and cnt.value == 0
            assert ctx._L.arp_residue_pairs_fetch(ctx._h, 0, *([None] * 7), C.byref(cnt)) == _capi.ARP_OK and cnt.value == 0
            _same(got, residue_pairs.empty(), name)
        ctx.close()


@pytest.mark.gpu
def test_left_out_records_do_not_split_the_row_they_tie_with():
    """seam_sentinel_tie with an installed selection state and the five bags launched one by one (all five valid: a complete
    pass): the group-group records of the amide without a residue are left out, and the row (3, 3) stays ONE row."""
    pc = seam_sentinel_tie()
    ctx = _ctx(pc)
    one = np.ones(pc.n_atoms, np.uint8)
    ctx.set_selection_state(one, one, np.ones(pc.n_rings, np.uint8), np.ones(pc.n_rings, np.uint8), np.ones(pc.n_amides, np.uint8),
                            np.ones(pc.n_amides, np.uint8))
    ctx.atom_contacts_launch(*PARAMS[0])
    with pytest.raises(ValueError, match='complete pass'):
        ctx.residue_pairs()
    bags = {name: (ctx.launch_bag(name), ctx.fetch_bag(name))[1] for name, *_ in PLANE_BAGS}
    bags['atom_atom'] = ctx.atom_contacts_fetch(64)
    got = ctx.residue_pairs()
    assert int((pc.amide_res[bags['group_group']['bgn']] < 0).sum()) + int((pc.amide_res[bags['group_group']['end']] < 0).sum()) == 2
    _same(got, _ref(pc, bags), 'fetched')
    _same(got, _ref(pc, _oracle_everything_selected(pc)), 'oracle')
    row = (got['res_a'] == 3) & (got['res_b'] == 3)
    assert row.sum() == 1 and got['plane_count'][row][0].tolist() == [0, 1, 0, 2]
    ctx.close()


@pytest.mark.gpu
def test_planes():
    for case in PLANES_CASES:
        pc, part = planes_packs()[case]
        ctx = _ctx(pc)
        for name, sel in (('whole', None), ('partial', part if part is not None else (np.arange(pc.n_atoms) % 3 == 0).astype(np.uint8))):
            ctx.set_selection(np.ones(pc.n_atoms, np.uint8) if sel is None else sel)
            counts = ctx.run_launch(*PARAMS[0])
            got = ctx.residue_pairs()
            bags, _ = ctx.fetch_packed()
            want = _ref(pc, bags)
            _same(got, want, (name, 'fetched'))
            _same(got, _ref(pc, _oracle_pass(pc, PARAMS[0], sel)), (name, 'oracle'))
            kept = [int(((np.asarray(tab_a)[bags[b][ka]] >= 0) & (np.asarray(tab_b)[bags[b][kb]] >= 0)).sum())
                    for (b, ka, kb, _, _), (tab_a, tab_b) in zip(PLANE_BAGS, ((pc.res_id, pc.ring_res), (pc.ring_res, pc.ring_res),
                                                                              (pc.amide_res, pc.amide_res), (pc.amide_res, pc.ring_res)))]
            assert got['plane_count'].sum(axis=0).tolist() == kept and all(kept[m] <= counts[b[0]] for m, b in enumerate(PLANE_BAGS))
            if sel is None and case == 9:
                assert ((got['n_contacts'] == 0) & (got['plane_count'].sum(axis=1) > 0)).any() and (got['res_a'] == got['res_b']).any()
        ctx.close()


@pytest.mark.gpu
def test_batch_table_splits_into_the_single_run_tables():
    pcs = [synth.proteinlike(n_res=40, seed=21, n_waters=20), planes_packs()[9][0], synth.proteinlike(n_res=60, seed=12, n_waters=20)]
    singles = []
    for pc in pcs:
        ctx = _ctx(pc)
        ctx.run_launch(*PARAMS[0])
        singles.append(ctx.residue_pairs())
        _same(singles[-1], _ref(pc, _oracle_pass(pc)), ('single', pc.id))
        ctx.close()
    big, off = batch.concat_complexes(pcs)
    ctx = _ctx(big)
    ctx.declare_batch(off)
    ctx.run_batch(*PARAMS[0], fetch=False)
    t = ctx.residue_pairs()
    # no row joins two structures
    sa = np.searchsorted(off['residue'], t['res_a'], side='right')
    sb = np.searchsorted(off['residue'], t['res_b'], side='right')
    assert np.array_equal(sa, sb) and len(np.unique(sa)) == 3
    parts = residue_pairs.split(t, off['residue'])
    for s in range(3):
        _same(parts[s], singles[s], ('batch', s))
    ctx.close()


@pytest.mark.gpu
def test_models_tables_and_the_persistence_table_beside_them():
    from arpeggio_amd.core import EnsembleComplex
    pc = copy.copy(_hub())
    pc.ensure_labels()
    F = 8
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    got = ens.run_residue_contacts([], *PARAMS[0])
    assert len(got) == F and ens._results is None
    differ = 0
    for f in range(F):
        q = ens.model_pack(f)
        want = _ref(q, _oracle_pass(q))
        _same(got[f], want, ('model', f))
        differ += int(len(want['res_a']) != len(got[0]['res_a']) or not np.array_equal(want['n_contacts'], got[0]['n_contacts']))
    assert differ > 0      # (the jitter shows: the models do not all have model 0's table)
    # the same pass through the context: per-model fold of the fetched bags, and the persistence table before and after
    ctx = ens._ctx
    before = ctx.models_persistence()
    t = ctx.residue_pairs()
    after = ctx.models_persistence()
    _same(before, after, 'persistence')
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    per = _capi.split_models(ctx.fetch_packed()[0], ctx._models)
    parts = residue_pairs.split(t, np.arange(F + 1) * pc.n_residues)
    for f in range(F):
        _same(parts[f], _ref(ens.model_pack(f), per[f]), ('fetched', f))
        _same(parts[f], got[f], ('context', f))
    _same(ctx.models_persistence(), before, 'persistence after the fetches')


def _packed_bytes(ctx):
    bags, _ = ctx.fetch_packed()
    return {name: {k: np.asarray(v).tobytes() for k, v in b.items()} for name, b in bags.items()}


@pytest.mark.gpu
def test_contract():
    pc = _hub()
    L = _capi.load()
    ctx = _capi.Context(0)
    h = ctx._h
    cnt = C.c_int64(-1)
    launch = lambda: L.arp_residue_pairs_launch(h, C.byref(cnt))
    fetch = lambda cap, *cols: L.arp_residue_pairs_fetch(h, cap, *(cols + (None,) * (7 - len(cols))), C.byref(cnt))
    # before any pass; after only the atom-atom launch
    assert launch() == _capi.ARP_E_ARG and fetch(0) == _capi.ARP_E_ARG
    ctx.set_complex(pc)
    assert launch() == _capi.ARP_E_ARG
    ctx.atom_contacts_launch(*PARAMS[0])
    assert launch() == _capi.ARP_E_ARG and fetch(0) == _capi.ARP_E_ARG
    with pytest.raises(ValueError, match='complete pass'):
        ctx.residue_pairs()
    # a pass: the table; a second launch returns the stored count
    ctx.run_launch(*PARAMS[0])
    t = ctx.residue_pairs()
    U = len(t['res_a'])
    assert U > 100
    assert launch() == _capi.ARP_OK and cnt.value == U
    cnt.value = -1
    assert launch() == _capi.ARP_OK and cnt.value == U
    # cap too small: ARP_E_CAPACITY with the count, nothing written; NULL columns
    a = np.full(U, -7, np.int32)
    assert fetch(U - 1, _capi._p(a)) == _capi.ARP_E_CAPACITY and cnt.value == U and np.all(a == -7)
    assert fetch(U, _capi._p(a)) == _capi.ARP_OK and np.array_equal(a, t['res_a'])
    assert fetch(U) == _capi.ARP_OK and cnt.value == U
    pl = np.zeros((U, 4), np.uint32)
    assert fetch(U, None, None, None, None, None, None, _capi._p(pl)) == _capi.ARP_OK and np.array_equal(pl, t['plane_count'])
    # the atom-atom bag refilled alone, or one ring / amide bag: the table went with the results it was made from
    ctx.atom_contacts_launch(*PARAMS[1])
    assert fetch(U) == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    _same(ctx.residue_pairs(), t, 'again')
    ctx.launch_bag('plane_plane')
    assert fetch(U) == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    _same(ctx.residue_pairs(), t, 'after a bag launch and a new pass')
    # a selection change after the pass
    ctx.set_selection(np.ones(pc.n_atoms, np.uint8))
    assert launch() == _capi.ARP_E_ARG and fetch(U) == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    _same(ctx.residue_pairs(), t, 'after the selection was set again')
    # a structure change after the pass
    ctx.set_complex(pc)
    assert launch() == _capi.ARP_E_ARG and fetch(U) == _capi.ARP_E_ARG
    # a shard context
    ctx.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    assert launch() == _capi.ARP_E_ARG
    assert b'shard' in L.arp_last_error(h)
    ctx.close()
    # the bags do not notice the table: both packed layouts, sort-after-pass on and off, the table made before the fetch
    for rows in (False, True):
        for sort_after in (False, True):
            plain = _ctx(pc, sort_after)
            plain.set_packed_layout(rows)
            plain.run_launch(*PARAMS[0])
            ref = _packed_bytes(plain)
            plain.close()
            ctx = _ctx(pc, sort_after)
            ctx.set_packed_layout(rows)
            ctx.run_launch(*PARAMS[0])
            before = _packed_bytes(ctx)
            _same(ctx.residue_pairs(), t, (rows, sort_after))
            after = _packed_bytes(ctx)
            assert before == after == ref, (rows, sort_after)
            ctx.run_launch(*PARAMS[0])
            _same(ctx.residue_pairs(), t, (rows, sort_after, 'table first'))
            assert _packed_bytes(ctx) == ref, (rows, sort_after, 'table first')
            ctx.close()


@pytest.mark.gpu
def test_interaction_complex_residue_contacts(tmp_path):
    from arpeggio_amd.core import InteractionComplex
    pc = copy.copy(_hub())
    ic = InteractionComplex(pc)
    ic.run_arpeggio([], *PARAMS[0])
    t = ic.residue_contacts()
    _same(t, _ref(ic.pc, ic._bags), 'complex')
    path = ic.write_residue_contacts(str(tmp_path))
    assert os.path.basename(path) == ic.id + '.rescontacts'
    with open(path, newline='') as fh:
        assert len(list(csv.reader(fh))) == len(t['res_a']) + 1
