"""Interaction networks: the connected components of the contact graph (arpeggio_amd/networks.py, csrc/arp_networks.h,
Context.networks, InteractionComplex.networks / write_networks, EnsembleComplex.run_networks).

The yardstick is ``yardstick`` below: a plain-Python union-find with a dict, over bags that never went through the new code
(``fetch_packed`` / ``run_models`` bags and the oracle's).  It is itself held against hand-written answers.  Both
``networks.components`` and the device result are compared with it, never only with each other.  Everything is an integer, a
minimum, a count or an OR, so every comparison is exact."""
import copy
import csv
import ctypes as C
import functools
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, contact_filter, networks, synth, tables
from arpeggio_amd.core import config
from helpers import tiny_complex
from test_persistence import _ctx_with_models, _mask
from test_residue_pairs import _oracle_pass

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
ALL, CALL = contact_filter.SIFT_ALL, contact_filter.CTYPE_ALL
COLS = [k for k, _ in tables.NETWORKS.columns]
PASS = (5.0, 0.1, True)
OK, E_ARG, E_CAP = _capi.ARP_OK, _capi.ARP_E_ARG, _capi.ARP_E_CAPACITY


# ------------------------------------------------------------------------------------------------------- the yardstick
def yardstick(bag, n_nodes, sift_any=ALL, ctype_mask=CALL, res_id=None):
    """(label, rows): label a list of n_nodes ints, rows a list of (root, n_nodes, n_edges, sift_or, ctype_or) ascending by
    root.  One record at a time, a dict for the parents."""
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            x = parent[x]
        return x

    edges = []
    for i, j, s, c in zip(np.asarray(bag['i']).tolist(), np.asarray(bag['j']).tolist(), np.asarray(bag['sift']).tolist(),
                          np.asarray(bag['ctype']).tolist()):
        if not (s & sift_any) or not (ctype_mask >> c) & 1:
            continue
        a, b = (i, j) if res_id is None else (int(res_id[i]), int(res_id[j]))
        if a < 0 or b < 0:
            continue
        assert a < n_nodes and b < n_nodes
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
        edges.append((a, s, c))
    label = [find(v) if v in parent else -1 for v in range(n_nodes)]
    rows = {r: [r, 0, 0, 0, 0] for r in sorted(set(label) - {-1})}
    for v in range(n_nodes):
        if label[v] >= 0:
            rows[label[v]][1] += 1
    for a, s, c in edges:
        row = rows[label[a]]
        row[2] += 1
        row[3] |= s
        row[4] |= 1 << c
    return label, [tuple(r) for r in rows.values()]


def _rows(table):
    assert list(table) == COLS and [table[k].dtype for k in COLS] == [np.dtype(dt) for _, dt in tables.NETWORKS.columns]
    return list(zip(*(table[k].tolist() for k in COLS)))


def _same(got, want, what):
    """A (label, table) result against the yardstick's (label, rows)."""
    label, table = got
    assert label.dtype == np.int32 and label.tolist() == want[0], what
    assert _rows(table) == want[1], what


def _bag(i, j, sift, ctype):
    return {'i': np.asarray(i, np.int32), 'j': np.asarray(j, np.int32), 'sift': np.asarray(sift, np.uint16),
            'ctype': np.asarray(ctype, np.uint8)}


# ------------------------------------------------------------------------------------------------------------- CPU
H, V, P, I = BIT['hbond'], BIT['vdw'], BIT['proximal'], BIT['ionic']
# 9 nodes.  {0, 4, 2} by (4, 0) and (2, 4); {5, 7} by a double record; 3 has only a record with itself; 1, 6, 8 have none
HAND = _bag([4, 2, 5, 7, 3], [0, 4, 7, 5, 3], [H, V | P, I, H, P], [2, 0, 1, 1, 5])


def _both(bag, n, *args, **kw):
    """The yardstick's answer, after ``networks.components`` has been held against it."""
    want = yardstick(bag, n, *args, **kw)
    _same(networks.components(bag, n, *args, **kw), want, (args, kw))
    return want


def test_yardstick_and_components_on_hand_made_bags():
    label, rows = _both(HAND, 9)
    assert label == [0, -1, 0, 3, 0, 5, -1, 5, -1]
    # two components and isolated nodes; a multi-edge counts twice; the equal-node record is an edge of 3 and joins nothing
    assert rows == [(0, 3, 2, H | V | P, 1 << 2 | 1 << 0), (3, 1, 1, P, 1 << 5), (5, 2, 2, I | H, 1 << 1)]
    # a sift mask that removes (2, 4): the component splits, 2 leaves; sift_or stays the whole sift of what takes part
    label, rows = _both(HAND, 9, H | I)
    assert label == [0, -1, -1, -1, 0, 5, -1, 5, -1]
    assert rows == [(0, 2, 1, H, 1 << 2), (5, 2, 2, I | H, 1 << 1)]
    label, rows = _both(HAND, 9, P)
    assert label == [-1, -1, 2, 3, 2, -1, -1, -1, -1] and rows == [(2, 2, 1, V | P, 1), (3, 1, 1, P, 1 << 5)]
    # a ctype mask that removes (4, 0) and the double record
    label, rows = _both(HAND, 9, ALL, 1 << 0 | 1 << 5)
    assert label == [-1, -1, 2, 3, 2, -1, -1, -1, -1]
    # a record that merges two components, and the same record masked away
    merged = _bag([4, 2, 5, 7, 3, 2], [0, 4, 7, 5, 3, 7], [H, V | P, I, H, P, V], [2, 0, 1, 1, 5, 6])
    label, rows = _both(merged, 9)
    assert label == [0, -1, 0, 3, 0, 0, -1, 0, -1] and rows[0] == (0, 5, 5, H | V | P | I, 1 << 2 | 1 << 0 | 1 << 1 | 1 << 6)
    assert _both(merged, 9, ALL, CALL & ~(1 << 6)) == _both(HAND, 9)
    # no record at all, and masks that none meets
    assert _both(_bag([], [], [], []), 4) == ([-1] * 4, [])
    assert _both(HAND, 9, BIT['xbond']) == ([-1] * 9, [])
    assert _both(HAND, 0, BIT['xbond']) == ([], [])


def test_residue_level_on_a_hand_made_bag():
    res = np.array([0, 0, 1, 2, -1, 3, 3, 4], np.int32)
    # (0, 2): residues 0-1; (1, 3): 0-2; (5, 6): both residue 3, an edge of 3 that joins nothing; (4, 7): atom 4 has no residue
    bag = _bag([0, 1, 5, 4], [2, 3, 6, 7], [H, P, V, I], [2, 2, 0, 1])
    label, rows = _both(bag, 5, res_id=res)
    assert label == [0, 0, 0, 3, -1]
    assert rows == [(0, 3, 2, H | P, 1 << 2), (3, 1, 1, V, 1)]
    with pytest.raises(ValueError, match='beyond n_nodes'):
        networks.components(bag, 3, res_id=res)


def test_masks_are_checked():
    for sa, cm, what in ((0, CALL, 'mask of 0'), (ALL, 0, 'mask of 0'), (1 << 15, CALL, 'beyond'), (ALL, 1 << 7, 'beyond')):
        with pytest.raises(ValueError, match=what):
            networks.components(HAND, 9, sa, cm)


def test_members_of_atoms_largest_and_splits():
    label, table = networks.components(HAND, 9)
    assert networks.members(label, 0).tolist() == [0, 2, 4] and networks.members(label, 5).tolist() == [5, 7]
    assert networks.members(label, 1).tolist() == [] and networks.members(label, 2).tolist() == []
    assert networks.of_atoms(label, [7, 1, 2, 4]).tolist() == [0, 5] and networks.of_atoms(label, [1, 6]).tolist() == []
    assert networks.largest(table) == 0 and networks.largest(networks.empty()) == -1
    tie = {'n_nodes': np.array([2, 5, 5], np.int32)}
    assert networks.largest(tie) == 1
    # two structures of 5 and 4 nodes: 0-4 | 5-8.  HAND has no record across 4 | 5
    parts = networks.split_structures(label, table, [0, 5, 9])
    assert [p[0].tolist() for p in parts] == [[0, -1, 0, 3, 0], [0, -1, 0, -1]]
    assert _rows(parts[0][1]) == [(0, 3, 2, H | V | P, 5), (3, 1, 1, P, 32)] and _rows(parts[1][1]) == [(0, 2, 2, I | H, 2)]
    assert all(p[0].dtype == np.int32 for p in parts)
    with pytest.raises(ValueError, match='reaches into another'):
        networks.split_structures(label, table, [0, 3, 9])
    with pytest.raises(ValueError, match='node count last'):
        networks.split_structures(label, table, [0, 5, 8])
    # three models of 3 nodes
    three = _bag([0, 3, 7], [1, 5, 8], [H, V, P], [0, 0, 0])
    label3, table3 = networks.components(three, 9)
    per = networks.split_models(label3, table3, 3)
    assert [p[0].tolist() for p in per] == [[0, 0, -1], [0, -1, 0], [-1, 1, 1]]
    assert [_rows(p[1]) for p in per] == [[(0, 2, 1, H, 1)], [(0, 2, 1, V, 1)], [(1, 2, 1, P, 1)]]
    with pytest.raises(ValueError, match='divide'):
        networks.split_models(label3, table3, 4)


def _labelled():
    pc = synth.proteinlike(n_res=12, seed=3, n_waters=4)
    pc.ensure_labels()
    return pc


def test_csv_text_and_records(tmp_path):
    from arpeggio_amd.core import export
    pc = _labelled()
    lab = export.Labels(pc, pc.component_types)
    n = pc.n_atoms
    bag = _bag([0, 1, n - 2], [1, 5, n - 1], [H, V | P, I], [2, 2, 3])
    label, table = networks.components(bag, n)
    path = networks.write_networks(str(tmp_path), 'x1', label, table, pc)
    assert path == os.path.join(str(tmp_path), 'x1.networks')
    with open(path, newline='') as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == networks.CSV_HEADER == ['root', 'n_nodes', 'n_edges', 'contacts', 'interacting_entities', 'members']
    assert rows[1] == [lab.atom_macro(0), '3', '2', 'vdw|proximal|hbond', 'INTER', '|'.join(lab.atom_macro(v) for v in (0, 1, 5))]
    assert rows[2] == [lab.atom_macro(n - 2), '2', '1', 'ionic', 'SELECTION_WATER', lab.atom_macro(n - 2) + '|' + lab.atom_macro(n - 1)]
    assert len(rows) == 3
    rec = networks.to_records(label, table, pc)
    assert rec[0]['root'] == lab.atom_dict(0) and rec[0]['members'] == [lab.atom_dict(v) for v in (0, 1, 5)]
    assert (rec[0]['n_nodes'], rec[0]['n_edges'], rec[0]['contact'], rec[0]['interacting_entities']) == (3, 2, ['vdw', 'proximal', 'hbond'], ['INTER'])
    # residue level: residue labels
    rl, rt = networks.components(bag, pc.n_residues, res_id=pc.res_id)
    networks.write_csv(path, rl, rt, pc, 'residue')
    with open(path, newline='') as fh:
        rows = list(csv.reader(fh))
    want = yardstick(bag, pc.n_residues, res_id=pc.res_id)
    assert [r[0] for r in rows[1:]] == [lab.res_macro[r[0]] for r in want[1]]
    assert [r[5].split('|') for r in rows[1:]] == [[lab.res_macro[v] for v in range(pc.n_residues) if want[0][v] == r[0]] for r in want[1]]
    assert networks.to_records(rl, rt, pc, 'residue')[0]['root'].keys() == {'label_comp_id', 'auth_seq_id', 'auth_asym_id', 'pdbx_PDB_ins_code', 'label_comp_type'}
    with pytest.raises(ValueError, match='level'):
        networks.write_csv(path, label, table, pc, 'chain')


# ------------------------------------------------------------------------------------------------------------- GPU
def _ctx(pc, params=PASS, sel=None):
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(False)
    ctx.set_complex(pc)
    if sel is not None:
        ctx.set_selection(sel)
    ctx.run_launch(*params)
    return ctx


def _aa(ctx):
    """The atom-atom bag of fetch_packed() in the records layout, copied out of its buffer."""
    ctx.set_packed_layout(False)
    bags, _ = ctx.fetch_packed()
    return {k: np.array(v) for k, v in bags['atom_atom'].items()}


def _check(ctx, bag, n_nodes, sift_any=ALL, ctype_mask=CALL, res_id=None, what=None):
    """The device result and ``networks.components`` on ``bag``, each against the yardstick on ``bag``; returns the yardstick's."""
    want = yardstick(bag, n_nodes, sift_any, ctype_mask, res_id)
    _same(ctx.networks(sift_any, ctype_mask, res_id is not None), want, ('device', what, hex(sift_any), hex(ctype_mask)))
    _same(networks.components(bag, n_nodes, sift_any, ctype_mask, res_id), want, ('host', what, hex(sift_any), hex(ctype_mask)))
    st = ctx.stats()
    assert st['networks_rows'] == len(want[1]) and st['networks_nodes'] == n_nodes
    return want


N_CHAIN = 4099


@functools.lru_cache(maxsize=None)
def _scrambled_chain(per_residue=1, n=N_CHAIN, seed=11):
    """``n`` atoms on a line 3 A apart; atom a sits at position pos[a], a seeded random permutation; hydrophobes on the
    positions with (p // 10) % 2 == 0; ``per_residue`` spatially consecutive atoms a residue."""
    pos = np.random.default_rng(seed).permutation(n)
    xyz = np.stack([3.0 * pos, np.zeros(n), np.zeros(n)], axis=1)
    tm = np.where((pos // 10) % 2 == 0, config.ATOM_TYPE_BIT['hydrophobe'], 0)
    return tiny_complex(xyz, type_mask=tm, res_id=pos // per_residue), pos


@pytest.mark.gpu
def test_scrambled_chain():
    """4098 records (more than 16 blocks of 256, no multiple of 64) over ids that are a random permutation of the positions:
    long parent paths, unions racing across blocks, and wave aggregation with one root and with many roots in a wave."""
    pc, pos = _scrambled_chain()
    n = N_CHAIN
    ctx = _ctx(pc)
    bag, obag = _aa(ctx), _oracle_pass(pc, PASS)['atom_atom']
    assert len(bag['i']) == len(obag['i']) == n - 1
    for b, what in ((bag, 'fetched'), (obag, 'oracle')):
        label, rows = _check(ctx, b, n, what=what)
        assert label == [0] * n and [r[:3] for r in rows] == [(0, n, n - 1)]
        label, rows = _check(ctx, b, n, BIT['hydrophobic'], what=what)
        assert int((np.asarray(b['sift']) & BIT['hydrophobic'] != 0).sum()) == 1845
        assert len(rows) == 205 and {r[1:3] for r in rows} == {(10, 9)} and label.count(-1) == 2049
        # a block of ten hydrophobes is ten consecutive positions; its root is the smallest id on them
        inv = np.argsort(pos)
        assert [r[0] for r in rows] == sorted(int(inv[p0:p0 + 10].min()) for p0 in range(0, n - 9, 20))
    ctx.close()


@functools.lru_cache(maxsize=None)
def _lattice(cut):
    nx, ny = 64, 65
    n = nx * ny
    pos = np.random.default_rng(5).permutation(n)
    x, y = pos % nx, pos // nx
    z = np.where((x == 30) & cut, 50.0, 0.0)
    return tiny_complex(np.stack([3.0 * x, 3.0 * y, z], axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize('cut', (False, True), ids=('whole', 'cut'))
def test_lattice(cut):
    """64 x 65 atoms 3 A apart in a plane, ids scrambled: edges at 3.0 and 4.24 A, so cycles everywhere — most unions are
    redundant and the CAS on the few roots is contended.  ``cut``: the column x = 30 lifted 50 A, which leaves three pieces."""
    pc = _lattice(cut)
    n = pc.n_atoms
    ctx = _ctx(pc)
    bag, obag = _aa(ctx), _oracle_pass(pc, PASS)['atom_atom']
    assert len(bag['i']) == len(obag['i']) > 3 * n
    for b, what in ((bag, 'fetched'), (obag, 'oracle')):
        label, rows = _check(ctx, b, n, what=what)
        assert sorted(r[1] for r in rows) == (sorted([30 * 65, 65, 33 * 65]) if cut else [n])
        assert rows[0][0] == 0 and sum(r[2] for r in rows) == len(b['i'])
        _check(ctx, b, n, BIT['proximal'], what=what)      # the diagonals alone: still cycles, two interleaved sub-lattices
    ctx.close()


def _line(positions):
    p = np.asarray(positions, np.float64)
    return tiny_complex(np.stack([p, np.zeros(len(p)), np.zeros(len(p))], axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize('n', (64, 65, 256, 257, 512))
def test_seams(n):
    """Chains in id order whose node counts end inside, at the end of and one past a wave and a tile of the root count."""
    # ---- the last two atoms 50 A behind the rest: the component {n - 2, n - 1}, whose root is the last node that can be one
    p = 3.0 * np.arange(n)
    p[n - 2:] += 50.0
    ctx = _ctx(_line(p))
    label, rows = _check(ctx, _aa(ctx), n, what='tail')
    assert [r[:3] for r in rows] == [(0, n - 2, n - 3), (n - 2, 2, 1)] and label[-2:] == [n - 2, n - 2]
    # masks that no record meets: 0 rows, all -1
    assert _check(ctx, _aa(ctx), n, BIT['metal_complex'], what='no record meets') == ([-1] * n, [])
    ctx.close()
    # ---- pairs 50 A apart: a root on every even id, n // 2 rows (every lane pair of every wave of the rank); an odd n leaves
    # the last atom alone
    ctx = _ctx(_line(53.0 * (np.arange(n) // 2) + 3.0 * (np.arange(n) % 2)))
    label, rows = _check(ctx, _aa(ctx), n, what='pairs')
    assert [r[:3] for r in rows] == [(2 * q, 2, 1) for q in range(n // 2)] and label[-1] == (-1 if n % 2 else n - 2)
    ctx.close()


@pytest.mark.gpu
def test_an_empty_bag():
    ctx = _ctx(_line([0.0, 50.0, 100.0]))
    bag = _aa(ctx)
    assert len(bag['i']) == 0
    assert _check(ctx, bag, 3) == ([-1] * 3, [])
    assert _check(ctx, bag, 3, res_id=np.arange(3)) == ([-1] * 3, [])
    ctx.close()


@pytest.mark.gpu
def test_residue_level():
    """The scrambled chain with three spatially consecutive atoms a residue: a chain of residues."""
    pc, pos = _scrambled_chain(3)
    nres = pc.n_residues
    assert nres == (N_CHAIN + 2) // 3
    ctx = _ctx(pc)
    bag, obag = _aa(ctx), _oracle_pass(pc, PASS)['atom_atom']
    for b, what in ((bag, 'fetched'), (obag, 'oracle')):
        inter = int((pc.res_id[b['i']] != pc.res_id[b['j']]).sum())
        label, rows = _check(ctx, b, nres, res_id=pc.res_id, what=what)
        assert label == [0] * nres and [r[:3] for r in rows] == [(0, nres, inter)] and inter == nres - 1
        _check(ctx, b, nres, BIT['hydrophobic'], res_id=pc.res_id, what=what)
        _check(ctx, b, N_CHAIN, what=what)      # the atom level of the same pass: other arguments remake the result
    ctx.close()


@pytest.mark.gpu
def test_a_batch_never_joins_its_structures():
    a, b = _scrambled_chain(1, 300, 1)[0], _scrambled_chain(2, 131, 2)[0]
    ctx = _capi.Context(0)
    off = ctx.set_batch([a, b])
    ctx.run_launch(*PASS)
    bag = _aa(ctx)
    for lvl, key, res in (('atom', 'atom', None), ('residue', 'residue', np.concatenate([a.res_id, b.res_id + a.n_residues]))):
        n = int(off[key][-1])
        label, rows = _check(ctx, bag, n, res_id=res, what=lvl)
        # a is one chain at both levels; b (two atoms a residue, no record inside a residue) is one chain of residues, and at
        # atom level the 65 pairs across its residue boundaries
        first_b = int(off[key][1])
        assert rows[0][:2] == (0, first_b) and all(r[0] >= first_b for r in rows[1:]) and len(rows) == 1 + (65 if res is None else 1)
        for hyd in (ALL, BIT['hydrophobic']):
            got = ctx.networks(hyd, CALL, res is not None)
            parts = networks.split_structures(*got, off[key])
            for s, pc in enumerate((a, b)):
                one = _ctx(pc)
                nn = pc.n_atoms if res is None else pc.n_residues
                want = _check(one, _aa(one), nn, hyd, res_id=None if res is None else pc.res_id, what=(lvl, s))
                _same(parts[s], want, (lvl, s, hex(hyd)))
                one.close()
    ctx.close()


def _three_models():
    """A chain of 150 atoms in three models; model 1 is cut in the middle."""
    pc, pos = _scrambled_chain(3, 150, 4)
    xyz = np.repeat(np.asarray(pc.xyz, np.float32)[None], 3, axis=0)
    xyz[1, pos >= 75, 1] += np.float32(50.0)
    return copy.copy(pc), xyz, np.zeros((3, 0, 3))


@pytest.mark.gpu
def test_models_and_run_networks():
    from arpeggio_amd.core import EnsembleComplex
    pc, xyz, h_xyz = _three_models()
    n, F = pc.n_atoms, 3
    ctx = _ctx_with_models(pc, xyz, h_xyz, sort_after=False)
    per = ctx.run_models(*PASS)
    bag = _aa(ctx)
    _check(ctx, bag, F * n, what='models')
    # residue r holds the positions 3 r ... 3 r + 2: a chain of 50 residues, cut in model 1 between the residues 24 and 25
    nres = pc.n_residues
    label, rows = _check(ctx, bag, F * nres, res_id=np.concatenate([pc.res_id + f * nres for f in range(F)]), what='models, residues')
    assert [r[:2] for r in rows] == [(0, nres), (nres, 25), (nres + 25, 25), (2 * nres, nres)]
    parts = networks.split_models(*ctx.networks(), n)
    for f in range(F):
        _same(parts[f], yardstick(per[f]['atom_atom'], n), f)
    ctx.close()
    pc.ensure_labels()
    ens = EnsembleComplex((pc, xyz, h_xyz))
    for level, nn, res in (('atom', n, None), ('residue', pc.n_residues, pc.res_id)):
        for contacts in (None, ['hydrophobic']):
            lab, t = ens.run_networks([], *PASS, contacts=contacts, level=level)
            assert lab.shape == (F, nn) and lab.dtype == np.int32 and list(t) == COLS + ['model'] and t['model'].dtype == np.int32
            sa = ALL if contacts is None else BIT['hydrophobic']
            want_rows = []
            for f in range(F):
                wl, wr = yardstick(per[f]['atom_atom'], nn, sa, res_id=res)
                assert lab[f].tolist() == wl, (level, contacts, f)
                want_rows += [r + (f,) for r in wr]
            assert list(zip(*(t[k].tolist() for k in COLS + ['model']))) == want_rows, (level, contacts)
    assert ens.stats['networks_launches'] == 4
    with pytest.raises(ValueError, match='level'):
        ens.run_networks([], *PASS, level='chain')


@functools.lru_cache(maxsize=None)
def _protein():
    pc = synth.proteinlike()
    pc.ensure_labels()
    return pc


@pytest.mark.gpu
def test_a_protein_through_context_and_interaction_complex(tmp_path):
    from arpeggio_amd.core import InteractionComplex, export
    pc = _protein()
    n, params = pc.n_atoms, (5.0, 0.1, False)
    hp = BIT['hbond'] | BIT['polar']
    # whole structure
    ctx = _ctx(pc, params)
    bag, obag = _aa(ctx), _oracle_pass(pc, params)['atom_atom']
    for b, what in ((bag, 'fetched'), (obag, 'oracle')):
        label, rows = _check(ctx, b, n, hp, what=what)
        assert len(rows) > 3 and max(r[1] for r in rows) > 2
        _check(ctx, b, n, what=what)
        _check(ctx, b, pc.n_residues, hp, res_id=pc.res_id, what=what)
    ctx.close()
    # a ligand selection and INTER
    sel = _mask(pc, ['/A/508/'])
    ctx = _ctx(pc, params, sel)
    bag, obag = _aa(ctx), _oracle_pass(pc, params, sel)['atom_atom']
    for b, what in ((bag, 'fetched, ligand'), (obag, 'oracle, ligand')):
        label, rows = _check(ctx, b, n, ALL, 1 << CT['INTER'], what=what)
        assert len(rows) >= 1
        assert networks.of_atoms(np.asarray(label), np.nonzero(sel)[0]).tolist() == [r[0] for r in rows]      # every INTER record has a ligand atom
    ctx.close()
    ic = InteractionComplex(copy.copy(pc))
    with pytest.raises(AttributeError):
        ic.networks()
    ic.run_arpeggio(['/A/508/'], *params)
    aa = {k: np.asarray(ic._bags['atom_atom'][k]) for k in ('i', 'j', 'sift', 'ctype')}
    _same(ic.networks(contacts=['hbond', 'polar']), yardstick(aa, n, hp), 'ic, hbond | polar')
    want = yardstick(aa, n, ALL, 1 << CT['INTER'])
    _same(ic.networks(interacting_entities=['INTER']), want, 'ic, INTER')
    _same(ic.networks(level='residue'), yardstick(aa, pc.n_residues, res_id=pc.res_id), 'ic, residue')
    with pytest.raises(ValueError, match='nothing_like_it'):
        ic.networks(contacts=['nothing_like_it'])
    with pytest.raises(ValueError, match='level'):
        ic.networks(level='chain')
    path = ic.write_networks(str(tmp_path), interacting_entities=['INTER'])
    assert path == os.path.join(str(tmp_path), ic.id + '.networks')
    lab = export.Labels(pc, pc.component_types)
    with open(path, newline='') as fh:
        got = list(csv.reader(fh))
    assert got[0] == networks.CSV_HEADER and len(got) == 1 + len(want[1])
    for line, r in zip(got[1:], want[1]):
        assert line[:3] == [lab.atom_macro(r[0]), str(r[1]), str(r[2])] and line[4] == 'INTER'
        assert line[5].split('|') == [lab.atom_macro(v) for v in range(n) if want[0][v] == r[0]]
    # a contact filter changes the fetched records, not the resident bag the networks are made from
    ic.set_contact_filter(contacts=['ionic'])
    ic.run_arpeggio(['/A/508/'], *params)
    assert len(ic._bags['atom_atom']['i']) < len(aa['i'])
    _same(ic.networks(interacting_entities=['INTER']), want, 'ic, with a contact filter')


# ---- residency, voiding, refusals
def _table_fetch(ctx, name, spec, U):
    t = tables.alloc(spec, U, np.zeros)
    n = C.c_int64(-1)
    rc = getattr(ctx._L, name)(ctx._h, U, *(_capi._p(t[k]) for k, _ in spec.columns), C.byref(n))
    return rc, b''.join(t[k].tobytes() for k, _ in spec.columns)


def _everything(ctx):
    """The five bags as bytes."""
    ctx.set_packed_layout(False)
    bags, _ = ctx.fetch_packed()
    return {(name, k): np.asarray(v).tobytes() for name, b in bags.items() if isinstance(b, dict) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _hub_models():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    pc.ensure_labels()
    return (pc,) + tuple(synth.models_of(pc, 3, seed=4))


@pytest.mark.gpu
def test_residency_and_voiding():
    """The resident result is returned without work and remade on other arguments; a new pass, a selection and a pass, and a
    models upload void it; the packed layout, a plane bag alone and the making of every other derived result do not; the bags
    and the other tables are byte-identical around a launch."""
    from arpeggio_amd import similarity
    pc, xyz, h_xyz = _hub_models()
    F, n = 3, pc.n_atoms
    hp = BIT['hbond'] | BIT['polar']
    specific = contact_filter.SPECIFIC[0]
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    ctx.run_launch(5.0)
    bags = _everything(ctx)
    bag = _aa(ctx)
    want, want_hp = yardstick(bag, F * n), yardstick(bag, F * n, hp)
    assert want != want_hp and len(want_hp[1]) > 3

    def others():
        made = dict(persist=ctx.models_persistence(), respair=ctx.residue_pairs(), respersist=ctx.models_residue_persistence(),
                    bridges=ctx.water_bridges(specific), bridgepersist=ctx.models_water_bridge_persistence(specific),
                    lifetimes=ctx.models_lifetimes(1))
        out = {(name, k): v.tobytes() for name, t in made.items() for k, v in t.items()}
        out['filtered'] = ctx.contacts_filter(specific, 0x7F)
        out['similarity'] = ctx.models_similarity(similarity.planes(None, ('atom_atom',))).tobytes()
        return out

    def fetch(rows):
        lab = np.full(F * n, 7, np.int32)
        nn = C.c_int64(-1)
        rc = ctx._L.arp_networks_labels_fetch(ctx._h, F * n, _capi._p(lab), C.byref(nn))
        return rc, _table_fetch(ctx, 'arp_networks_fetch', tables.NETWORKS, rows)[0]

    before = others()
    n0 = ctx.stats()['networks_launches']
    _same(ctx.networks(), want, 'first')
    st = ctx.stats()
    assert st['networks_launches'] == n0 + 1 and st['networks_rows'] == len(want[1]) and st['networks_nodes'] == F * n
    _same(ctx.networks(), want, 'resident')
    assert ctx.stats() == st                                           # returned without work
    assert _everything(ctx) == bags and others() == before             # nothing else changed, and the making of every other result ...
    _same(ctx.networks(), want, 'after the others')
    assert ctx.stats()['networks_launches'] == n0 + 1                  # ... did not void it
    _same(ctx.networks(hp), want_hp, 'other masks')                    # remade on other arguments
    assert ctx.stats()['networks_launches'] == n0 + 2
    _same(ctx.networks(hp, CALL, True), yardstick(bag, F * pc.n_residues, hp, res_id=np.concatenate([pc.res_id + f * pc.n_residues for f in range(F)])), 'residue')
    assert ctx.stats()['networks_launches'] == n0 + 3 and ctx.stats()['networks_nodes'] == F * pc.n_residues
    _same(ctx.networks(hp), want_hp, 'atom level again')
    assert _everything(ctx) == bags and others() == before
    rows = len(want_hp[1])
    # not voided by the packed layout or by a plane bag alone
    ctx.set_packed_layout(True)
    ctx.launch_bag('plane_plane')
    assert fetch(rows) == (OK, OK)
    ctx.set_packed_layout(False)
    n1 = ctx.stats()['networks_launches']
    _same(ctx.networks(hp), want_hp, 'still resident')
    assert ctx.stats()['networks_launches'] == n1
    # voided by a new pass
    ctx.run_launch(5.0)
    assert fetch(rows) == (E_ARG, E_ARG)
    _same(ctx.networks(hp), want_hp, 'after a new pass')
    assert ctx.stats()['networks_launches'] == n1 + 1
    # ... by a selection (refused until the pass that follows) and a pass
    ctx.set_selection(np.ones(ctx.n, np.uint8))
    assert fetch(rows) == (E_ARG, E_ARG)
    with pytest.raises(ValueError, match='no atom-contact results'):
        ctx.networks(hp)
    ctx.run_launch(5.0)
    assert fetch(rows) == (E_ARG, E_ARG)
    _same(ctx.networks(hp), want_hp, 'after a selection and a pass')
    # ... by a models upload
    ctx.set_models(xyz, h_xyz)
    assert fetch(rows) == (E_ARG, E_ARG)
    with pytest.raises(ValueError, match='no atom-contact results'):
        ctx.networks(hp)
    ctx.run_launch(5.0)
    _same(ctx.networks(hp), want_hp, 'after a models upload and a pass')
    ctx.close()


@pytest.mark.gpu
def test_refusals():
    pc = _protein()
    n = pc.n_atoms
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    L, h = ctx._L, ctx._h
    cnt = C.c_int64(-1)
    launch = lambda sa=ALL, cm=CALL, fl=0: L.arp_networks_launch(h, sa, cm, fl, C.byref(cnt))
    lab = np.full(n, 7, np.int32)
    labels = lambda cap: L.arp_networks_labels_fetch(h, cap, _capi._p(lab), C.byref(cnt))
    # no pass
    assert launch() == E_ARG and b'no atom-contact results' in L.arp_last_error(h)
    assert labels(n) == E_ARG and _table_fetch(ctx, 'arp_networks_fetch', tables.NETWORKS, 4)[0] == E_ARG
    with pytest.raises(ValueError, match='no atom-contact results'):
        ctx.networks()
    ctx.run_launch(5.0, 0.1, False)
    assert labels(n) == E_ARG      # a pass, no launch yet
    # masks and flags, in the house order: beyond the bits, then 0, then the flag
    for sa, cm, fl, what in ((0, CALL, 0, 'mask of 0'), (ALL, 0, 0, 'mask of 0'), (1 << 15, CALL, 0, 'beyond'), (ALL, 1 << 7, 0, 'beyond'),
                             (0, 1 << 7, 0, 'beyond'), (ALL, CALL, 2, 'unknown flag'), (0, CALL, 2, 'mask of 0')):
        assert launch(sa, cm, fl) == E_ARG and what in L.arp_last_error(h).decode(), (sa, cm, fl)
    for sa, cm in ((0, CALL), (1 << 15, CALL), (ALL, 1 << 7)):
        with pytest.raises(ValueError):
            ctx.networks(sa, cm)
    assert L.arp_networks_launch(h, ALL, CALL, 0, None) == E_ARG and L.arp_networks_launch(None, ALL, CALL, 0, C.byref(cnt)) == E_ARG
    # small fetch buffers: ARP_E_CAPACITY with the count, nothing written
    label, table = ctx.networks()
    rows = len(table['root'])
    assert rows >= 1
    assert labels(n - 1) == E_CAP and cnt.value == n and (lab == 7).all()
    assert labels(n) == OK and cnt.value == n and np.array_equal(lab, label)
    t = tables.alloc(tables.NETWORKS, rows, np.zeros)
    args = lambda cap: (h, cap, *(_capi._p(t[k]) for k in COLS), C.byref(cnt))
    assert L.arp_networks_fetch(*args(rows - 1)) == E_CAP and cnt.value == rows and not t['n_nodes'].any()
    assert L.arp_networks_fetch(*args(rows)) == OK and all(np.array_equal(t[k], table[k]) for k in COLS)
    # any column pointer may be NULL
    cnt.value = -1
    assert L.arp_networks_fetch(h, rows, None, None, None, None, None, C.byref(cnt)) == OK and cnt.value == rows
    # a refused launch leaves the resident result
    assert launch(0) == E_ARG and labels(n) == OK
    info = np.zeros(3, np.int64)
    assert L.arp_networks_info(h, _capi._p(info)) == OK and info.tolist() == [rows, n, 1]
    assert L.arp_networks_info(h, None) == E_ARG
    # a shard
    ctx.set_ownership(np.ones(n, np.uint8), np.arange(n, dtype=np.int32))
    assert launch() == E_ARG and b'shard' in L.arp_last_error(h)
    ctx.close()
