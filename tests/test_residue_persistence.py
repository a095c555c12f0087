"""Residue contact persistence over the models of an ensemble, reduced on the device (arp_models_residue_persistence_launch /
_fetch, Context.models_residue_persistence, EnsembleComplex.run_residue_persistence, arpeggio_amd.residue_persistence).

The yardstick is never the device reduction: it is ``reference_table`` below — a plain loop over the models in ascending order
that folds per-model residue tables made by ``test_residue_pairs.reference_table`` from bags that did not come through the new
code (the oracle's five bags of each model, and the bags ``run_models`` fetches and cuts).  Every comparison is exact: integers
equal, the three float columns compared as bytes.  No tolerance anywhere."""
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
from oracle import ref_py
from arpeggio_amd import _capi, residue_persistence, synth
from helpers import tiny_complex
from test_models import _same
from test_persistence import PARAMS
from test_residue_pairs import PLANE_BAGS, _aa, _cluster, _hub, _ids, _mask, _oracle_everything_selected, _oracle_pass, _ref
from test_residue_pairs import reference_table as pair_table

F_HUB = 8


def reference_table(per_model_tables):
    """The residue persistence table of per-model residue-pair tables (model-local residue ids): key res_a * nres + res_b,
    np.unique, then ONE loop over the models in ascending order.  A model touches a row at most once, so ``acc[idx] += d``
    there IS the one-by-one order of dist_sum."""
    nres = max([int(t['res_b'].max()) + 1 for t in per_model_tables if len(t['res_b'])] + [1])
    keys = [t['res_a'].astype(np.int64) * nres + t['res_b'].astype(np.int64) for t in per_model_tables]
    uk = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    U = len(uk)
    nm = np.zeros(U, np.int64)
    first, last = np.full(U, -1, np.int32), np.full(U, -1, np.int32)
    n = np.zeros(U, np.int64)
    cls = np.zeros((U, 5), np.int64)
    bits = np.zeros((U, 15), np.int64)
    dmin, dmax = np.full(U, np.inf, np.float32), np.full(U, -np.inf, np.float32)
    acc = np.zeros(U, np.float64)
    ct = np.zeros(U, np.uint8)
    for f, t in enumerate(per_model_tables):
        idx = np.searchsorted(uk, keys[f])
        assert len(np.unique(idx)) == len(idx), 'a pair twice in one model'
        nm[idx] += 1
        first[idx] = np.where(first[idx] < 0, f, first[idx])
        last[idx] = f
        n[idx] += t['n_contacts']
        has = t['n_contacts'] > 0
        cls[idx, 0] += has
        cls[idx, 1:] += t['plane_count'] > 0
        bits[idx] += t['bit_count'] > 0
        d = np.asarray(t['dist_min'], np.float32)[has]
        at = idx[has]
        dmin[at] = np.minimum(dmin[at], d)
        dmax[at] = np.maximum(dmax[at], d)
        acc[at] += d.astype(np.float64)
        ct[idx] |= t['ctype_mask']
    assert nm.max(initial=0) <= 65535
    return dict(res_a=(uk // nres).astype(np.int32), res_b=(uk % nres).astype(np.int32), n_models=nm.astype(np.uint16), first=first,
                last=last, n_contacts=n.astype(np.uint32), class_models=cls.astype(np.uint16), bit_models=bits.astype(np.uint16),
                dist_min=dmin, dist_max=dmax, dist_sum=acc, ctype_mask=ct)


def _pairs(t):
    return list(zip(t['res_a'].tolist(), t['res_b'].tolist()))


def _model(res_id, ring_res=(), amide_res=(), **bags):
    return pair_table(bags, res_id, np.asarray(ring_res, np.int32), np.asarray(amide_res, np.int32))


# ---- the structures of the seam tests: models as translated copies of a cluster, 16 A apart along x
def _translated(pc, F, away=None):
    """[F, n, 3] float32: model f = the pack shifted by 16 f A along x; ``away`` = (model, residue): that residue of that model
    moved 50 A along z as one piece."""
    xyz = np.repeat(np.asarray(pc.xyz, np.float32)[None], F, axis=0)
    xyz[:, :, 0] += (16.0 * np.arange(F, dtype=np.float32))[:, None]
    if away is not None:
        f, r = away
        xyz[f, pc.res_id == r, 2] += np.float32(50.0)
    return np.ascontiguousarray(xyz), np.zeros((F, 0, 3))


def _host_model_pack(pc, xyz_f):
    """Model f of a seam structure for the oracle: the topology with the model's coordinates and, from the oracle's own
    geometry functions, the planes of its amides (the seam structures have no rings)."""
    q = copy.copy(pc)
    q.xyz = np.ascontiguousarray(xyz_f)
    assert pc.n_rings == 0
    if pc.n_amides:
        q.amide_center, q.amide_normal = ref_py.amide_geometry(q.xyz, pc.amide_atoms)
    return q


def seam_two_residues(n):
    """``n`` atoms of ``_cluster`` in two interleaved residues: (n / 2)^2 records in one row."""
    return tiny_complex(_cluster(n), res_id=[k & 1 for k in range(n)])


def seam_single_residue():
    return tiny_complex(_cluster(8), res_id=[0] * 8)


SEAMS = (('a', 16, 3, None), ('b', 24, 3, None), ('c', 16, 4, (1, 1)), ('d', 16, 1, None))      # (name, atoms, F, away)


def seam_sentinel_tie():
    """Four residues and — in the test — four models: nres_t - 1 = 3 and F - 1 = 3 are all ones in their two bits.  Residue 3
    carries two planar amides (N, C, O, C-alpha in one z plane) stacked 3.5 A apart: group-group records of the pair (3, 3),
    whose key in model 3 is all ones in the bits of (res_a, res_b, f).  A third amide, its atoms in residue 2 but WITHOUT a
    residue of its own in the topology (amide_res -1), is stacked on the second: its group-group records are left out.
    Residues 0 and 1 are single atoms beside the stack."""
    quad = np.array([(0.0, 0.0, 0.0), (1.3, 0.0, 0.0), (1.9, 1.1, 0.0), (2.0, -1.2, 0.0)])
    xyz = np.concatenate([[(-2.0, 0.0, 0.0), (-2.0, 2.0, 3.5)], quad, quad + (0, 0, 3.5), quad + (0, 0, 7.0)])
    pc = tiny_complex(xyz, res_id=[0, 1] + [3] * 8 + [2] * 4,
                      amides=(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.array([3, 3, -1], np.int32)))
    pc.amide_atoms = np.arange(2, 14, dtype=np.int32).reshape(3, 4)
    return pc


@functools.lru_cache(maxsize=None)
def _hub_models(F=F_HUB):
    pc = _hub()
    pc.ensure_labels()
    return (pc,) + tuple(synth.models_of(pc, F, seed=4, jitter=0.3))


# ------------------------------------------------------------------------------------------------------------- CPU
def test_reference_table_on_hand_made_tables():
    """Three models over atoms in residues [0, 1, 1, 2, 0], one ring of residue 2, one amide of residue 2."""
    H, V, P = 1 << 5, 1 << 3, 1 << 4
    res_id = [0, 1, 1, 2, 0]
    # model 0: (0, 1) twice (3.0, 2.5), (0, 2) once; the ring pair (2, 2)
    m0 = _model(res_id, [2], [2], atom_atom=_aa([0, 0, 3], [1, 2, 4], [3.0, 2.5, 4.0], [H | P, P, V], [2, 1, 0]),
                plane_plane=_ids('bgn', [0], 'end', [0]))
    # model 1: the pair (0, 1) is missing; (1, 2) through an atom-plane record only
    m1 = _model(res_id, [2], [2], atom_plane=_ids('atom', [1], 'ring', [0]))
    # model 2: (0, 1) with plane records ONLY (a ring of residue 1 against two atoms of residue 0), (0, 2) again
    m2 = _model(res_id, [1], [2], atom_atom=_aa([3], [4], [3.5], [V | P], [2]), atom_plane=_ids('atom', [0, 4], 'ring', [0, 0]))
    # model 3: (0, 1) once more, farther
    m3 = _model(res_id, [2], [2], atom_atom=_aa([1], [4], [3.25], [V], [2]))
    t = reference_table([m0, m1, m2, m3])
    assert _pairs(t) == [(0, 1), (0, 2), (1, 2), (2, 2)]
    assert t['n_models'].tolist() == [3, 2, 1, 1]
    assert t['first'].tolist() == [0, 0, 1, 0] and t['last'].tolist() == [3, 2, 1, 0]
    assert t['n_contacts'].tolist() == [3, 2, 0, 0]
    assert t['class_models'].tolist() == [[2, 1, 0, 0, 0], [2, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0]]
    assert t['bit_models'][0].tolist() == [0, 0, 0, 1, 1, 1] + [0] * 9      # vdw in model 3, proximal and hbond in model 0 — once each
    assert t['bit_models'][1].tolist() == [0, 0, 0, 2, 1] + [0] * 10
    assert not t['bit_models'][2:].any()
    # dist_min: the smallest record; dist_max: the largest of the per-model minima (2.5 and 3.25, not 3.0)
    assert t['dist_min'].tolist() == [2.5, 3.5, np.inf, np.inf] and t['dist_max'].tolist() == [3.25, 4.0, -np.inf, -np.inf]
    assert t['dist_sum'].tolist() == [5.75, 7.5, 0.0, 0.0]
    assert t['ctype_mask'].tolist() == [(1 << 2) | (1 << 1), (1 << 0) | (1 << 2), 0, 0]
    assert [t[k].dtype for k, _ in residue_persistence.COLUMNS] == [np.dtype(dt) for _, dt in residue_persistence.COLUMNS]
    assert list(t) == [k for k, _ in residue_persistence.COLUMNS]
    assert t['class_models'].shape == (4, 5) and t['bit_models'].shape == (4, 15)
    # the order of dist_sum: float32 values whose float64 sum depends on the order
    big, small = np.float32(2.0 ** 60), np.float32(1.0)
    one = lambda d: _model([0, 1], atom_atom=_aa([0], [1], [d], [0], [0]))
    t = reference_table([one(big), one(small), one(-big)])
    assert t['dist_sum'][0] == (np.float64(big) + np.float64(small)) - np.float64(big) == 0.0      # (any other order gives 1.0)
    assert t['dist_min'][0] == -big and t['dist_max'][0] == big and t['class_models'][0, 0] == 3
    # no model, and models without a record
    e = _model(res_id)
    _same(reference_table([e, e]), residue_persistence.empty(), 'empty models')
    _same(reference_table([]), residue_persistence.empty(), 'no model')


def _random_models(rs, F, nres, empty=()):
    ident = np.arange(nres)
    out = []
    for f in range(F):
        k = 0 if f in empty else rs.randint(5, 40)
        i, j = rs.randint(0, nres, k), rs.randint(0, nres, k)
        keep = i != j
        bags = dict(atom_atom=_aa(i[keep], j[keep], rs.rand(int(keep.sum())) * 5 + 1, rs.randint(0, 1 << 15, int(keep.sum())),
                                  rs.randint(0, 7, int(keep.sum()))))
        if k:
            bags['plane_plane'] = _ids('bgn', rs.randint(0, nres, 4), 'end', rs.randint(0, nres, 4))
            bags['group_plane'] = _ids('amide', rs.randint(0, nres, 3), 'ring', rs.randint(0, nres, 3))
        out.append(pair_table(bags, ident, ident, ident))
    return out


_MERGED_EXACTLY = ('res_a', 'res_b', 'n_models', 'first', 'last', 'n_contacts', 'class_models', 'bit_models', 'dist_min', 'dist_max', 'ctype_mask')


def test_merge_of_two_chunks_equals_the_whole_at_every_boundary():
    rs = np.random.RandomState(13)
    F, nres = 7, 9
    models = _random_models(rs, F, nres, empty=(3,))
    whole = reference_table(models)
    assert len(whole['res_a']) > 20 and whole['n_models'].max() > 1 and (whole['class_models'][:, 0] == 0).any()
    key = lambda t: t['res_a'].astype(np.int64) * nres + t['res_b']
    for c in range(1, F):
        t1, t2 = reference_table(models[:c]), reference_table(models[c:])
        m = residue_persistence.merge(t1, t2, c)
        assert list(m) == [k for k, _ in residue_persistence.COLUMNS]
        for k in _MERGED_EXACTLY:
            _same({k: m[k]}, {k: whole[k]}, (c, k))
        # dist_sum: t1's sum + t2's sum, in that order, to the bit (a pair of one chunk alone: the other's sum is 0.0)
        s1, s2 = np.zeros(len(m['res_a'])), np.zeros(len(m['res_a']))
        s1[np.searchsorted(key(m), key(t1))] = t1['dist_sum']
        s2[np.searchsorted(key(m), key(t2))] = t2['dist_sum']
        _same({'dist_sum': m['dist_sum']}, {'dist_sum': s1 + s2}, c)
    # three chunks, left to right
    m = residue_persistence.merge(residue_persistence.merge(reference_table(models[:2]), reference_table(models[2:5]), 2),
                                  reference_table(models[5:]), 5)
    for k in _MERGED_EXACTLY:
        _same({k: m[k]}, {k: whole[k]}, ('three', k))
    assert np.allclose(m['dist_sum'], whole['dist_sum'], rtol=1e-12, atol=0)      # (rounding of the chunk sums only)
    # an empty table on either side
    for m in (residue_persistence.merge(residue_persistence.empty(), whole, 0), residue_persistence.merge(whole, residue_persistence.empty(), F)):
        _same(m, whole, 'empty side')
    # counts that leave their type
    hi = dict(whole, n_models=np.full(len(whole['res_a']), 40000, np.uint16))
    with pytest.raises(OverflowError):
        residue_persistence.merge(hi, hi, 40000)
    hc = dict(whole, n_contacts=np.full(len(whole['res_a']), 1 << 31, np.uint32))
    with pytest.raises(OverflowError):
        residue_persistence.merge(hc, hc, 1)
    with pytest.raises(ValueError):
        residue_persistence.merge(whole, whole, -1)


def test_frequency_records_and_csv_on_a_small_table(tmp_path):
    from arpeggio_amd.core import export
    pc = _hub()
    pc.ensure_labels()
    H, P = 1 << 5, 1 << 4
    a0, a1 = (int(np.nonzero(pc.res_id == r)[0][0]) for r in (0, 3))
    ring_res, none = np.array([5], np.int32), np.zeros(0, np.int32)
    m0 = pair_table(dict(atom_atom=_aa([a0, a0], [a1, a1 + 1], [3.5, 3.0], [H | P, P], [2, 1]), plane_plane=_ids('bgn', [0], 'end', [0])),
                    pc.res_id, ring_res, none)
    m1 = pair_table(dict(atom_atom=_aa([a0], [a1], [4.0], [P], [2])), pc.res_id, ring_res, none)
    t = reference_table([m0, pair_table({}, pc.res_id, ring_res, none), m1, m0])
    assert _pairs(t) == [(0, 3), (5, 5)]
    fr = residue_persistence.frequency(t, 4)
    assert fr['contact'].tolist() == [0.75, 0.5] and fr['contact'].dtype == np.float64
    assert fr['classes'].shape == (2, 5) and fr['classes'][0, 0] == 0.75 and fr['classes'][1].tolist() == [0, 0, 0.5, 0, 0]
    assert fr['bits'].shape == (2, 15) and fr['bits'][0, 4] == 0.75 and fr['bits'][0, 5] == 0.5
    with pytest.raises(ValueError):
        residue_persistence.frequency(t, 0)
    lab = export.Labels(pc, pc.component_types)
    rec = residue_persistence.to_records(t, pc)
    assert len(rec) == 2
    want = lab.atom_dict(a0)
    del want['auth_atom_id']
    assert rec[0]['bgn'] == want and rec[0]['end']['auth_seq_id'] == int(pc.res_seq[3]) and rec[1]['bgn'] == rec[1]['end']
    assert rec[0]['n_models'] == 3 and rec[0]['first_model'] == 0 and rec[0]['last_model'] == 3 and rec[0]['n_contacts'] == 5
    assert rec[0]['distance_min'] == 3.0 and rec[0]['distance_max'] == 4.0 and rec[0]['distance_sum'] == 10.0
    assert rec[0]['distance_mean'] == 10.0 / 3
    assert rec[0]['contact'] == {'proximal': 3, 'hbond': 2} and rec[0]['classes'] == {'atom_atom': 3}
    assert rec[0]['interacting_entities'] == ['INTRA_SELECTION', 'INTER']
    assert rec[1]['n_models'] == 2 and rec[1]['classes'] == {'plane_plane': 2} and rec[1]['contact'] == {} and rec[1]['n_contacts'] == 0
    assert rec[1]['distance_min'] is None and rec[1]['distance_max'] is None and rec[1]['distance_mean'] is None
    assert json.loads(json.dumps(rec)) == rec
    path = tmp_path / 'small.csv'
    residue_persistence.write_csv(str(path), t, pc)
    with open(path, newline='') as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == residue_persistence.CSV_HEADER and len(rows[0]) == 9 + 5 + 15 + 1 and len(rows) == 3
    assert rows[1][:9] == [lab.res_macro[0], lab.res_macro[3], '3', '0', '3', '5', '3.0', '4.0', '10.0'] and rows[1][-1] == 'INTRA_SELECTION|INTER'
    assert [int(x) for x in rows[1][9:14]] == [3, 0, 0, 0, 0] and [int(x) for x in rows[1][14:29]] == t['bit_models'][0].tolist()
    assert rows[2][:9] == [lab.res_macro[5], lab.res_macro[5], '2', '0', '3', '0', '', '', ''] and rows[2][-1] == ''
    assert [int(x) for x in rows[2][9:14]] == [0, 0, 2, 0, 0]
    assert os.path.basename(residue_persistence.write_residue_persistence(str(tmp_path), 'x1', t, pc)) == 'x1.respersist'
    assert (tmp_path / 'x1.respersist').read_bytes() == path.read_bytes()


def test_constants_and_columns_match_the_header():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert int(re.search(r'#define\s+ARP_RESPERSIST_BITS\s+(\d+)', hdr).group(1)) == _capi.RESPERSIST_BITS == residue_persistence.N_BITS == 15
    assert _capi.RESPERSIST_COLUMNS == residue_persistence.COLUMNS and len(residue_persistence.COLUMNS) == 12
    assert residue_persistence.CLASSES == ('atom_atom',) + tuple(b[0] for b in PLANE_BAGS)
    assert 'arp_models_residue_persistence_launch' in _capi.SYMBOLS and 'arp_models_residue_persistence_fetch' in _capi.SYMBOLS
    # the fetch takes the columns in the order of COLUMNS
    args = re.search(r'int arp_models_residue_persistence_fetch\(([^;]*)\);', hdr).group(1)
    names = re.findall(r'(\w+)\s*(?:/\*[^*]*\*/)?\s*(?:,|$)', args)
    assert names == ['ctx', 'cap'] + [k for k, _ in residue_persistence.COLUMNS] + ['count']
    _same(residue_persistence.empty(), {k: np.zeros((0, {'class_models': 5, 'bit_models': 15}[k]) if k in ('class_models', 'bit_models') else 0, dt)
                                        for k, dt in residue_persistence.COLUMNS}, 'empty')


def _seam_oracle_tables(pc, xyz):
    return [_ref(q, _oracle_pass(q)) for q in (_host_model_pack(pc, xyz[f]) for f in range(len(xyz)))]


def test_the_seam_structures_are_what_they_claim():
    """By the oracle, on the CPU: the figures the GPU seam cases lean on."""
    for name, n, F, away in SEAMS:
        pc = seam_two_residues(n)
        xyz, _ = _translated(pc, F, away)
        per = _seam_oracle_tables(pc, xyz)
        counts = [int(t['n_contacts'].sum()) for t in per]
        t = reference_table(per)
        if name in ('a', 'd'):
            assert counts == [64] * F      # every model boundary of the one row falls on a multiple of 64
        if name == 'b':
            assert counts == [144] * F and 144 % 64 != 0 and 144 > 128      # 432 records: boundaries at 144 and 288, mid-step
        if name == 'c':
            assert counts == [64, 0, 64, 64]
            assert t['n_models'].tolist() == [3] and t['first'].tolist() == [0] and t['last'].tolist() == [3]
        assert _pairs(t) == [(0, 1)] and t['n_contacts'].tolist() == [sum(counts)], name
    s = seam_single_residue()
    xyz, _ = _translated(s, 3)
    _same(reference_table(_seam_oracle_tables(s, xyz)), residue_persistence.empty(), 'single residue')
    # the sentinel tie: in every model group-group records of (3, 3) and left-out ones of the amide without a residue
    d = seam_sentinel_tie()
    assert d.n_residues == 4
    xyz, _ = _translated(d, 4)
    per = []
    for f in range(4):
        q = _host_model_pack(d, xyz[f])
        bags = _oracle_everything_selected(q)
        gg = bags['group_group']
        res = np.stack([q.amide_res[gg['bgn']], q.amide_res[gg['end']]], axis=1)
        assert int((res.min(axis=1) < 0).sum()) == 2 and int(((res == 3).all(axis=1)).sum()) == 2, f      # both orders of each amide pair
        per.append(_ref(q, bags))
    t = reference_table(per)
    row = (t['res_a'] == 3) & (t['res_b'] == 3)
    assert row.sum() == 1 and t['n_models'][row][0] == 4 and t['class_models'][row][0].tolist() == [0, 0, 0, 4, 0]
    assert t['class_models'][:, 3].sum() == 4 and len(t['res_a']) > 1 and t['n_contacts'].sum() > 0


def test_the_parity_structure_has_partial_rows_and_plane_rows():
    """proteinlike40, F = 8, 5.0 A, whole structure, by the oracle: rows that are not in every model, rows whose models do not
    all have an atom-atom record, intra-residue rows and records in the ring / amide classes.  The planes of each model come
    from the oracle's geometry functions here; the GPU cases take them from the device (``EnsembleComplex.model_pack``)."""
    pc, xyz, h_xyz = _hub_models()
    per = []
    for f in range(F_HUB):
        q = copy.copy(pc)
        q.xyz, q.h_xyz = np.ascontiguousarray(xyz[f]), np.ascontiguousarray(h_xyz[f])
        q.ring_center, q.ring_normal = ref_py.ring_geometry(q.xyz, pc.ring_atoms)
        q.ring_res = ref_py.ring_residues(q.xyz, pc.res_id, q.ring_center)[0]
        q.amide_center, q.amide_normal = ref_py.amide_geometry(q.xyz, pc.amide_atoms)
        per.append(_ref(q, _oracle_pass(q)))
    t = reference_table(per)
    assert (t['n_models'] < F_HUB).any() and (t['class_models'][:, 0] < t['n_models']).any()
    assert (t['res_a'] == t['res_b']).any() and t['class_models'][:, 1:].any()
    print('rows', len(t['res_a']), 'partial', int((t['n_models'] < F_HUB).sum()), 'intra-residue', int((t['res_a'] == t['res_b']).sum()),
          'models per class', t['class_models'].sum(axis=0).tolist())


# ------------------------------------------------------------------------------------------------------------- GPU
def _ctx_with_models(pc, xyz, h_xyz, sort_after=True):
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(sort_after)
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    return ctx


@functools.lru_cache(maxsize=None)
def _hub_ensemble():
    """The hub's eight models resident in an EnsembleComplex, and the packs of the models (planes as the device made them)."""
    from arpeggio_amd.core import EnsembleComplex
    pc, xyz, h_xyz = _hub_models()
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    return ens, tuple(ens.model_pack(f) for f in range(F_HUB))


def _hub_selections(pc):
    """Whole structure, one residue, a residue range: (name, mask of one model or None)."""
    r = pc.n_residues // 3
    rng = np.zeros(pc.n_atoms, np.uint8)
    rng[(pc.res_id >= r) & (pc.res_id < r + 12)] = 1
    return (('whole', None), ('one residue', _mask(pc, ['/%s/%d/' % (pc.res_chain[r], int(pc.res_seq[r]))])), ('range', rng))


@pytest.mark.gpu
@pytest.mark.parametrize('params', PARAMS, ids=[str(p[0]) for p in PARAMS])
def test_table_equals_both_folds(params):
    ens, packs = _hub_ensemble()
    pc, ctx = ens.pc, ens._ctx
    for name, sel in _hub_selections(pc):
        what = (params, name)
        got = ens.run_residue_persistence([] if sel is None else np.nonzero(sel)[0], *params)
        assert ens.residue_persistence is got and ens.residue_persistence_models == F_HUB and ens._results is None
        want = reference_table([_ref(q, _oracle_pass(q, params, sel)) for q in packs])
        print(what, 'rows', len(want['res_a']), 'records', int(want['n_contacts'].sum()), 'models per class', want['class_models'].sum(axis=0).tolist())
        _same(got, want, what + ('oracle',))
        per = _capi.split_models(ctx.fetch_packed()[0], ctx._models)
        _same(got, reference_table([_ref(q, b) for q, b in zip(packs, per)]), what + ('fetched',))
        _same(ctx.models_residue_persistence(), got, what + ('after the fetch',))
        assert len(got['res_a']) > 0
        if sel is None:
            assert (got['n_models'] < F_HUB).any() and (got['class_models'][:, 0] < got['n_models']).any()


@pytest.mark.gpu
def test_segment_seams():
    for name, n, F, away in SEAMS:
        pc = seam_two_residues(n)
        xyz, h_xyz = _translated(pc, F, away)
        ctx = _ctx_with_models(pc, xyz, h_xyz)
        per = ctx.run_models(*PARAMS[0])
        got = ctx.models_residue_persistence()
        packs = [_host_model_pack(pc, xyz[f]) for f in range(F)]
        _same(got, reference_table([_ref(q, b) for q, b in zip(packs, per)]), (name, 'fetched'))
        _same(got, reference_table([_ref(q, _oracle_pass(q)) for q in packs]), (name, 'oracle'))
        assert _pairs(got) == [(0, 1)], name
        if name == 'b':
            assert got['n_contacts'].tolist() == [432] and got['n_models'].tolist() == [3]
        if name == 'c':
            assert got['n_models'].tolist() == [3] and got['first'].tolist() == [0] and got['last'].tolist() == [3]
            assert got['class_models'][0].tolist() == [3, 0, 0, 0, 0]
        if name == 'd':
            assert got['n_models'].tolist() == [1] and got['dist_min'].tobytes() == got['dist_max'].tobytes()
            assert got['dist_sum'][0] == np.float64(got['dist_min'][0])
        ctx.close()
    # (e) a single residue: no record, no row
    pc = seam_single_residue()
    xyz, h_xyz = _translated(pc, 3)
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    counts = ctx.run_launch(*PARAMS[0])
    assert counts['atom_atom'] == 0
    got = ctx.models_residue_persistence()
    _same(got, residue_persistence.empty(), 'single residue')
    cnt = C.c_int64(-1)
    assert ctx._L.arp_models_residue_persistence_launch(ctx._h, C.byref(cnt)) == _capi.ARP_OK and cnt.value == 0
    assert ctx._L.arp_models_residue_persistence_fetch(ctx._h, 0, *([None] * 12), C.byref(cnt)) == _capi.ARP_OK and cnt.value == 0
    ctx.close()


@pytest.mark.gpu
def test_a_fetch_of_one_column_returns_the_bytes_of_the_full_fetch():
    """Seam structure a (16 atoms, two residues, F = 3), each of the three device-reduced tables, every column: a fetch with
    only that column non-NULL gives the bytes the full fetch gives for it.  The slab of a table is laid out in the order of its
    fetch's arguments; a column copied from another column's place would show here."""
    _, n, F, away = SEAMS[0]
    pc = seam_two_residues(n)
    xyz, h_xyz = _translated(pc, F, away)
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    ctx.run_launch(*PARAMS[0])
    for table, fetch, columns in ((ctx.models_persistence, 'arp_models_persistence_fetch', _capi.PERSIST_COLUMNS),
                                  (ctx.residue_pairs, 'arp_residue_pairs_fetch', _capi.RESPAIR_COLUMNS),
                                  (ctx.models_residue_persistence, 'arp_models_residue_persistence_fetch', _capi.RESPERSIST_COLUMNS)):
        full = table()
        U = len(full[columns[0][0]])
        assert U > 0 and list(full) == [k for k, _ in columns], fetch
        for q, (k, dt) in enumerate(columns):
            one = np.empty(full[k].shape, dt)
            one.view(np.uint8)[...] = 0xA5
            args = [None] * len(columns)
            args[q] = _capi._p(one)
            cnt = C.c_int64(-1)
            assert getattr(ctx._L, fetch)(ctx._h, U, *args, C.byref(cnt)) == _capi.ARP_OK and cnt.value == U, (fetch, k)
            assert one.tobytes() == full[k].tobytes(), (fetch, k)
    ctx.close()


@pytest.mark.gpu
def test_left_out_records_do_not_split_the_row_they_tie_with():
    """seam_sentinel_tie in four models with an installed selection state and the five bags launched one by one (all five
    valid: a complete pass): the group-group records of the amide without a residue are left out, and (3, 3) is ONE row with
    all four models."""
    pc = seam_sentinel_tie()
    F = 4
    xyz, h_xyz = _translated(pc, F)
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    ones = lambda k: np.ones(F * k, np.uint8)
    ctx.set_selection_state(ones(pc.n_atoms), ones(pc.n_atoms), ones(pc.n_rings), ones(pc.n_rings), ones(pc.n_amides), ones(pc.n_amides))
    ctx.atom_contacts_launch(*PARAMS[0])
    with pytest.raises(ValueError, match='complete pass'):
        ctx.models_residue_persistence()
    bags = {name: (ctx.launch_bag(name), ctx.fetch_bag(name))[1] for name, *_ in PLANE_BAGS}
    bags['atom_atom'] = ctx.atom_contacts_fetch(F * pc.n_atoms * pc.n_atoms)
    got = ctx.models_residue_persistence()
    am_res = np.concatenate([np.where(pc.amide_res >= 0, pc.amide_res + f * pc.n_residues, -1) for f in range(F)])
    gg = bags['group_group']
    assert int(((am_res[gg['bgn']] < 0) | (am_res[gg['end']] < 0)).sum()) == 2 * F
    packs = [_host_model_pack(pc, xyz[f]) for f in range(F)]
    per = _capi.split_models(bags, ctx._models)
    _same(got, reference_table([_ref(q, b) for q, b in zip(packs, per)]), 'fetched')
    _same(got, reference_table([_ref(q, _oracle_everything_selected(q)) for q in packs]), 'oracle')
    row = (got['res_a'] == 3) & (got['res_b'] == 3)
    assert row.sum() == 1 and got['n_models'][row][0] == 4 and got['class_models'][row][0].tolist() == [0, 0, 0, 4, 0]
    assert (got['first'][row][0], got['last'][row][0]) == (0, 3)
    ctx.close()


@pytest.mark.gpu
def test_planes():
    """The hub's own rings and amides: intra-residue rows and models counted in the ring / amide classes."""
    ens, packs = _hub_ensemble()
    got = ens.run_residue_persistence([], *PARAMS[0])
    _same(got, reference_table([_ref(q, _oracle_pass(q, PARAMS[0], None)) for q in packs]), 'oracle')
    assert (got['res_a'] == got['res_b']).any() and got['class_models'][:, 1:].any()
    plane_only = got['class_models'][:, 0] == 0
    assert plane_only.any() and np.all(np.isposinf(got['dist_min'][plane_only])) and np.all(np.isneginf(got['dist_max'][plane_only]))
    assert np.all(got['dist_sum'][plane_only] == 0.0) and np.all(got['n_contacts'][plane_only] == 0)


@pytest.mark.gpu
def test_streaming_chunks_accumulate_to_the_merge_of_the_chunk_tables():
    from arpeggio_amd.core import EnsembleComplex
    pc = _hub()
    xyz, h_xyz = synth.models_of(pc, 5, seed=9, jitter=0.3)
    ens = EnsembleComplex((copy.copy(pc), xyz[:2], h_xyz[:2]))
    refs = []
    for lo, hi in ((0, 2), (2, 5)):
        if lo:
            ens.set_coordinates(xyz[lo:hi], h_xyz[lo:hi])
        ens.run_arpeggio([], *PARAMS[0])
        refs.append(reference_table([_ref(ens.model_pack(k), ens.model(k)._bags) for k in range(hi - lo)]))
        ens.run_residue_persistence([], *PARAMS[0], accumulate=True)
        assert ens.residue_persistence_models == hi
    want = residue_persistence.merge(refs[0], refs[1], 2)
    _same(ens.residue_persistence, want, 'streamed')
    one = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    whole = one.run_residue_persistence([], *PARAMS[0])
    for k in _MERGED_EXACTLY:
        _same({k: ens.residue_persistence[k]}, {k: whole[k]}, ('one pass', k))
    # dist_sum is first + second: where a chunk does not have the pair its sum is 0.0
    key = lambda t: t['res_a'].astype(np.int64) * pc.n_residues + t['res_b']
    s1, s2 = np.zeros(len(whole['res_a'])), np.zeros(len(whole['res_a']))
    s1[np.searchsorted(key(whole), key(refs[0]))] = refs[0]['dist_sum']
    s2[np.searchsorted(key(whole), key(refs[1]))] = refs[1]['dist_sum']
    _same({'dist_sum': ens.residue_persistence['dist_sum']}, {'dist_sum': s1 + s2}, 'first + second')
    # accumulate=False starts over
    ens.run_residue_persistence([], *PARAMS[0])
    assert ens.residue_persistence_models == 3
    _same(ens.residue_persistence, refs[1], 'restart')


def _packed_bytes(ctx):
    bags, _ = ctx.fetch_packed()
    out = {name: {k: np.asarray(v).tobytes() for k, v in b.items()} for name, b in bags.items()}
    aa = ctx.atom_contacts_fetch(len(np.asarray(bags['atom_atom']['j'])), sort=True)
    out['fetch'] = {k: np.asarray(v).tobytes() for k, v in aa.items()}
    return out


def _table_bytes(t):
    return {k: np.asarray(v).tobytes() for k, v in t.items()}


@pytest.mark.gpu
def test_contract():
    pc, xyz, h_xyz = _hub_models()
    F = 3
    xyz, h_xyz = xyz[:F], h_xyz[:F]
    L = _capi.load()
    ctx = _capi.Context(0)
    h = ctx._h
    cnt = C.c_int64(-1)
    launch = lambda: L.arp_models_residue_persistence_launch(h, C.byref(cnt))
    fetch = lambda cap, *cols: L.arp_models_residue_persistence_fetch(h, cap, *(cols + (None,) * (12 - len(cols))), C.byref(cnt))
    # before anything; a structure that is no set of models, with a complete pass
    assert launch() == _capi.ARP_E_ARG and fetch(0) == _capi.ARP_E_ARG
    ctx.set_complex(pc)
    ctx.run_launch(*PARAMS[0])
    assert launch() == _capi.ARP_E_ARG and b'no models resident' in L.arp_last_error(h)
    with pytest.raises(ValueError, match='no models resident'):
        ctx.models_residue_persistence()
    # models resident: no pass yet; the atom-atom launch alone is no complete pass
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    assert launch() == _capi.ARP_E_ARG and b'complete pass' in L.arp_last_error(h) and fetch(0) == _capi.ARP_E_ARG
    ctx.atom_contacts_launch(*PARAMS[0])
    assert launch() == _capi.ARP_E_ARG and fetch(0) == _capi.ARP_E_ARG
    with pytest.raises(ValueError, match='complete pass'):
        ctx.models_residue_persistence()
    # a pass: the table; a second launch returns the stored count
    ctx.run_launch(*PARAMS[0])
    t = ctx.models_residue_persistence()
    U = len(t['res_a'])
    assert U > 100
    assert launch() == _capi.ARP_OK and cnt.value == U
    cnt.value = -1
    assert launch() == _capi.ARP_OK and cnt.value == U
    # cap too small: ARP_E_CAPACITY with the count, nothing written; NULL columns
    a = np.full(U, -7, np.int32)
    s = np.full(U, -7.0, np.float64)
    assert fetch(U - 1, _capi._p(a), *([None] * 9), _capi._p(s)) == _capi.ARP_E_CAPACITY and cnt.value == U and np.all(a == -7) and np.all(s == -7.0)
    assert fetch(U, _capi._p(a)) == _capi.ARP_OK and np.array_equal(a, t['res_a'])
    assert fetch(U) == _capi.ARP_OK and cnt.value == U
    cm, bm = np.zeros((U, 5), np.uint16), np.zeros((U, 15), np.uint16)
    assert fetch(U, None, None, None, None, None, None, _capi._p(cm), _capi._p(bm), None, None, _capi._p(s)) == _capi.ARP_OK
    assert np.array_equal(cm, t['class_models']) and np.array_equal(bm, t['bit_models']) and s.tobytes() == t['dist_sum'].tobytes()
    # the other two tables in any order: none voids another, each stays what it was
    p0, r0 = ctx.models_persistence(), ctx.residue_pairs()
    _same(ctx.models_residue_persistence(), t, 'after both tables')
    ctx.run_launch(*PARAMS[0])
    r1 = ctx.residue_pairs()
    t1 = ctx.models_residue_persistence()
    p1 = ctx.models_persistence()
    _same(t1, t, 'between the tables')
    _same(ctx.models_residue_persistence(), t, 'after the tables')
    _same(p1, p0, 'persistence')
    _same(r1, r0, 'residue pairs')
    _same(ctx.models_persistence(), p0, 'persistence again')
    _same(ctx.residue_pairs(), r0, 'residue pairs again')
    # the atom-atom bag refilled alone, or one ring / amide bag: the table went with the results it was made from
    ctx.atom_contacts_launch(*PARAMS[1])
    assert fetch(U) == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    _same(ctx.models_residue_persistence(), t, 'again')
    ctx.launch_bag('plane_plane')
    assert fetch(U) == _capi.ARP_E_ARG
    # a new pass
    ctx.run_launch(*PARAMS[1])
    assert fetch(U) == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    _same(ctx.models_residue_persistence(), t, 'after a bag launch and new passes')
    # a selection change after the pass
    ctx.set_selection(np.ones(F * pc.n_atoms, np.uint8))
    assert launch() == _capi.ARP_E_ARG and fetch(U) == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    _same(ctx.models_residue_persistence(), t, 'after the selection was set again')
    # a model change after the pass
    ctx.set_models(xyz, h_xyz)
    assert launch() == _capi.ARP_E_ARG and fetch(U) == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    _same(ctx.models_residue_persistence(), t, 'after the models were set again')
    # a structure change after the pass: no models any more
    ctx.set_complex(pc)
    assert launch() == _capi.ARP_E_ARG and fetch(U) == _capi.ARP_E_ARG
    # a shard context
    ctx.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    assert launch() == _capi.ARP_E_ARG
    assert b'shard' in L.arp_last_error(h)
    ctx.close()


@pytest.mark.gpu
def test_more_models_than_the_uint16_columns_count_are_refused():
    """65 536 models of a two-atom topology: refused before anything is looked at but the number of models."""
    pc = tiny_complex(_cluster(2), res_id=[0, 1])
    F = 65536
    xyz = np.ascontiguousarray(np.repeat(np.asarray(pc.xyz, np.float32)[None], F, axis=0))
    ctx = _capi.Context(0)
    ctx.set_topology(pc)
    ctx.set_models(xyz, np.zeros((F, 0, 3)))
    cnt = C.c_int64(-1)
    assert ctx._L.arp_models_residue_persistence_launch(ctx._h, C.byref(cnt)) == _capi.ARP_E_ARG
    assert b'65 535' in ctx._L.arp_last_error(ctx._h)
    ctx.close()


@pytest.mark.gpu
def test_bags_and_the_other_tables_do_not_notice_the_table():
    """Both packed layouts, sort-after-pass on and off: the packed bags, the sorted atom-atom fetch, the persistence table and
    the residue-pair table are byte-identical with, without, before and after the call."""
    pc, xyz, h_xyz = _hub_models()
    F = 3
    xyz, h_xyz = xyz[:F], h_xyz[:F]
    want = None
    for rows in (False, True):
        for sort_after in (False, True):
            what = (rows, sort_after)
            plain = _ctx_with_models(pc, xyz, h_xyz, sort_after)      # never calls the reduction
            plain.set_packed_layout(rows)
            plain.run_launch(*PARAMS[0])
            ref = _packed_bytes(plain)
            ref_p, ref_r = _table_bytes(plain.models_persistence()), _table_bytes(plain.residue_pairs())
            plain.close()
            ctx = _ctx_with_models(pc, xyz, h_xyz, sort_after)
            ctx.set_packed_layout(rows)
            ctx.run_launch(*PARAMS[0])
            before = _packed_bytes(ctx)
            t = ctx.models_residue_persistence()
            want = t if want is None else want
            _same(t, want, what)
            assert _packed_bytes(ctx) == before == ref, what
            assert _table_bytes(ctx.models_persistence()) == ref_p and _table_bytes(ctx.residue_pairs()) == ref_r, what
            _same(ctx.models_residue_persistence(), want, what + ('after the others',))
            # the table first, straight after a pass
            ctx.run_launch(*PARAMS[0])
            _same(ctx.models_residue_persistence(), want, what + ('table first',))
            assert _packed_bytes(ctx) == ref, what + ('table first',)
            assert _table_bytes(ctx.residue_pairs()) == ref_r and _table_bytes(ctx.models_persistence()) == ref_p, what + ('table first',)
            ctx.close()
