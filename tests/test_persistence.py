"""Contact persistence over the models of an ensemble, reduced on the device (arp_models_persistence_launch / _fetch,
Context.models_persistence, EnsembleComplex.run_persistence, arpeggio_amd.persistence).

The yardstick is never the device reduction: it is ``reference_table`` below — a plain NumPy reduction of per-model bags
that did not come through the new code (the oracle's, or the bags ``run_models`` fetches and cuts).  Every comparison is
exact: integers equal, floats compared as bytes.  No tolerance anywhere."""
import copy
import os
import re

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, persistence, synth
from test_models import CASES, _same, _selectors

PARAMS = ((5.0, 0.1, False), (4.0, 0.25, True), (7.5, 0.1, False))


def reference_table(per_model_bags, n):
    """The persistence table of per-model atom-atom bags (model-local ids, i < j, a pair at most once per model): key
    a * n + b, np.unique, one loop over the models in ascending order — ``acc[idx] += dist`` there IS the one-by-one order
    of dist_sum, because a model touches a row at most once."""
    keys = [b['i'].astype(np.int64) * n + b['j'].astype(np.int64) for b in per_model_bags]
    uk = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    U = len(uk)
    nm = np.zeros(U, np.int64)
    first, last = np.full(U, -1, np.int32), np.full(U, -1, np.int32)
    dmin, dmax = np.full(U, np.inf, np.float32), np.full(U, -np.inf, np.float32)
    acc = np.zeros(U, np.float64)
    bits = np.zeros((U, 15), np.int64)
    ct = np.zeros(U, np.uint8)
    for f, b in enumerate(per_model_bags):
        assert np.all(b['i'] < b['j'])
        idx = np.searchsorted(uk, keys[f])
        assert len(np.unique(idx)) == len(idx), 'a pair twice in one model'
        nm[idx] += 1
        first[idx] = np.where(first[idx] < 0, f, first[idx])
        last[idx] = f
        d = np.asarray(b['dist'], np.float32)
        dmin[idx] = np.minimum(dmin[idx], d)
        dmax[idx] = np.maximum(dmax[idx], d)
        acc[idx] += d.astype(np.float64)
        bits[idx] += (b['sift'].astype(np.int64)[:, None] >> np.arange(15)) & 1
        ct[idx] |= (1 << b['ctype'].astype(np.int64)).astype(np.uint8)
    assert nm.max(initial=0) <= 65535
    return dict(a=(uk // n).astype(np.int32), b=(uk % n).astype(np.int32), n_models=nm.astype(np.uint16), first=first, last=last,
                dist_min=dmin, dist_max=dmax, dist_sum=acc, bit_count=bits.astype(np.uint16), ctype_mask=ct)


def _bag(i, j, dist, sift, ctype):
    return dict(i=np.array(i, np.int32), j=np.array(j, np.int32), dist=np.array(dist, np.float32), sift=np.array(sift, np.uint16),
                ctype=np.array(ctype, np.uint8))


def _random_bags(rs, F, n, kmax, empty=()):
    """Per-model bags with distinct pairs, i < j, in canonical order."""
    iu, ju = np.triu_indices(n, 1)
    bags = []
    for f in range(F):
        k = 0 if f in empty else rs.randint(1, kmax)
        pick = np.sort(rs.choice(len(iu), k, replace=False))
        bags.append(_bag(iu[pick], ju[pick], rs.rand(k) * 5 + 1, rs.randint(0, 1 << 15, k), rs.randint(0, 7, k)))
    return bags


def _model_pack(pc, xyz_k, h_k):
    q = copy.copy(pc)
    q.xyz, q.h_xyz = np.ascontiguousarray(xyz_k), np.ascontiguousarray(h_k)
    return q


def _oracle_bags(pc, xyz, h_xyz, params=(5.0, 0.1, False), sel=None):
    out = []
    for k in range(len(xyz)):
        oc = oracle.OracleComplex(_model_pack(pc, xyz[k], h_xyz[k]))
        oc.make_selection(sel)
        out.append(oc.atom_contacts(*params))
    return out


def _hub():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    return pc


# ------------------------------------------------------------------------------------------------------------- CPU
def test_reference_table_on_hand_made_bags():
    """Three models over 6 atoms: (0, 1) in all three with differing SIFt, (0, 2) in the first only, (1, 4) in the last only,
    (2, 3) in the first and the last; the middle model has one record — and a fourth case where it has none."""
    H, V, P = 1 << 5, 1 << 3, 1 << 4
    m0 = _bag([0, 0, 2], [1, 2, 3], [3.0, 4.5, 2.0], [H | P, V, P], [2, 1, 0])
    m1 = _bag([0], [1], [3.5], [P], [2])
    m2 = _bag([0, 1, 2], [1, 4, 3], [2.5, 4.0, 2.25], [H, V | P, P], [1, 2, 0])
    t = reference_table([m0, m1, m2], 6)
    assert t['a'].tolist() == [0, 0, 1, 2] and t['b'].tolist() == [1, 2, 4, 3]
    assert t['n_models'].tolist() == [3, 1, 1, 2]
    assert t['first'].tolist() == [0, 0, 2, 0] and t['last'].tolist() == [2, 0, 2, 2]
    assert t['dist_min'].tolist() == [2.5, 4.5, 4.0, 2.0] and t['dist_max'].tolist() == [3.5, 4.5, 4.0, 2.25]
    assert t['dist_sum'].tolist() == [9.0, 4.5, 4.0, 4.25]
    assert t['bit_count'][0].tolist() == [0, 0, 0, 0, 2, 2] + [0] * 9      # proximal twice, hbond twice
    assert t['bit_count'][1].tolist() == [0, 0, 0, 1] + [0] * 11
    assert t['bit_count'][3].tolist() == [0, 0, 0, 0, 2] + [0] * 10
    assert t['ctype_mask'].tolist() == [(1 << 2) | (1 << 1), 1 << 1, 1 << 2, 1 << 0]
    assert t['dist_sum'].dtype == np.float64 and t['n_models'].dtype == np.uint16 and t['bit_count'].shape == (4, 15)
    # a model with no records in the middle
    e = _bag([], [], [], [], [])
    t = reference_table([m0, e, m2], 6)
    assert t['n_models'].tolist() == [2, 1, 1, 2] and t['first'].tolist() == [0, 0, 2, 0] and t['last'].tolist() == [2, 0, 2, 2]
    # the order of dist_sum: float32 values whose float64 sum depends on the order
    big, small = np.float32(2.0 ** 60), np.float32(1.0)
    t = reference_table([_bag([0], [1], [big], [0], [0]), _bag([0], [1], [small], [0], [0]), _bag([0], [1], [-big], [0], [0])], 3)
    assert t['dist_sum'][0] == (np.float64(big) + np.float64(small)) - np.float64(big) == 0.0      # (any other order gives 1.0)
    assert len(reference_table([e, e], 6)['a']) == 0


def test_merge_of_two_chunks_equals_the_whole_at_every_boundary():
    rs = np.random.RandomState(11)
    F, n = 7, 30
    bags = _random_bags(rs, F, n, 60, empty=(3,))
    whole = reference_table(bags, n)
    assert len(whole['a']) > 50 and whole['n_models'].max() > 1
    for c in range(1, F):
        t1, t2 = reference_table(bags[:c], n), reference_table(bags[c:], n)
        m = persistence.merge(t1, t2, c)
        assert list(m) == [k for k, _ in persistence.COLUMNS]
        for k in ('a', 'b', 'n_models', 'first', 'last', 'dist_min', 'dist_max', 'bit_count', 'ctype_mask'):
            _same({k: m[k]}, {k: whole[k]}, (c, k))
        # dist_sum: t1's sum + t2's sum, in that order, to the bit (a pair of one chunk alone: the other's sum is 0.0)
        key = lambda t: t['a'].astype(np.int64) * n + t['b']
        s1, s2 = np.zeros(len(m['a'])), np.zeros(len(m['a']))
        s1[np.searchsorted(key(m), key(t1))] = t1['dist_sum']
        s2[np.searchsorted(key(m), key(t2))] = t2['dist_sum']
        _same({'dist_sum': m['dist_sum']}, {'dist_sum': s1 + s2}, c)
    # three chunks, left to right
    m = persistence.merge(persistence.merge(reference_table(bags[:2], n), reference_table(bags[2:5], n), 2), reference_table(bags[5:], n), 5)
    for k in ('a', 'b', 'n_models', 'first', 'last', 'dist_min', 'dist_max', 'bit_count', 'ctype_mask'):
        _same({k: m[k]}, {k: whole[k]}, ('three', k))
    # an empty table on either side
    for m in (persistence.merge(persistence.empty(), whole, 0), persistence.merge(whole, persistence.empty(), F)):
        _same(m, whole, 'empty side')
    # uint16 overflow
    t = reference_table(bags[:1], n)
    hi = dict(t, n_models=np.full(len(t['a']), 40000, np.uint16))
    with pytest.raises(OverflowError):
        persistence.merge(hi, hi, 40000)
    hb = dict(t, bit_count=np.full((len(t['a']), 15), 40000, np.uint16))
    with pytest.raises(OverflowError):
        persistence.merge(hb, hb, 1)


def test_frequency_and_records_on_a_small_case():
    pc = _hub()
    pc.ensure_labels()
    m0 = _bag([0, 2], [1, 5], [3.0, 4.0], [(1 << 5) | (1 << 4), 1 << 11], [2, 0])
    m1 = _bag([0], [1], [3.5], [1 << 4], [1])
    t = reference_table([m0, m1, _bag([], [], [], [], []), m1], pc.n_atoms)
    fr = persistence.frequency(t, 4)
    assert fr['contact'].tolist() == [0.75, 0.25] and fr['contact'].dtype == np.float64
    assert fr['bits'].shape == (2, 15) and fr['bits'][0, 4] == 0.75 and fr['bits'][0, 5] == 0.25 and fr['bits'][1, 11] == 0.25
    with pytest.raises(ValueError):
        persistence.frequency(t, 0)
    from arpeggio_amd.core import export
    lab = export.Labels(pc, pc.component_types)
    rec = persistence.to_records(t, pc)
    assert len(rec) == 2
    assert rec[0]['bgn'] == lab.atom_dict(0) and rec[0]['end'] == lab.atom_dict(1) and rec[1]['end'] == lab.atom_dict(5)
    assert rec[0]['n_models'] == 3 and rec[0]['first_model'] == 0 and rec[0]['last_model'] == 3
    assert rec[0]['contact'] == {'proximal': 3, 'hbond': 1} and rec[1]['contact'] == {'hydrophobic': 1}
    assert rec[0]['interacting_entities'] == ['INTRA_SELECTION', 'INTER'] and rec[0]['distance_sum'] == 10.0
    assert rec[0]['distance_mean'] == 10.0 / 3 and rec[0]['distance_min'] == 3.0 and rec[0]['distance_max'] == 3.5
    import json
    assert json.loads(json.dumps(rec)) == rec


def test_the_oracle_fixture_exercises_partial_persistence():
    """proteinlike40, F = 64, 5.0 A, whole structure, by the CPU oracle: the figures the GPU cases lean on."""
    pc = _hub()
    xyz, h_xyz = synth.models_of(pc, 64, seed=4, jitter=0.3)
    bags = _oracle_bags(pc, xyz, h_xyz)
    assert sum(len(b['i']) for b in bags) == 73118
    t = reference_table(bags, pc.n_atoms)
    assert len(t['a']) == 2832
    assert int((t['n_models'] == 64).sum()) == 296 and int((t['n_models'] == 1).sum()) == 311
    # rows whose records do not all carry the same SIFt: some bit is set in some but not all of the row's models
    mixed = ((t['bit_count'] > 0) & (t['bit_count'] < t['n_models'][:, None])).any(axis=1)
    assert int(mixed.sum()) == 1236


def test_stage_capacity_constant_matches_the_header():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert int(re.search(r'#define\s+ARP_PERSIST_STAGE_MAX\s+(\d+)', hdr).group(1)) == _capi.PERSIST_STAGE_MAX
    assert int(re.search(r'#define\s+ARP_PERSIST_BITS\s+(\d+)', hdr).group(1)) == _capi.PERSIST_BITS == persistence.N_BITS == 15
    assert tuple(k for k, _ in _capi.PERSIST_COLUMNS) == tuple(k for k, _ in persistence.COLUMNS)


# ------------------------------------------------------------------------------------------------------------- GPU
def _ctx_with_models(pc, xyz, h_xyz, sort_after=True):
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(sort_after)
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    return ctx


def _mask(pc, sel):
    from arpeggio_amd.core import utils
    m = np.zeros(pc.n_atoms, np.uint8)
    m[utils.selection_parser(sel, pc) if sel else np.arange(pc.n_atoms)] = 1
    return m


def _aa(per_model):
    return [m['atom_atom'] for m in per_model]


@pytest.mark.gpu
@pytest.mark.parametrize('name,make,F,jitter', CASES, ids=[c[0] for c in CASES])
def test_table_equals_the_reduction_of_the_per_model_bags(name, make, F, jitter):
    """Through EnsembleComplex (its own pass) and through Context (the same pass as the fetched bags): the table equals
    ``reference_table`` of the bags ``run_models`` returns; whole structure at 5.0 A also of the ORACLE's per-model bags."""
    from arpeggio_amd.core import EnsembleComplex
    pc = make()
    pc.ensure_labels()
    n = pc.n_atoms
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=jitter)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    rows = 0
    for params in PARAMS:
        for sel in _selectors(pc):
            what = (name, params, tuple(sel))
            ctx.set_selection(np.tile(_mask(pc, sel), F))
            want = reference_table(_aa(ctx.run_models(*params)), n)
            print(what, 'records', int(want['n_models'].astype(np.int64).sum()), 'rows', len(want['a']))
            _same(ctx.models_persistence(), want, what + ('context',))
            got = ens.run_persistence(sel, *params)
            _same(got, want, what + ('ensemble',))
            assert ens.persistence is got and ens.persistence_models == F and ens._results is None
            rows += len(want['a'])
            if F == 1:      # the table is the bag with counts 1
                bag = ctx.run_models(*params)[0]['atom_atom']
                assert np.array_equal(got['a'], bag['i']) and np.array_equal(got['b'], bag['j']) and np.all(got['n_models'] == 1)
                assert np.array_equal(got['dist_min'], bag['dist']) and np.array_equal(got['dist_max'], bag['dist'])
                assert np.array_equal(got['dist_sum'], bag['dist'].astype(np.float64))
                assert np.array_equal(got['bit_count'], ((bag['sift'][:, None] >> np.arange(15)) & 1).astype(np.uint16))
                assert np.array_equal(got['ctype_mask'], (1 << bag['ctype'].astype(np.int64)).astype(np.uint8))
            if params == PARAMS[0] and not sel:
                packs = [ens.model_pack(k) for k in range(F)]
                obags = []
                for q in packs:
                    oc = oracle.OracleComplex(q)
                    oc.make_selection(None)
                    obags.append(oc.atom_contacts(*params))
                _same(got, reference_table(obags, n), what + ('oracle',))
    assert rows > 0
    ctx.close()


@pytest.mark.gpu
def test_hub_atom_with_ten_thousand_records():
    """proteinlike40, F = 256, 7.5 A: 1 178 918 records in 8 072 rows, 13 769 of them on one bgn atom — beyond any per-atom
    stage (ARP_PERSIST_STAGE_MAX, 0 = the implementation has none): the general path is run, not assumed."""
    pc = _hub()
    F = 256
    while True:
        xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
        ctx = _ctx_with_models(pc, xyz, h_xyz)
        per = _aa(ctx.run_models(7.5, 0.1, False))
        heaviest = int(np.bincount(np.concatenate([b['i'] for b in per]), minlength=pc.n_atoms).max())
        if _capi.PERSIST_STAGE_MAX == 0 or heaviest > _capi.PERSIST_STAGE_MAX:
            break
        ctx.close()
        F *= 2
        assert F <= 65535
    got = ctx.models_persistence()
    want = reference_table(per, pc.n_atoms)
    print('hub: F', F, 'records', sum(len(b['i']) for b in per), 'rows', len(want['a']), 'heaviest atom', heaviest)
    if F == 256:
        assert sum(len(b['i']) for b in per) == 1178918 and len(want['a']) == 8072 and heaviest == 13769
    assert _capi.PERSIST_STAGE_MAX == 0 or heaviest > _capi.PERSIST_STAGE_MAX
    _same(got, want, 'hub')
    ctx.close()


@pytest.mark.gpu
def test_table_and_bags_do_not_depend_on_layout_sort_or_call_order():
    pc = synth.proteinlike(n_res=120, seed=11, n_waters=60)
    F = 12
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    plain = _ctx_with_models(pc, xyz, h_xyz, sort_after=False)      # never calls the reduction
    plain.run_launch(5.0, 0.1, False)
    bags0, _ = plain.fetch_packed()
    want = reference_table(_aa(_capi.split_models(bags0, plain._models)), pc.n_atoms)
    assert len(want['a']) > 1000
    for rows in (False, True):
        plain.set_packed_layout(rows)
        plain.run_launch(5.0, 0.1, False)
        ref_bags, _ = plain.fetch_packed()
        for sort_after in (False, True):
            for order in ('before', 'after', 'without', 'twice'):
                what = (rows, sort_after, order)
                ctx = _ctx_with_models(pc, xyz, h_xyz, sort_after=sort_after)
                ctx.set_packed_layout(rows)
                ctx.run_launch(5.0, 0.1, False)
                bags = None
                if order == 'after':
                    bags, _ = ctx.fetch_packed()
                t = ctx.models_persistence()
                if order == 'twice':
                    _same(ctx.models_persistence(), t, what)
                if order in ('before', 'twice'):
                    bags, _ = ctx.fetch_packed()
                _same(t, want, what)
                if bags is not None:
                    assert isinstance(bags['atom_atom'], _capi.RowsBag) == rows
                    if rows:
                        assert np.array_equal(bags['atom_atom']['row'], ref_bags['atom_atom']['row'])
                    for f, (g, w) in enumerate(zip(_capi.split_models(bags, ctx._models), _capi.split_models(ref_bags, plain._models))):
                        for name in w:
                            _same(g[name], w[name], what + (f, name))
                    aa = ctx.atom_contacts_fetch(len(bags0['atom_atom']['i']), sort=True)
                    _same({k: aa[k] for k in ('i', 'j', 'dist', 'sift', 'ctype')}, {k: np.asarray(bags0['atom_atom'][k]) for k in ('i', 'j', 'dist', 'sift', 'ctype')}, what + ('fetch',))
                    _same(ctx.models_persistence(), want, what + ('after the fetches',))
                ctx.close()
    plain.close()


@pytest.mark.gpu
def test_streaming_chunks_accumulate_to_the_merge_of_the_chunk_tables():
    from arpeggio_amd.core import EnsembleComplex
    pc = _hub()
    n = pc.n_atoms
    xyz, h_xyz = synth.models_of(pc, 48, seed=9, jitter=0.3)
    ens = EnsembleComplex((copy.copy(pc), xyz[:16], h_xyz[:16]))
    refs = []
    for c in range(3):
        lo, hi = 16 * c, 16 * (c + 1)
        if c:
            ens.set_coordinates(xyz[lo:hi], h_xyz[lo:hi])
        ens.run_arpeggio([], 5.0, 0.1, False)
        refs.append(reference_table([ens.model(k)._bags['atom_atom'] for k in range(16)], n))
        ens.run_persistence([], 5.0, 0.1, False, accumulate=True)
        assert ens.persistence_models == hi
    want = persistence.merge(persistence.merge(refs[0], refs[1], 16), refs[2], 32)
    _same(ens.persistence, want, 'streamed')
    one = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    whole = one.run_persistence([], 5.0, 0.1, False)
    for k in ('a', 'b', 'n_models', 'first', 'last', 'dist_min', 'dist_max', 'bit_count', 'ctype_mask'):
        _same({k: ens.persistence[k]}, {k: whole[k]}, ('one pass', k))
    # accumulate=False starts over
    ens.run_persistence([], 5.0, 0.1, False)
    assert ens.persistence_models == 16
    _same(ens.persistence, refs[2], 'restart')


@pytest.mark.gpu
def test_refusals_and_empty_tables():
    import ctypes as C
    pc = _hub()
    F = 6
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.run_launch(5.0, 0.1, False)
    with pytest.raises(ValueError, match='no models resident'):
        ctx.models_persistence()
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    with pytest.raises(ValueError, match='no results'):      # models resident, no pass yet
        ctx.models_persistence()
    ctx.run_launch(5.0, 0.1, False)
    t = ctx.models_persistence()
    U = len(t['a'])
    assert U > 100
    L, h = ctx._L, ctx._h
    n1, n2 = C.c_int64(-1), C.c_int64(-1)
    assert L.arp_models_persistence_launch(h, C.byref(n1)) == 0 and L.arp_models_persistence_launch(h, C.byref(n2)) == 0
    assert n1.value == n2.value == U
    # cap too small: ARP_E_CAPACITY with the count; then NULL columns are allowed
    cnt = C.c_int64(-1)
    a = np.full(U, -7, np.int32)
    assert L.arp_models_persistence_fetch(h, U - 1, _capi._p(a), *([None] * 9), C.byref(cnt)) == _capi.ARP_E_CAPACITY
    assert cnt.value == U and np.all(a == -7)
    assert L.arp_models_persistence_fetch(h, U, _capi._p(a), *([None] * 9), C.byref(cnt)) == 0 and np.array_equal(a, t['a'])
    # a selection change after the pass voids the table with the results
    ctx.set_selection(np.tile(_mask(pc, []), F))
    with pytest.raises(ValueError, match='no results'):
        ctx.models_persistence()
    assert L.arp_models_persistence_fetch(h, U, _capi._p(a), *([None] * 9), C.byref(cnt)) == _capi.ARP_E_ARG
    ctx.run_launch(5.0, 0.1, False)
    _same(ctx.models_persistence(), t, 'after the selection was set again')
    # a blob upload after the pass: no models resident any more
    ctx.set_blob(_capi.pack_blob(pc, pinned=False))
    with pytest.raises(ValueError, match='no models resident'):
        ctx.models_persistence()
    ctx.run_launch(5.0, 0.1, False)
    with pytest.raises(ValueError, match='no models resident'):
        ctx.models_persistence()
    # models without any contact: every atom of the selection_plus set alone (one water selected, far from everything)
    far = xyz.copy()
    hfar = h_xyz.copy()
    w = int(np.nonzero(np.array([pc.res_name[r] == 'HOH' for r in range(pc.n_residues)]))[0][0])
    atoms = np.nonzero(pc.res_id == w)[0]
    for a_ in atoms:
        far[:, a_] += np.float32(80.0)
        hfar[:, pc.h_off[a_]:pc.h_off[a_ + 1]] += 80.0
    ctx.set_topology(pc)
    ctx.set_models(far, hfar)
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[atoms] = 1
    ctx.set_selection(np.tile(sel, F))
    counts = ctx.run_launch(5.0, 0.1, False)
    assert counts['atom_atom'] == 0
    t0 = ctx.models_persistence()
    _same(t0, persistence.empty(), 'no contacts')
    assert L.arp_models_persistence_fetch(h, 0, *([None] * 10), C.byref(cnt)) == 0 and cnt.value == 0
    ctx.close()


@pytest.mark.gpu
def test_a_model_without_records_in_the_middle():
    """One water selected; in model 2 of 5 it is moved 50 A away from everything, so that model has no record at all."""
    from arpeggio_amd.core import EnsembleComplex
    pc = _hub()
    F = 5
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.1)
    waters = [r for r in range(pc.n_residues) if pc.res_name[r] == 'HOH']
    # a water with neighbours in every model (the oracle decides): the one with the most records
    best, atoms = -1, None
    for w in waters:
        at = np.nonzero(pc.res_id == w)[0]
        sel = np.zeros(pc.n_atoms, np.uint8)
        sel[at] = 1
        k = min(len(b['i']) for b in _oracle_bags(pc, xyz, h_xyz, sel=sel))
        if k > best:
            best, atoms = k, at
    assert best > 0
    for a_ in atoms:
        xyz[2, a_] += np.float32(50.0)
        h_xyz[2, pc.h_off[a_]:pc.h_off[a_ + 1]] += 50.0
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[atoms] = 1
    obags = _oracle_bags(pc, xyz, h_xyz, sel=sel)
    assert len(obags[2]['i']) == 0 and all(len(obags[k]['i']) > 0 for k in (0, 1, 3, 4))
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    got = ens.run_persistence(atoms, 5.0, 0.1, False)
    want = reference_table(obags, pc.n_atoms)
    _same(got, want, 'oracle')
    assert np.all(got['n_models'] <= 4) and got['n_models'].max() >= 2
    spans = got['last'] > got['first']
    assert spans.any() and np.all((got['first'] != 2) & (got['last'] != 2))
    ens.run_arpeggio(atoms, 5.0, 0.1, False)
    assert len(ens.model(2)._bags['atom_atom']['i']) == 0
    _same(got, reference_table([ens.model(k)._bags['atom_atom'] for k in range(F)], pc.n_atoms), 'run_models')
