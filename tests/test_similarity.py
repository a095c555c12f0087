"""Interaction-fingerprint similarity between the models of an ensemble, made on the device (arp_models_similarity_launch /
_fetch, Context.models_similarity, EnsembleComplex.run_similarity, arpeggio_amd.similarity).

The yardstick is never the device: it is ``reference_inter`` below — every model's features as a set of (row key, plane)
integers made from per-model bags that did not come through the new code (the bags ``run_models`` fetches and cuts, and the
oracle's), and ``inter[f][g] = len(np.intersect1d(...))``.  Every comparison is of exact integers.  No tolerance anywhere."""
import copy
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, contact_filter, similarity, synth, tables
from arpeggio_amd.core import config
from helpers import tiny_complex
from test_models import CASES, _selectors
from test_persistence import _ctx_with_models, _mask
from test_residue_pairs import PLANE_BAGS, _oracle_pass

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
NP_ = similarity.N_PLANES
ALL16 = similarity.ATOM_PLANES
ALL20 = (1 << NP_) - 1
DEFAULT = similarity.planes(None, ('atom_atom',))      # every contact but bare proximity, and "any atom-atom record"


# ------------------------------------------------------------------------------------------------------- the yardstick
def model_features(bags, planes, ctype_mask, n, res=None):
    """The features of one model as sorted unique integers key * 20 + plane.  ``bags``: the model's bags with model-local ids
    (only 'atom_atom' is read at atom level).  Atom level (``res`` None): key = i * n + j.  Residue level: ``res`` =
    (res_id, ring_res, amide_res) of the model, key = min(res) * nres + max(res) over all five bags, a record with a residue
    of -1 left out — the mapping of ``test_residue_persistence``'s reference (``test_residue_pairs.reference_table``)."""
    out = []
    aa = bags.get('atom_atom')
    if res is None:
        key_aa = None if aa is None else np.asarray(aa['i']).astype(np.int64) * n + np.asarray(aa['j']).astype(np.int64)
        keep_aa = None if aa is None else np.ones(len(key_aa), bool)
    else:
        tab = {'a': np.asarray(res[0], np.int64), 'r': np.asarray(res[1], np.int64), 'm': np.asarray(res[2], np.int64)}
        nres = int(n)

        def pair_key(ra, rb):
            return (ra >= 0) & (rb >= 0), np.minimum(ra, rb) * nres + np.maximum(ra, rb)
        keep_aa, key_aa = (None, None) if aa is None else pair_key(tab['a'][np.asarray(aa['i'])], tab['a'][np.asarray(aa['j'])])
        for m, (name, ka, kb, ta, tb) in enumerate(PLANE_BAGS):
            b = bags.get(name)
            q = similarity.CLASS_PLANE + 1 + m
            if b is not None and len(b[ka]) and (planes >> q) & 1:
                keep, key = pair_key(tab[ta][np.asarray(b[ka])], tab[tb][np.asarray(b[kb])])
                out.append(key[keep] * NP_ + q)
    if aa is not None and len(key_aa):
        takes_part = keep_aa & (((ctype_mask >> np.asarray(aa['ctype']).astype(np.int64)) & 1) != 0)
        has = (np.asarray(aa['sift']).astype(np.int64) & 0x7FFF) | (1 << similarity.CLASS_PLANE)
        for q in range(similarity.CLASS_PLANE + 1):
            if (planes >> q) & 1:
                out.append(key_aa[takes_part & (((has >> q) & 1) != 0)] * NP_ + q)
    return np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)


def inter_of(features):
    F = len(features)
    m = np.zeros((F, F), np.uint32)
    for f in range(F):
        for g in range(f, F):
            m[f, g] = m[g, f] = len(np.intersect1d(features[f], features[g], assume_unique=True))
    return m


def reference_inter(per_model_bags, planes, ctype_mask, n, res=None):
    """uint32 [F, F] of per-model bags; ``res``: per model (res_id, ring_res, amide_res) for the residue level, ``n`` then the
    residues of a model."""
    return inter_of([model_features(b, planes, ctype_mask, n, None if res is None else res[f]) for f, b in enumerate(per_model_bags)])


def _bag(i, j, sift, ctype):
    return dict(i=np.array(i, np.int32), j=np.array(j, np.int32), dist=np.zeros(len(i), np.float32), sift=np.array(sift, np.uint16),
                ctype=np.array(ctype, np.uint8))


# ------------------------------------------------------------------------------------------------------------- CPU
def test_reference_on_hand_made_bags():
    """Three models over 6 atoms.  (0, 1) is in all three with differing SIFt; (2, 3) in model 0 only; model 1 is empty but for
    ... nothing: it has no record; (1, 4) in models 0 and 2, in model 2 with a contact type the mask excludes."""
    H, V, P = BIT['hbond'], BIT['vdw'], BIT['proximal']
    INTER, INTRA = CT['INTER'], CT['INTRA_NON_SELECTION']
    m0 = {'atom_atom': _bag([0, 2, 1], [1, 3, 4], [H | P, V, H], [INTER, INTER, INTER])}
    m1 = {'atom_atom': _bag([], [], [], [])}
    m2 = {'atom_atom': _bag([0, 1], [1, 4], [P, H], [INTER, INTRA])}
    planes = H | V | P | (1 << 15)
    # model 0: (0,1){H,P,aa} (2,3){V,aa} (1,4){H,aa} = 7 features; model 2, all types: (0,1){P,aa} (1,4){H,aa} = 4
    want_all = [[7, 0, 4], [0, 0, 0], [4, 0, 4]]
    assert reference_inter([m0, m1, m2], planes, 0x7F, 6).tolist() == want_all
    # INTER only: model 2 loses (1, 4): (0,1){P,aa} = 2, all shared with model 0
    assert reference_inter([m0, m1, m2], planes, 1 << INTER, 6).tolist() == [[7, 0, 2], [0, 0, 0], [2, 0, 2]]
    # the hbond plane alone: model 0 (0,1), (1,4); model 2 (1,4) — under INTER only, none
    assert reference_inter([m0, m1, m2], H, 0x7F, 6).tolist() == [[2, 0, 1], [0, 0, 0], [1, 0, 1]]
    assert reference_inter([m0, m1, m2], H, 1 << INTER, 6).tolist() == [[2, 0, 0], [0, 0, 0], [0, 0, 0]]
    # residue level: atoms in residues [0, 0, 1, 1, 2, 2], one ring of residue 2 and one of none; an atom-plane record each
    res = ([0, 0, 1, 1, 2, 2], [2, -1], [])
    r0 = dict(m0, atom_plane=dict(atom=np.array([0, 1], np.int32), ring=np.array([0, 1], np.int32)))
    r2 = dict(m2, atom_plane=dict(atom=np.array([1], np.int32), ring=np.array([0], np.int32)))
    # model 0 rows: (0,0){H,P,aa} (1,1){V,aa} (0,2){H,aa; atom_plane} — the record on ring 1 is left out; model 2: (0,0){P,aa} (0,2){H,aa; atom_plane}
    got = reference_inter([r0, m1, r2], planes | (1 << 16), 0x7F, 3, [res] * 3)
    assert got.tolist() == [[8, 0, 5], [0, 0, 0], [5, 0, 5]]


def test_planes_names_and_errors():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert int(re.search(r'#define\s+ARP_SIM_PLANES\s+(\d+)', hdr).group(1)) == similarity.N_PLANES == _capi.SIM_PLANES == 20
    assert int(re.search(r'#define\s+ARP_SIM_MAX_MODELS\s+(\d+)', hdr).group(1)) == similarity.MAX_MODELS == _capi.SIM_MAX_MODELS == 4096
    assert int(re.search(r'#define\s+ARP_SIM_BY_RESIDUE\s+(\d+)u', hdr).group(1)) == similarity.BY_RESIDUE == _capi.SIM_BY_RESIDUE == 1
    for s in ('arp_models_similarity_launch', 'arp_models_similarity_fetch'):
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    assert similarity.planes() == contact_filter.SPECIFIC[0] == 0x7FEF
    assert similarity.planes(['hbond', 'aromatic'], ['atom_atom']) == BIT['hbond'] | BIT['aromatic'] | (1 << 15)
    assert similarity.planes('hbond') == BIT['hbond'] and similarity.planes([], 'group_plane') == 1 << 19
    assert similarity.planes(config.SIFT_NAMES[:15], tables.CLASSES) == ALL20 and similarity.ATOM_PLANES == 0xFFFF
    for k, name in enumerate(tables.CLASSES):
        assert similarity.planes([], [name]) == 1 << (15 + k)
    with pytest.raises(ValueError, match='hbonds'):
        similarity.planes(['hbond', 'hbonds'])
    with pytest.raises(ValueError, match='ring_ring'):
        similarity.planes(None, ['ring_ring'])
    with pytest.raises(ValueError, match='no plane'):
        similarity.planes([], ())


def test_tanimoto_distance_and_medoid():
    inter = np.array([[4, 2, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint32)
    assert similarity.counts(inter).tolist() == [4, 2, 0, 0]
    t = similarity.tanimoto(inter)
    assert t.dtype == np.float64
    assert t.tolist() == [[1.0, 0.5, 0.0, 0.0], [0.5, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]]      # empty-empty: 1.0
    assert similarity.distance(inter).tolist() == (1.0 - t).tolist()
    assert similarity.medoid(inter) == 2                  # sums 1.5, 1.5, 2, 2: the lowest index of the tie
    assert similarity.medoid(np.array([[3, 1], [1, 3]], np.uint32)) == 0
    three = np.array([[4, 1, 1], [1, 4, 3], [1, 3, 4]], np.uint32)
    assert similarity.medoid(three) == 1 and similarity.tanimoto(three)[1, 2] == 3 / 5
    big = np.array([[4000000000, 4000000000], [4000000000, 4000000000]], np.uint32)      # (no uint32 wrap in n_f + n_g - I)
    assert similarity.tanimoto(big).tolist() == [[1.0, 1.0], [1.0, 1.0]]
    with pytest.raises(ValueError):
        similarity.tanimoto(np.zeros((2, 3), np.uint32))


def test_write_csv_and_records(tmp_path):
    inter = np.array([[3, 1, 0], [1, 3, 2], [0, 2, 2]], np.uint32)
    p = similarity.write_similarity(str(tmp_path), 'ens', inter)
    assert os.path.basename(p) == 'ens.modelsim'
    assert open(p, newline='').read() == ('f,g,shared,n_f,n_g,tanimoto\r\n0,1,1,3,3,0.2\r\n0,2,0,3,2,0.0\r\n1,2,2,3,2,' + repr(2 / 3) + '\r\n')
    rec = similarity.to_records(inter, ['1', '2', '5'])
    assert rec[2] == {'bgn': '2', 'end': '5', 'type': 'model-similarity', 'shared': 2, 'n_bgn': 3, 'n_end': 2, 'tanimoto': 2 / 3}
    assert len(rec) == 3 and similarity.to_records(inter)[0]['end'] == 1


# ------------------------------------------------------------------------------------------------------------- GPU
def _chain(n):
    """``n`` atoms on a line 3 A apart, a residue each (no polypeptide: no sequence-adjacency filter): at 5 A the records are
    the n - 1 neighbour pairs."""
    return tiny_complex(np.stack([3.0 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1))


def _aa_only(per_model):
    return [{'atom_atom': m['atom_atom']} for m in per_model]


@pytest.mark.gpu
@pytest.mark.parametrize('U', [63, 64, 65, 129])
def test_word_seams(U):
    """A chain of U + 1 atoms in three models; atom 40 of model 1 is 50 A away, so that model lacks exactly the rows (39, 40)
    and (40, 41).  U rows end inside, at the end of and one past a 64-bit word."""
    n, F = U + 1, 3
    pc = _chain(n)
    xyz = np.repeat(np.asarray(pc.xyz, np.float32)[None], F, axis=0)
    xyz[1, 40, 1] += np.float32(50.0)
    h_xyz = np.zeros((F, 0, 3))
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    per = ctx.run_models(5.0, 0.1, True)
    assert [len(m['atom_atom']['i']) for m in per] == [U, U - 2, U]
    opacks = []
    for f in range(F):
        q = copy.copy(pc)
        q.xyz = np.ascontiguousarray(xyz[f])
        opacks.append({'atom_atom': _oracle_pass(q, (5.0, 0.1, True))['atom_atom']})
    for planes in (ALL16, 1 << 15, DEFAULT):
        got = ctx.models_similarity(planes)
        st = ctx.stats()
        assert st['sim_rows'] == U == n - 1 and st['sim_words'] == bin(planes).count('1') * ((U + 63) // 64)
        want = reference_inter(_aa_only(per), planes, 0x7F, n)
        assert np.array_equal(got, want) and got.dtype == np.uint32, (U, planes)
        assert np.array_equal(got, reference_inter(opacks, planes, 0x7F, n)), (U, planes, 'oracle')
        if planes == 1 << 15:
            assert got.tolist() == [[U, U - 2, U], [U - 2, U - 2, U - 2], [U, U - 2, U]]
    ctx.close()


F_TILES = 130


@functools.lru_cache(maxsize=None)
def _tile_models():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    pc.ensure_labels()
    return (pc,) + tuple(synth.models_of(pc, F_TILES, seed=4, jitter=0.3))


@functools.lru_cache(maxsize=None)
def _tile_reference(cutoff):
    """The features of all F_TILES models at a cutoff, from the bags run_models fetches, and their matrix: made once; a case of
    F models compares with its leading block (model f of ``models_of`` does not depend on F)."""
    pc, xyz, h_xyz = _tile_models()
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    feats = [model_features(m, DEFAULT, 0x7F, pc.n_atoms) for m in ctx.run_models(cutoff, 0.1, False)]
    ctx.close()
    return feats, inter_of(feats)


@pytest.mark.gpu
@pytest.mark.parametrize('cutoff', [5.0, 7.5])
@pytest.mark.parametrize('F', [1, 2, 63, 64, 65, 130])
def test_tile_seams(F, cutoff):
    """One ragged tile, one full tile, a diagonal + an off-diagonal + ragged tiles, three tile rows; at 7.5 A (the hub case) the
    words are many enough for more than one slice: the atomic-add path."""
    pc, xyz, h_xyz = _tile_models()
    feats, want = _tile_reference(cutoff)
    ctx = _ctx_with_models(pc, xyz[:F], h_xyz[:F])
    per = ctx.run_models(cutoff, 0.1, False)
    for f in range(F):      # the yardstick's inputs for these F models are those the shared reference was made from
        assert np.array_equal(model_features(per[f], DEFAULT, 0x7F, pc.n_atoms), feats[f]), f
    got = ctx.models_similarity(DEFAULT)
    st = ctx.stats()
    print('F', F, 'cutoff', cutoff, st)
    assert got.shape == (F, F) and np.array_equal(got, got.T)
    assert np.diagonal(got).tolist() == [len(x) for x in feats[:F]]
    assert np.array_equal(got, want[:F, :F])
    if cutoff == 7.5:
        assert st['sim_slices'] > 1
    assert st['sim_words'] == bin(DEFAULT).count('1') * ((st['sim_rows'] + 63) // 64)
    ctx.close()


@pytest.mark.gpu
def test_plane_handling():
    pc, xyz, h_xyz = _tile_models()
    F = 9
    ctx = _ctx_with_models(pc, xyz[:F], h_xyz[:F])
    lig = _selectors(pc)[2]
    for sel, ctype_mask in (([], 0x7F), (lig, 1 << CT['INTER']), (lig, 0x7F)):
        ctx.set_selection(np.tile(_mask(pc, sel), F))
        per = _aa_only(ctx.run_models(5.0, 0.1, False))
        types = np.concatenate([m['atom_atom']['ctype'] for m in per])
        if sel:
            assert (types == CT['INTER']).any() and (types != CT['INTER']).any()      # the mask has something to exclude
        for planes in (similarity.planes(['hbond', 'aromatic'], ['atom_atom']), BIT['hbond'], BIT['proximal'], 1 << 15, ALL16):
            got = ctx.models_similarity(planes, ctype_mask)
            want = reference_inter(per, planes, ctype_mask, pc.n_atoms)
            assert np.array_equal(got, want), (sel, ctype_mask, planes)
            assert want.any() or planes not in (1 << 15, ALL16)
    ctx.close()


@pytest.mark.gpu
def test_residue_level():
    """CASES[0] (proteinlike120, F = 20), three selections, all 20 planes, against the yardstick over run_models' bags — and,
    whole structure, over the oracle's.  Its (row, model) cells hold several records.  It has no left-out record and cannot
    have one: a ring has atoms within 3 A of its centre in every model, so no ring_res is -1, and a ring or amide without a
    residue is in no selection set of a pass.  Left-out records are the case of the test below."""
    from arpeggio_amd.core import EnsembleComplex
    name, make, F, jitter = CASES[0]
    pc = make()
    pc.ensure_labels()
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=jitter)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    ctx = ens._ctx
    packs = [ens.model_pack(f) for f in range(F)]
    res = [(q.res_id, q.ring_res, q.amide_res) for q in packs]
    several = False
    for sel in _selectors(pc):
        ctx.set_selection(np.tile(_mask(pc, sel), F))
        per = ctx.run_models(5.0, 0.1, False)
        for f, m in enumerate(per):
            assert (np.asarray(res[f][1]) >= 0).all() and (np.asarray(res[f][2]) >= 0).all()
            ra, rb = res[f][0][m['atom_atom']['i']], res[f][0][m['atom_atom']['j']]
            cells = np.minimum(ra, rb).astype(np.int64) * pc.n_residues + np.maximum(ra, rb)
            several |= len(np.unique(cells)) < len(cells)
        want = reference_inter(per, ALL20, 0x7F, pc.n_residues, res)
        got = ctx.models_similarity(ALL20, by_residue=True)
        assert np.array_equal(got, want), sel
        assert want.any() and (np.diagonal(want) > 0).all()
        if not sel:
            obags = [_oracle_pass(q) for q in packs]
            assert np.array_equal(got, reference_inter(obags, ALL20, 0x7F, pc.n_residues, res)), 'oracle'
            # the class planes alone, and an INTER-only atom-atom part beside them
            for planes, ctm in ((0x1F << 15, 0x7F), (ALL20, 1 << CT['INTRA_NON_SELECTION'])):
                assert np.array_equal(ctx.models_similarity(planes, ctm, by_residue=True), reference_inter(per, planes, ctm, pc.n_residues, res))
        via = ens.run_similarity(sel, 5.0, 0.1, False, contacts=config.SIFT_NAMES[:15], classes=tables.CLASSES, level='residue')
        assert np.array_equal(via, want), (sel, 'ensemble')
    assert several      # (row, model) cells with several records


@pytest.mark.gpu
def test_residue_level_leaves_out_records_without_a_residue():
    """``test_residue_persistence.seam_sentinel_tie`` in four models with an installed selection state and the five bags
    launched one by one (a complete pass): the group-group records of the amide without a residue (-1) are left out, and the
    pair (3, 3) of model 3 — all ones in the bits of (res_a, res_b, f) — is a row like any other."""
    from test_residue_persistence import _translated, seam_sentinel_tie
    pc = seam_sentinel_tie()
    F = 4
    xyz, h_xyz = _translated(pc, F)
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    ones = lambda k: np.ones(F * k, np.uint8)
    ctx.set_selection_state(ones(pc.n_atoms), ones(pc.n_atoms), ones(pc.n_rings), ones(pc.n_rings), ones(pc.n_amides), ones(pc.n_amides))
    ctx.atom_contacts_launch(5.0, 0.1, False)
    bags = {name: (ctx.launch_bag(name), ctx.fetch_bag(name))[1] for name, *_ in PLANE_BAGS}
    bags['atom_atom'] = ctx.atom_contacts_fetch(F * pc.n_atoms * pc.n_atoms)
    per = _capi.split_models(bags, ctx._models)
    res = [(pc.res_id, pc.ring_res, pc.amide_res)] * F
    for f, m in enumerate(per):      # the yardstick's inputs: left-out records and kept ones of (3, 3) in every model
        gg = np.stack([pc.amide_res[m['group_group']['bgn']], pc.amide_res[m['group_group']['end']]], axis=1)
        assert (gg.min(axis=1) < 0).any() and (gg == 3).all(axis=1).any(), f
    for planes in (ALL20, 1 << 18, (1 << 18) | (1 << 15)):
        got = ctx.models_similarity(planes, by_residue=True)
        want = reference_inter(per, planes, 0x7F, pc.n_residues, res)
        assert np.array_equal(got, want) and (np.diagonal(want) > 0).all(), planes
    assert ctx.models_similarity(1 << 18, by_residue=True).tolist() == [[1] * F] * F      # the one row (3, 3), in every model
    ctx.close()


@pytest.mark.gpu
def test_a_model_without_records_in_the_middle():
    """One water selected; in model 2 of 5 it is 50 A away from everything: a zero row and a zero column."""
    pc, xyz, h_xyz = _tile_models()
    F = 5
    xyz, h_xyz = xyz[:F].copy(), h_xyz[:F].copy()
    w = [r for r in range(pc.n_residues) if pc.res_name[r] == 'HOH'][0]
    atoms = np.nonzero(pc.res_id == w)[0]
    # beside a protein atom in every model, so that every other model has records
    anchor = int(np.nonzero(pc.res_id == 0)[0][0])
    for f in range(F):
        shift = xyz[f, anchor] + np.array([3.0, 0.0, 0.0], np.float32) - xyz[f, atoms[0]]
        xyz[f, atoms] += shift
        for a_ in atoms:
            h_xyz[f, pc.h_off[a_]:pc.h_off[a_ + 1]] += shift.astype(np.float64)
    for a_ in atoms:
        xyz[2, a_] += np.float32(50.0)
        h_xyz[2, pc.h_off[a_]:pc.h_off[a_ + 1]] += 50.0
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[atoms] = 1
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    ctx.set_selection(np.tile(sel, F))
    per = _aa_only(ctx.run_models(5.0, 0.1, False))
    assert len(per[2]['atom_atom']['i']) == 0 and all(len(per[k]['atom_atom']['i']) > 0 for k in (0, 1, 3, 4))
    got = ctx.models_similarity(ALL16)
    assert np.array_equal(got, reference_inter(per, ALL16, 0x7F, pc.n_atoms))
    assert not got[2].any() and not got[:, 2].any() and all(got[k, k] > 0 for k in (0, 1, 3, 4))
    obags = []
    for f in range(F):
        q = copy.copy(pc)
        q.xyz, q.h_xyz = np.ascontiguousarray(xyz[f]), np.ascontiguousarray(h_xyz[f])
        oc = oracle.OracleComplex(q)
        oc.make_selection(sel)
        obags.append({'atom_atom': oc.atom_contacts(5.0, 0.1, False)})
    assert np.array_equal(got, reference_inter(obags, ALL16, 0x7F, pc.n_atoms)), 'oracle'
    # every model without records: an all-zero matrix, no rows
    far = xyz.copy()
    hfar = h_xyz.copy()
    for a_ in atoms:
        far[:, a_] += np.float32(80.0)
        hfar[:, pc.h_off[a_]:pc.h_off[a_ + 1]] += 80.0
    ctx.set_models(far, hfar)
    ctx.set_selection(np.tile(sel, F))
    assert ctx.run_launch(5.0, 0.1, False)['atom_atom'] == 0
    for by_res in (False, True):
        z = ctx.models_similarity(ALL16, by_residue=by_res)
        assert z.shape == (F, F) and not z.any() and ctx.stats()['sim_rows'] == 0
    ctx.close()


def _everything(ctx):
    """The five bags and the two persistence tables as bytes."""
    bags, _ = ctx.fetch_packed()
    out = {(name, k): np.asarray(v).tobytes() for name, b in bags.items() if isinstance(b, dict) for k, v in b.items()}
    for name, t in (('persist', ctx.models_persistence()), ('respersist', ctx.models_residue_persistence())):
        out.update({(name, k): v.tobytes() for k, v in t.items()})
    return out


@pytest.mark.gpu
def test_nothing_else_changes_and_a_second_launch_does_no_work():
    pc, xyz, h_xyz = _tile_models()
    F = 6
    xyz, h_xyz = xyz[:F], h_xyz[:F]
    plain = _ctx_with_models(pc, xyz, h_xyz, sort_after=False)      # never calls the new code
    per = plain.run_models(5.0, 0.1, False)
    planes_dev = plain.models_planes()
    res = [(pc.res_id, planes_dev['ring_res'][f], pc.amide_res) for f in range(F)]
    want_atom = reference_inter(_aa_only(per), DEFAULT, 0x7F, pc.n_atoms)
    want_hb = reference_inter(_aa_only(per), BIT['hbond'], 0x7F, pc.n_atoms)
    want_res = reference_inter(per, ALL20, 0x7F, pc.n_residues, res)
    assert not np.array_equal(want_atom, want_hb)
    for rows in (False, True):
        plain.set_packed_layout(rows)
        plain.run_launch(5.0, 0.1, False)
        ref = _everything(plain)
        for sort_after, order in itertools.product((False, True), ('fetch first', 'similarity first')):
            what = (rows, sort_after, order)
            ctx = _ctx_with_models(pc, xyz, h_xyz, sort_after=sort_after)
            ctx.set_packed_layout(rows)
            ctx.run_launch(5.0, 0.1, False)
            if order == 'fetch first':
                assert _everything(ctx) == ref, what
            n0 = ctx.stats()['sim_launches']
            got = ctx.models_similarity(DEFAULT)
            assert np.array_equal(got, want_atom), what
            st = ctx.stats()
            assert st['sim_launches'] == n0 + 1
            assert np.array_equal(ctx.models_similarity(DEFAULT), got) and ctx.stats() == st, what      # the resident matrix
            assert _everything(ctx) == ref, what
            assert np.array_equal(ctx.models_similarity(DEFAULT), got) and ctx.stats() == st, what      # no table voided it
            assert np.array_equal(ctx.models_similarity(BIT['hbond']), want_hb) and ctx.stats()['sim_launches'] == n0 + 2      # other arguments
            assert np.array_equal(ctx.models_similarity(ALL20, by_residue=True), want_res) and ctx.stats()['sim_launches'] == n0 + 3
            assert np.array_equal(ctx.models_similarity(ALL20, 1 << CT['INTER'], by_residue=True),
                                  reference_inter(per, ALL20, 1 << CT['INTER'], pc.n_residues, res))
            assert _everything(ctx) == ref, what
            ctx.run_launch(5.0, 0.1, False)      # a new pass voids it: made again
            assert np.array_equal(ctx.models_similarity(ALL20, 1 << CT['INTER'], by_residue=True),
                                  reference_inter(per, ALL20, 1 << CT['INTER'], pc.n_residues, res))
            assert ctx.stats()['sim_launches'] == n0 + 5
            ctx.close()
    plain.close()


@pytest.mark.gpu
def test_refusals():
    pc, xyz, h_xyz = _tile_models()
    F = 4
    xyz, h_xyz = xyz[:F], h_xyz[:F]
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.run_launch(5.0, 0.1, False)
    with pytest.raises(ValueError, match='no models resident'):
        ctx.models_similarity(DEFAULT)
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    with pytest.raises(ValueError, match='no results'):
        ctx.models_similarity(DEFAULT)
    L, h = ctx._L, ctx._h
    nm, nr = C.c_int64(-1), C.c_int64(-1)
    buf = np.full((F, F), 7, np.uint32)
    assert L.arp_models_similarity_fetch(h, F, _capi._p(buf), C.byref(nm)) == _capi.ARP_E_ARG      # nothing launched
    ctx.atom_contacts_launch(5.0, 0.1, False)      # the atom-atom bag alone: atom level runs, residue level refuses
    got = ctx.models_similarity(DEFAULT)
    assert got.any()
    with pytest.raises(ValueError, match='complete pass'):
        ctx.models_similarity(DEFAULT, by_residue=True)
    for planes, ctm, flags, what in ((0, 0x7F, 0, 'planes'), (1 << 20, 0x7F, 0, 'planes'), (1 << 16, 0x7F, 0, 'residue level only'),
                                     (ALL20, 0x7F, 0, 'residue level only'), (DEFAULT, 0, 0, 'ctype_mask'), (DEFAULT, 0x80, 0, 'ctype_mask'),
                                     (DEFAULT, 0x7F, 2, 'unknown flag'), (ALL20, 0x7F, 3, 'unknown flag')):
        assert L.arp_models_similarity_launch(h, planes, ctm, flags, C.byref(nm), C.byref(nr)) == _capi.ARP_E_ARG, what
        assert what in L.arp_last_error(h).decode(), what
    # a refused launch leaves the resident matrix; a small cap: ARP_E_CAPACITY with F, nothing written
    assert L.arp_models_similarity_fetch(h, F - 1, _capi._p(buf), C.byref(nm)) == _capi.ARP_E_CAPACITY
    assert nm.value == F and (buf == 7).all()
    assert L.arp_models_similarity_fetch(h, F, _capi._p(buf), C.byref(nm)) == _capi.ARP_OK and np.array_equal(buf, got)
    # a selection change voids it with the results
    ctx.set_selection(np.tile(_mask(pc, []), F))
    with pytest.raises(ValueError, match='no results'):
        ctx.models_similarity(DEFAULT)
    assert L.arp_models_similarity_fetch(h, F, _capi._p(buf), C.byref(nm)) == _capi.ARP_E_ARG
    ctx.close()
    # a shard
    c2 = _capi.Context(0)
    c2.set_complex(pc)
    c2.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    with pytest.raises(ValueError, match='shard'):
        c2.models_similarity(DEFAULT)
    c2.close()
    # more models than ARP_SIM_MAX_MODELS: refused at the launch, before anything is sized
    two = tiny_complex([(0.0, 0.0, 0.0), (3.0, 0.0, 0.0)])
    many = similarity.MAX_MODELS + 1
    c3 = _ctx_with_models(two, np.repeat(np.asarray(two.xyz, np.float32)[None], many, axis=0), np.zeros((many, 0, 3)))
    assert c3._L.arp_models_similarity_launch(c3._h, 1 << 15, 0x7F, 0, C.byref(nm), C.byref(nr)) == _capi.ARP_E_CAPACITY
    assert nm.value == many and '4096' in c3._L.arp_last_error(c3._h).decode()
    c3.close()


@pytest.mark.gpu
def test_run_similarity_and_write_similarity(tmp_path):
    """CASES[3] (proteinlike40, F = 64) end to end: the matrix, the CSV text and the medoid."""
    from arpeggio_amd.core import EnsembleComplex
    name, make, F, jitter = CASES[3]
    pc = make()
    pc.ensure_labels()
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=jitter)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    with pytest.raises(AttributeError, match='run_similarity first'):
        ens.write_similarity(str(tmp_path))
    with pytest.raises(ValueError, match='residue'):
        ens.run_similarity([], 5.0, 0.1, False, classes=('plane_plane',))
    lig = _selectors(pc)[2]
    for sel, kw, planes, ctm in (([], {}, contact_filter.SPECIFIC[0], 0x7F),
                                 (lig, dict(contacts=('hbond', 'vdw', 'hydrophobic'), classes=('atom_atom',), interacting_entities=('INTER',)),
                                  BIT['hbond'] | BIT['vdw'] | BIT['hydrophobic'] | (1 << 15), 1 << CT['INTER'])):
        got = ens.run_similarity(sel, 5.0, 0.1, False, **kw)
        assert ens.similarity is got and got.shape == (F, F) and ens._results is None and ens.similarity_rows == ens.stats['sim_rows'] > 0
        per = _aa_only(ens._ctx.run_models(5.0, 0.1, False))
        want = reference_inter(per, planes, ctm, pc.n_atoms)
        assert np.array_equal(got, want) and want.any(), sel
        p = ens.write_similarity(str(tmp_path))
        assert os.path.basename(p) == ens.id + '.modelsim'
        lines = open(p, newline='').read().split('\r\n')
        assert lines[0] == 'f,g,shared,n_f,n_g,tanimoto' and len(lines) == F * (F - 1) // 2 + 2 and lines[-1] == ''
        w = want.astype(np.int64)
        n_ = np.diagonal(w)
        at = 1
        for f in range(F):
            for g in range(f + 1, F):
                u = int(n_[f] + n_[g] - w[f, g])
                assert lines[at] == '%d,%d,%d,%d,%d,%s' % (f, g, w[f, g], n_[f], n_[g], repr(float(w[f, g] / u) if u else 1.0)), (f, g)
                at += 1
        t = np.array([[1.0 if f == g or not (n_[f] + n_[g] - w[f, g]) else w[f, g] / (n_[f] + n_[g] - w[f, g]) for g in range(F)] for f in range(F)])
        assert similarity.medoid(got) == int(np.argmax(t.sum(axis=1)))
