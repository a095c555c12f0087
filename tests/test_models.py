"""Every model of a multi-model structure in one pass (arp_set_topology / arp_set_models, core.EnsembleComplex,
protein_reader.read_mmcif_models).  The reference keeps the first model only (protein_reader.py:67-69); here each model's
five bags, selection sets and plane geometry must be bit-identical to the single-structure run of that model
(InteractionComplex with its plane geometry computed on the GPU), and the reader must give every model of a file with
model 1's topology."""
import copy
import json
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, batch, synth
from arpeggio_amd.core import protein_reader

BAGS = ('atom_atom', 'atom_plane', 'plane_plane', 'group_group', 'group_plane')


def _cif_models(pc, xyz):
    """mmCIF text with one model per coordinate set of ``xyz`` [F, n, 3] (explicit hydrogens are atoms of ``pc``)."""
    pc.ensure_labels()
    head = ['group_PDB', 'id', 'type_symbol', 'label_atom_id', 'label_alt_id', 'label_comp_id', 'label_asym_id', 'label_entity_id',
            'label_seq_id', 'pdbx_PDB_ins_code', 'Cartn_x', 'Cartn_y', 'Cartn_z', 'occupancy', 'B_iso_or_equiv', 'auth_seq_id',
            'auth_asym_id', 'pdbx_PDB_model_num']
    rows = []
    n = pc.n_atoms
    for f in range(len(xyz)):
        for i in range(n):
            r = int(pc.res_id[i])
            het = pc.res_name[r] in ('HOH', 'HEM')
            name = pc.atom_name[i]
            q = '"' + name + '"' if "'" in name else name
            rows.append(' '.join(['HETATM' if het else 'ATOM', str(f * n + i + 1), pc.element[i].upper(), q, '.', pc.res_name[r],
                                  pc.res_chain[r], '1', str(int(pc.res_seq[r])), '?'] +
                                 ['%.3f' % float(v) for v in xyz[f, i].astype(np.float64)] +
                                 ['1.00', '10.00', str(int(pc.res_seq[r])), pc.res_chain[r], str(f + 1)]))
    return 'data_synth\n_entry.id SYNTH\nloop_\n' + ''.join('_atom_site.' + h + '\n' for h in head) + '\n'.join(rows) + '\n'


def _same_topology(a, b, serial=True):
    for name in protein_reader._TOPOLOGY + ('res_seq', 'vdw', 'cov', 'flags') + (('serial',) if serial else ()):
        x, y = getattr(a, name), getattr(b, name)
        if name == 'ring_atoms':
            assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)), name
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), name


# ------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('n_res,seed,F', [(40, 21, 8), (120, 11, 3)])
def test_read_mmcif_models_gives_every_model_with_the_first_models_topology(tmp_path, n_res, seed, F):
    pc0 = synth.proteinlike(n_res=n_res, seed=seed, n_waters=20)
    xyz, _ = synth.models_of(pc0, F, seed=3)
    p = tmp_path / 'ens.cif'
    p.write_text(_cif_models(pc0, xyz))
    pc, mx, mh, numbers = protein_reader.read_mmcif_models(str(p))
    assert numbers == [str(k) for k in range(1, F + 1)] and mx.shape == (F, pc0.n_atoms, 3) and mx.dtype == np.float32
    first = protein_reader.read_mmcif(str(p))                         # read_mmcif on the multi-model file: model 1, as before
    _same_topology(pc, first)
    assert np.array_equal(pc.xyz, first.xyz) and np.array_equal(pc.h_xyz, first.h_xyz)
    text = np.round(xyz.astype(np.float64), 3).astype(np.float32)       # each model's three-decimal text
    for k in range(F):
        assert np.array_equal(mx[k], text[k]), k
        one = protein_reader.read_mmcif(str(p), model=k + 1)          # the model read alone: same topology, its hydrogens in CSR order
        _same_topology(one, pc, serial=k == 0)      # (atom ids differ from model to model)
        assert np.array_equal(mh[k], one.h_xyz.reshape(-1, 3)), k
        is_h = np.array([e in ('H', 'D') for e in pc.element])
        owner = np.repeat(np.arange(pc.n_atoms), np.diff(pc.h_off))
        # the hydrogens of atom a (h_off CSR) sit at the coordinates of the explicit hydrogens whose parent is a
        kids = np.nonzero(is_h)[0]
        for a in np.unique(owner)[:20]:
            want = sorted(map(tuple, np.round(text[k][kids[pc.hydrogen_parent[kids] == a]].astype(np.float64), 3)))
            got = sorted(map(tuple, np.round(mh[k][owner == a], 3)))
            assert want == got, (k, a)
    # one model -> F = 1, equal to read_mmcif
    q = tmp_path / 'one.cif'
    q.write_text(_cif_models(pc0, xyz[:1]))
    pc1, x1, h1, n1 = protein_reader.read_mmcif_models(str(q))
    assert x1.shape[0] == 1 and n1 == ['1'] and np.array_equal(x1[0], first.xyz) and np.array_equal(h1[0], first.h_xyz)
    _same_topology(pc1, first)


def test_read_mmcif_models_names_the_model_whose_topology_differs(tmp_path):
    pc0 = synth.proteinlike(n_res=40, seed=21, n_waters=10)
    xyz, _ = synth.models_of(pc0, 4, seed=5)
    text = _cif_models(pc0, xyz)
    # model 2 lacks an atom
    lines = text.splitlines()
    n = pc0.n_atoms
    head = [k for k, ln in enumerate(lines) if ln.startswith(('ATOM', 'HETATM'))][0]
    heavy = next(i for i in range(n) if pc0.element[i] not in ('H', 'D') and pc0.res_name[pc0.res_id[i]] != 'HOH')
    p = tmp_path / 'missing.cif'
    p.write_text('\n'.join(ln for k, ln in enumerate(lines) if k != head + n + heavy) + '\n')
    with pytest.raises(ValueError, match='model 2 '):
        protein_reader.read_mmcif_models(str(p))
    # model 3: one residue of a polypeptide moved by 3 A -> its peptide link breaks
    good = tmp_path / 'good.cif'
    good.write_text(text)
    linked = protein_reader.read_mmcif(str(good))
    r = int(np.nonzero(linked.res_next >= 0)[0][0])
    bad = xyz.copy()
    bad[2, pc0.res_id == r] += np.array([3.0, 0.0, 0.0], np.float32)
    q = tmp_path / 'moved.cif'
    q.write_text(_cif_models(pc0, bad))
    with pytest.raises(ValueError, match='model 3 ') as ei:
        protein_reader.read_mmcif_models(str(q))
    assert 'differs' in str(ei.value)


def _merged(singles, counts):
    """Per-model bags (model-local ids) shifted and concatenated in canonical order: what one pass over the models returns."""
    key = {'atom_atom': ('i', 'j'), 'atom_plane': ('ring', 'atom'), 'plane_plane': ('bgn', 'end'), 'group_group': ('bgn', 'end'),
           'group_plane': ('amide', 'ring')}
    out = {}
    for name, (k1, k2) in key.items():
        parts = []
        for f, s in enumerate(singles):
            d = {c: v.copy() for c, v in s[name].items()}
            for c, what in _capi._MODEL_SPLIT[name][1].items():
                d[c] = (d[c] + f * counts[what]).astype(np.int32)
            parts.append(d)
        m = {c: np.concatenate([p[c] for p in parts]) for c in parts[0]}
        o = np.lexsort((m[k2], m[k1]))
        out[name] = {c: v[o] for c, v in m.items()}
    return out


def test_contiguous_split_equals_the_batch_split():
    rs = np.random.RandomState(7)
    counts = dict(n=50, nring=6, namide=9, F=5)
    singles = []
    for f in range(counts['F']):
        k = rs.randint(0, 40)
        aa = dict(i=rs.randint(0, 50, k).astype(np.int32), j=rs.randint(0, 50, k).astype(np.int32), dist=rs.rand(k).astype(np.float32),
                  sift=rs.randint(0, 1 << 15, k).astype(np.uint16), ctype=rs.randint(0, 4, k).astype(np.uint8))
        ap = dict(atom=rs.randint(0, 50, k).astype(np.int32), ring=rs.randint(0, 6, k).astype(np.int32), dist=rs.rand(k))
        pp = dict(bgn=rs.randint(0, 6, k).astype(np.int32), end=rs.randint(0, 6, k).astype(np.int32), dist=rs.rand(k))
        gg = dict(bgn=rs.randint(0, 9, k).astype(np.int32), end=rs.randint(0, 9, k).astype(np.int32), dist=rs.rand(k).astype(np.float32))
        gp = dict(amide=rs.randint(0, 9, k).astype(np.int32), ring=rs.randint(0, 6, k).astype(np.int32), dist=rs.rand(k))
        singles.append(dict(atom_atom=aa, atom_plane=ap, plane_plane=pp, group_group=gg, group_plane=gp))
    singles[2] = {name: {c: v[:0] for c, v in b.items()} for name, b in singles[2].items()}       # a model without records
    bags = _merged(singles, counts)
    got = _capi.split_models(bags, counts)
    off = dict(atom=np.arange(6) * 50, ring=np.arange(6) * 6, amide=np.arange(6) * 9)
    want_aa = batch.split_atom_contacts(bags['atom_atom'], off)
    for f in range(counts['F']):
        for c in want_aa[f]:
            assert np.array_equal(got[f]['atom_atom'][c], want_aa[f][c]), (f, c)
        for name in BAGS[1:]:
            w = batch.split_bag(name, bags[name], off)[f]
            assert set(w) == set(got[f][name])
            for c in w:
                assert np.array_equal(got[f][name][c], w[c]), (f, name, c)
    # the ROWS layout: row offsets instead of the first column
    aa = bags['atom_atom']
    row = np.searchsorted(aa['i'], np.arange(counts['F'] * 50 + 1)).astype(np.int32)
    rows = dict(bags, atom_atom=_capi.RowsBag(row=row, **{c: v for c, v in aa.items() if c != 'i'}))
    got_r = _capi.split_models(rows, counts)
    for f in range(counts['F']):
        for c in want_aa[f]:
            assert np.array_equal(got_r[f]['atom_atom'][c], want_aa[f][c]), (f, c)


# ------------------------------------------------------------------------------------------------------------- GPU
def _same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape)
        if x.dtype.kind == 'f':
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)
        else:
            assert np.array_equal(x, y), (what, k)


def _single_ic(pc, xyz_k, h_k, ctx):
    """The single-structure path for one model: InteractionComplex on the model's pack with its plane geometry pending."""
    from arpeggio_amd.core import InteractionComplex
    q = copy.copy(pc)
    q.xyz, q.h_xyz = np.ascontiguousarray(xyz_k), np.ascontiguousarray(h_k)
    q.plane_geometry_pending = True
    ic = InteractionComplex(q, 0.1, 5.0, 7.4)
    ic._ctx = ctx            # (one GPU context for every single run)
    ic.initialize()
    return ic


def _selectors(pc):
    lig = 'HEM' if 'HEM' in pc.res_name else 'BNZ'
    r = pc.n_residues // 3
    return ([], ['/%s/%d/' % (pc.res_chain[r], int(pc.res_seq[r]))], ['RESNAME:' + lig])


def _compare_model(ens, k, ic, what):
    m = ens.model(k)
    for name in BAGS:
        _same(m._bags[name], ic._bags[name], (what, k, name))
    assert np.array_equal(np.asarray(m.selection_plus), np.asarray(ic.selection_plus)), (what, k)
    assert np.array_equal(m.selection_plus_residues, ic.selection_plus_residues), (what, k)
    for attr in ('selection_ring_ids', 'selection_plus_ring_ids', 'selection_amide_ids', 'selection_plus_amide_ids'):
        assert getattr(m, attr) == getattr(ic, attr), (what, k, attr)


def _planes_equal(ens, k, ic, what):
    p = ens.planes
    for key, arr in (('ring_center', ic.pc.ring_center), ('ring_normal', ic.pc.ring_normal), ('ring_res', ic.pc.ring_res),
                     ('amide_center', ic.pc.amide_center), ('amide_normal', ic.pc.amide_normal)):
        _same({key: p[key][k]}, {key: np.asarray(arr)}, (what, k))


CASES = [('proteinlike120', lambda: synth.proteinlike(n_res=120, seed=11, n_waters=60), 20, 0.3),
         ('synthetic3000', lambda: synth.make_synthetic(3000, seed=5, box=(45, 45, 45), n_rings=30, n_amides=40), 8, 0.3),
         ('one_model', lambda: synth.proteinlike(n_res=60, seed=12, n_waters=20), 1, 0.0),
         ('proteinlike40', lambda: synth.proteinlike(n_res=40, seed=21, n_waters=20), 64, 0.3)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,make,F,jitter', CASES, ids=[c[0] for c in CASES])
def test_every_model_equals_its_single_run(name, make, F, jitter):
    """Per-model parity: all five bags, the selection sets, ring / amide geometry and ring residues of every model against the
    single-structure path for that model, for three parameter sets and three selections; the oracle for one parameter set."""
    import oracle
    from arpeggio_amd.core import EnsembleComplex
    pc = make()
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=jitter)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    assert ens.n_models == F
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(True)
    singles = [_single_ic(pc, xyz[k], h_xyz[k], ctx) for k in range(F)]
    for k in range(F):
        _planes_equal(ens, k, singles[k], name)
    n_rec = 0
    for params in ((5.0, 0.1, False), (4.0, 0.25, True), (7.5, 0.1, False)):
        for sel in _selectors(pc):
            ens.run_arpeggio(sel, *params)
            for k in range(F):
                ctx.set_complex(singles[k].pc)      # (the shared context holds the structure uploaded last)
                singles[k].run_arpeggio(sel, *params)
                _compare_model(ens, k, singles[k], (name, params, tuple(sel)))
                n_rec += len(singles[k]._bags['atom_atom']['i'])
            if params == (5.0, 0.1, False) and not sel:
                for k in range(F):
                    oc = oracle.OracleComplex(singles[k].pc)
                    oc.make_selection(None)
                    want = oc.atom_contacts(5.0, 0.1, False)
                    got = ens.model(k)._bags['atom_atom']
                    for c in ('i', 'j', 'sift', 'ctype'):
                        assert np.array_equal(got[c], want[c]), (name, k, c)
                    for bag, cols in (('atom_plane', ('atom', 'ring')), ('plane_plane', ('bgn', 'end')), ('group_group', ('bgn', 'end')),
                                      ('group_plane', ('amide', 'ring'))):
                        w = getattr(oc, bag)()
                        o = np.lexsort((w[cols[1]], w[cols[0]])) if bag != 'atom_plane' else np.lexsort((w['atom'], w['ring']))
                        for c in cols:
                            assert np.array_equal(ens.model(k)._bags[bag][c], np.asarray(w[c])[o]), (name, k, bag, c)
    assert n_rec > 0
    ctx.close()


@pytest.mark.gpu
def test_ring_residue_is_per_model():
    """An atom of another residue within 1.0 A of a ring centre in ONE model: that model's ring residue changes, and equals
    its single run's; the other models keep theirs."""
    from arpeggio_amd.core import EnsembleComplex
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    xyz, h_xyz = synth.models_of(pc, 3, seed=2)
    ctx = _capi.Context(0)
    r = 0
    ring_res0 = _single_ic(pc, xyz[0], h_xyz[0], ctx).pc.ring_res[r]
    centre = xyz[1][pc.ring_atoms[r]].astype(np.float64).mean(axis=0)
    other = next(i for i in range(pc.n_atoms) if pc.res_id[i] != ring_res0 and pc.res_name[pc.res_id[i]] == 'HOH')
    xyz[1, other] = (centre + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    single1 = _single_ic(pc, xyz[1], h_xyz[1], ctx)
    assert ens.planes['ring_res'][1][r] == single1.pc.ring_res[r] == pc.res_id[other] != ens.planes['ring_res'][0][r]
    assert ens.planes['ring_res'][0][r] == ring_res0
    for k in range(3):
        _planes_equal(ens, k, _single_ic(pc, xyz[k], h_xyz[k], ctx), 'ring residue')
    ctx.close()


@pytest.mark.gpu
def test_coordinate_chunks_and_bad_input():
    """set_coordinates twice with another F gives what a fresh object gives; between a coordinate change and the next launch
    the fetches refuse; a NaN in model 3 is refused and leaves the topology usable; a shard context and a context without a
    topology are refused."""
    from arpeggio_amd.core import EnsembleComplex
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    xyz, h_xyz = synth.models_of(pc, 12, seed=6, jitter=0.2)
    ens = EnsembleComplex((copy.copy(pc), xyz[:5], h_xyz[:5]))
    ens.run_arpeggio([], 5.0, 0.1, False)
    for lo, hi in ((5, 12), (2, 4)):
        ens.set_coordinates(xyz[lo:hi], h_xyz[lo:hi])
        with pytest.raises(ValueError):            # results of the previous models are void
            ens._ctx.fetch_packed()
        ens.run_arpeggio([], 5.0, 0.1, False)
        fresh = EnsembleComplex((copy.copy(pc), xyz[lo:hi], h_xyz[lo:hi]))
        fresh.run_arpeggio([], 5.0, 0.1, False)
        assert ens.n_models == hi - lo
        for k in range(hi - lo):
            for name in BAGS:
                _same(ens.model(k)._bags[name], fresh.model(k)._bags[name], (lo, k, name))
    # a NaN in model 3: ARP_E_ARG, nothing resident; then a valid call on the kept topology
    ctx = ens._ctx
    bad = xyz[:5].copy()
    bad[3, 7, 1] = np.nan
    with pytest.raises(ValueError, match='arp_set_models'):
        ctx.set_models(bad, h_xyz[:5])
    with pytest.raises(ValueError):
        ctx.models_planes()
    with pytest.raises(ValueError):
        ctx.run_launch()
    ctx.set_models(xyz[:5], h_xyz[:5])
    per = ctx.run_models(5.0, 0.1, False)
    ref = EnsembleComplex((copy.copy(pc), xyz[:5], h_xyz[:5]))
    ref.run_arpeggio([], 5.0, 0.1, False)
    for k in range(5):
        _same(per[k]['atom_atom'], ref.model(k)._bags['atom_atom'], ('after NaN', k))
    # no topology
    c2 = _capi.Context(0)
    c2._topology = dict(n=pc.n_atoms, nres=pc.n_residues, nring=pc.n_rings, namide=pc.n_amides, nh=int(pc.h_xyz.shape[0]))
    with pytest.raises(ValueError, match='no topology'):
        c2.set_models(xyz[:2], h_xyz[:2])
    # a shard (ownership declared)
    c2.set_complex(pc)
    c2.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    with pytest.raises(ValueError, match='shard'):
        c2.set_topology(pc)
    c2.close()


@pytest.mark.gpu
def test_two_model_reader_file_equals_the_executed_reference_and_its_single_run(tmp_path, golden_dir):
    """The reader fixture's file with its _atom_site rows repeated as model 2, waters moved rigidly: model 1 equals the executed
    reference's records, model 2 equals InteractionComplex on a one-model file of model 2, and get_contacts gives the same
    JSON text as the single runs."""
    from arpeggio_amd.core import EnsembleComplex, InteractionComplex
    from test_golden_core import check_planes
    z = np.load(os.path.join(golden_dir, 'core_cases.npz'), allow_pickle=False)
    text = str(z['reader/cif_text'])
    cat = _capi.CifCategory(text, '_atom_site.')
    tags = cat.tags
    cols = cat.columns()
    cat.close()
    lines = text.splitlines()
    first = next(k for k, ln in enumerate(lines) if ln.startswith(('ATOM', 'HETATM')))
    nrow = len(cols['id'])
    rows = lines[first:first + nrow]
    assert all(ln.startswith(('ATOM', 'HETATM')) for ln in rows)
    def cell(v):           # a value as CIF text: '?' / '.' for None / False, quoted when it holds a space or begins with a quote
        if v is None:
            return '?'
        if v is False:
            return '.'
        if v == '' or any(ch.isspace() for ch in v) or v[0] in '\'"_#$;[]':
            return '"%s"' % v if "'" in v else "'%s'" % v
        return v
    shift = {}
    rows2 = []
    for k in range(nrow):
        f = [cols[t][k] for t in tags]
        f[tags.index('id')] = str(int(f[tags.index('id')]) + 100000)
        f[tags.index('pdbx_PDB_model_num')] = str(int(f[tags.index('pdbx_PDB_model_num')]) + 1)
        if cols['label_comp_id'][k] in ('HOH', 'DOD'):
            d = shift.setdefault(cols['auth_seq_id'][k], np.array([0.7, -0.4, 0.5]) * (1 + len(shift) % 3))
            for a, t in enumerate(('Cartn_x', 'Cartn_y', 'Cartn_z')):
                f[tags.index(t)] = '%.3f' % (float(f[tags.index(t)]) + d[a])
        rows2.append(' '.join(cell(v) for v in f))
    assert shift
    two = lines[:first + nrow] + rows2 + lines[first + nrow:]
    p = tmp_path / 'reader_two.cif'
    p.write_text('\n'.join(two) + '\n')
    m2 = tmp_path / 'reader_model2.cif'
    m2.write_text('\n'.join(lines[:first] + rows2 + lines[first + nrow:]) + '\n')
    ens = EnsembleComplex(str(p), 0.1, 5.0, 7.4, allow_incomplete=True)
    assert ens.n_models == 2
    ens.structure_checks()
    ens.initialize()
    for case, selectors in (('reader:whole', []), ('reader:chain_b', ['/B//'])):
        ens.run_arpeggio(selectors, 5.0, 0.1, False)
        m = ens.model(0)
        got = m._bags['atom_atom']
        b, e = z[case + '/aa_bgn'], z[case + '/aa_end']
        o = np.lexsort((e, b))
        assert np.array_equal(got['i'], b[o]) and np.array_equal(got['j'], e[o]), case
        assert np.array_equal(got['dist'].view(np.uint32), z[case + '/aa_dist'][o].view(np.uint32)), case
        assert np.array_equal(got['sift'], z[case + '/aa_sift'][o]) and np.array_equal(got['ctype'], z[case + '/aa_ctype'][o]), case
        assert np.array_equal(np.sort(m.selection_plus), np.sort(z[case + '/selection_plus'])), case
        b4 = m._bags
        check_planes(z, case, b4['atom_plane'], b4['plane_plane'], b4['group_group'], b4['group_plane'])
        for attr in ('selection_ring_ids', 'selection_plus_ring_ids', 'selection_amide_ids', 'selection_plus_amide_ids'):
            assert sorted(getattr(m, attr)) == z[f'{case}/{attr}'].tolist(), (case, attr)
        assert np.array_equal(m.selection_plus_residues, z[case + '/selection_plus_residues']), case
        # model 2 against a one-model file of model 2 through InteractionComplex; JSON text of both models against single runs
        for k, path in ((1, m2), (0, tmp_path / 'reader_model1.cif')):
            if k == 0:
                path.write_text('\n'.join(lines) + '\n')
            ic = InteractionComplex(str(path), 0.1, 5.0, 7.4, allow_incomplete=True)
            ic.initialize()
            ic.run_arpeggio(selectors, 5.0, 0.1, False)
            _compare_model(ens, k, ic, (case, k))
            assert json.dumps(ens.model(k).get_contacts(), sort_keys=True) == json.dumps(ic.get_contacts(), sort_keys=True), (case, k)
            assert len(ic.get_contacts()) > 0
