"""HIP path vs the oracle through the C ABI.  Needs a real MI355X: `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest

from helpers import assert_planes_equal as _assert_planes_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def capi():
    from arpeggio_amd import _capi
    return _capi


@pytest.fixture(scope='module')
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def _assert_contacts_equal(got, exp):
    assert len(got['i']) == len(exp['i'])
    for k in ('i', 'j', 'sift', 'ctype'):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got['dist'].view(np.uint32), exp['dist'].view(np.uint32)), 'distance not bit-identical'


@pytest.mark.parametrize('n,seed', [(3000, 1), (20000, 3)])
def test_search_all_equals_brute_force(ctx, n, seed):
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(n, seed=seed)
    ctx.set_complex(pc)
    for radius in (5.0, 6.0, 2.5):
        gi, gj = ctx.search_all(radius)
        ei, ej, _ = oracle.search_all(pc.xyz, radius, grid=(n > 5000))
        assert np.array_equal(gi, ei) and np.array_equal(gj, ej), radius
    act = (np.arange(pc.n_atoms) % 3 != 0).astype(np.uint8)
    gi, gj = ctx.search_all(5.0, active=act)
    ei, ej, _ = oracle.search_all(pc.xyz, 5.0, active=act)
    assert np.array_equal(gi, ei) and np.array_equal(gj, ej)


def test_search_all_adversarial_points(ctx):
    """Points on cell faces, duplicates, pairs exactly at the radius, empty cells."""
    import oracle
    from helpers import tiny_complex
    g = np.arange(0, 31, 5, dtype=np.float32)
    pts = np.array([[x, y, z] for x in g for y in g[:3] for z in g[:2]], np.float32)   # lattice with spacing == radius
    pts = np.concatenate([pts, pts[:10], pts[:5] + np.float32(1e-6), [[100, 100, 100]], [[3, 4, 0]], [[0, 0, 0]]]).astype(np.float32)
    pc = tiny_complex(pts)
    ctx.set_complex(pc)
    for radius in (5.0, 4.999999, 7.0710678, 0.5):
        gi, gj = ctx.search_all(radius)
        ei, ej, _ = oracle.search_all(pc.xyz, radius, grid=False)
        assert np.array_equal(gi, ei) and np.array_equal(gj, ej), radius
        assert len(gi) > 0


@pytest.mark.parametrize('n,seed,seq_adj,comp', [(4000, 2, False, 0.1), (20000, 3, False, 0.1), (20000, 5, True, 0.25)])
def test_atom_contacts_whole_structure(ctx, n, seed, seq_adj, comp):
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(n, seed=seed)
    ctx.set_complex(pc)
    ctx.make_selection(None)
    got = ctx.atom_contacts(5.0, comp, seq_adj)
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None)
    exp = oc.atom_contacts(5.0, comp, seq_adj)
    _assert_contacts_equal(got, exp)
    assert got['stats']['accepted'] == exp['stats'][1]
    assert got['stats']['candidates'] == exp['stats'][0]
    # every flag is exercised by the synthetic set
    for b in range(15):
        assert ((exp['sift'] >> b) & 1).any(), b


def test_selection_and_all_contact_bags(ctx):
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(20000, seed=9)
    ctx.set_complex(pc)
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[(pc.res_id % 17) == 0] = 1
    masks = ctx.make_selection(sel)
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel, use_grid=True)
    assert np.array_equal(masks['plus'], plus)
    assert 0 < plus.sum() < pc.n_atoms
    assert np.array_equal(masks['ring_sel'], oc.ring_sel) and np.array_equal(masks['ring_plus'], oc.ring_plus)
    assert np.array_equal(masks['amide_sel'], oc.amide_sel) and np.array_equal(masks['amide_plus'], oc.amide_plus)
    got, exp = ctx.atom_contacts(), oc.atom_contacts()
    _assert_contacts_equal(got, exp)
    assert len(np.unique(exp['ctype'])) >= 5
    _assert_planes_equal(ctx.atom_plane(), oc.atom_plane(), ('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',))
    epp = oc.plane_plane()
    o = np.lexsort((epp['end'], epp['bgn']))
    epp = {k: v[o] for k, v in epp.items()}
    _assert_planes_equal(ctx.plane_plane(), epp, ('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end'))
    _assert_planes_equal(ctx.group_group(), oc.group_group(), ('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta'), tol=1e-4)
    _assert_planes_equal(ctx.group_plane(), oc.group_plane(), ('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta'))


def test_rings_config5_subset(ctx):
    """BASELINE configs[4] family at a size the oracle's O(R^2) loops finish quickly."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config5(n_rings=3000, n_amides=3000, seed=5, L=60.0)
    ctx.set_complex(pc)
    ctx.make_selection(None)
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None)
    epp = oc.plane_plane()
    o = np.lexsort((epp['end'], epp['bgn']))
    epp = {k: v[o] for k, v in epp.items()}
    gpp = ctx.plane_plane()
    assert len(gpp['bgn']) > 3000
    _assert_planes_equal(gpp, epp, ('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end'))
    _assert_planes_equal(ctx.group_group(), oc.group_group(), ('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta'), tol=1e-4)
    _assert_planes_equal(ctx.group_plane(), oc.group_plane(), ('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta'))
    _assert_planes_equal(ctx.atom_plane(), oc.atom_plane(), ('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',))


def test_golden_plane_fixtures_on_gpu(ctx, golden_dir):
    """The HIP plane kernels against records produced by the reference's own loops."""
    from arpeggio_amd.core import config
    from helpers import planes_only_complex
    g = np.load(os.path.join(golden_dir, 'planes_input.npz'))
    exp = json.load(open(os.path.join(golden_dir, 'planes_expected.json')))
    pc = planes_only_complex(g['ring_center'], g['ring_normal'], g['ring_res'], g['amide_center'], g['amide_normal'],
                             g['amide_res'], g['nres'])
    # reproduce the fixture's selection masks through residue membership: give every residue one atom
    nres = int(g['nres'])
    from helpers import tiny_complex
    xyz = np.zeros((nres, 3), np.float32)
    xyz[:, 0] = 1000.0 + 50.0 * np.arange(nres)        # far apart: the 6 A expansion adds nothing
    pc2 = tiny_complex(xyz, res_id=np.arange(nres), rings=(g['ring_center'], g['ring_normal'], g['ring_res']),
                       amides=(g['amide_center'], g['amide_normal'], g['amide_res']))
    # selection_plus == res_plus cannot be imposed directly (it is derived), so check with selection = plus set
    res_plus = np.zeros(nres, np.uint8)
    res_plus[g['ring_res'][g['ring_plus'] == 1]] = 1
    res_plus[g['amide_res'][g['amide_plus'] == 1]] = 1
    ctx.set_complex(pc2)
    masks = ctx.make_selection(res_plus)
    assert np.array_equal(masks['ring_plus'], g['ring_plus']) and np.array_equal(masks['amide_plus'], g['amide_plus'])
    got = ctx.plane_plane()
    e = exp['plane_plane']
    assert len(got['bgn']) == len(e)
    key = {(r['bgn_id'], r['end_id']): r for r in e}
    for k in range(len(e)):
        rec = key[(int(got['bgn'][k]), int(got['end'][k]))]
        assert got['dist'][k] == rec['distance']
        types = [config.PLANE_PLANE_NAMES[got['type1'][k]]]
        if got['type2'][k] < config.PP_SAME:
            types.append(config.PLANE_PLANE_NAMES[got['type2'][k]])
        assert types == rec['contact_type']
    gg = ctx.group_group()
    assert [(int(a), int(b)) for a, b in zip(gg['bgn'], gg['end'])] == [(r['bgn_id'], r['end_id']) for r in exp['group_group']]
    assert all(gg['dist'][k] == np.float32(r['distance']) for k, r in enumerate(exp['group_group']))
    gp = ctx.group_plane()
    assert [(int(a), int(b)) for a, b in zip(gp['amide'], gp['ring'])] == [(r['bgn_id'], r['end_id']) for r in exp['group_plane']]
    assert all(gp['dist'][k] == r['distance'] for k, r in enumerate(exp['group_plane']))


def test_full_size_config3_properties(ctx):
    """BASELINE configs[2] at full size: parity with the (grid) oracle plus size-independent properties."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(100_000, seed=3)
    ctx.set_complex(pc)
    ctx.make_selection(None)
    got = ctx.atom_contacts()
    # properties: canonical orientation, no duplicates, exclusive ladder, idempotence
    assert np.all(got['i'] < got['j'])
    key = got['i'].astype(np.int64) * pc.n_atoms + got['j']
    assert len(np.unique(key)) == len(key)
    ladder = got['sift'] & 0x1F
    assert np.all((ladder & (ladder - 1)) == 0) and np.all(ladder != 0)
    again = ctx.atom_contacts()
    _assert_contacts_equal(again, got)
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None)
    _assert_contacts_equal(got, oc.atom_contacts())
    from helpers import boundary_sensitive_pairs, report_boundary_pairs
    report_boundary_pairs('config3_100k_atoms', boundary_sensitive_pairs(pc, got))


def test_run_launch_single_sync_path(ctx):
    """arp_run_launch (everything enqueued back to back, one sync) == the stage-by-stage calls == oracle."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(20000, seed=13)
    ctx.set_complex(pc)
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[(pc.res_id % 11) == 3] = 1
    ctx.set_selection(sel)
    counts = ctx.run_launch(5.0, 0.1, False, 6.0)
    got = ctx.atom_contacts_fetch(counts['atom_atom'])
    oc = oracle.OracleComplex(pc)
    oc.make_selection(sel)
    exp = oc.atom_contacts()
    _assert_contacts_equal(got, exp)
    epp = oc.plane_plane()
    o = np.lexsort((epp['end'], epp['bgn']))
    epp = {k: v[o] for k, v in epp.items()}
    _assert_planes_equal(ctx.fetch_bag('plane_plane'), epp, ('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end'))
    _assert_planes_equal(ctx.fetch_bag('atom_plane'), oc.atom_plane(), ('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',))
    _assert_planes_equal(ctx.fetch_bag('group_group'), oc.group_group(), ('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta'), tol=1e-4)
    _assert_planes_equal(ctx.fetch_bag('group_plane'), oc.group_plane(), ('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta'))
    assert counts['plane_plane'] == len(epp['bgn'])
    # a second run on the same context (buffers already sized) gives the same answer
    for _ in range(3):
        counts2 = ctx.run_launch(5.0, 0.1, False, 6.0)
        assert counts2 == counts
        _assert_contacts_equal(ctx.atom_contacts_fetch(counts2['atom_atom']), exp)
    # a new selection re-uses the captured graph (same buffers, new mask contents)
    sel2 = np.zeros(pc.n_atoms, np.uint8)
    sel2[(pc.res_id % 7) == 1] = 1
    ctx.set_selection(sel2)
    c3 = ctx.run_launch(5.0, 0.1, False, 6.0)
    oc.make_selection(sel2)
    _assert_contacts_equal(ctx.atom_contacts_fetch(c3['atom_atom']), oc.atom_contacts())
    _assert_planes_equal(ctx.fetch_bag('atom_plane'), oc.atom_plane(), ('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',))
    # different parameters invalidate it
    c4 = ctx.run_launch(4.0, 0.2, True, 6.0)
    _assert_contacts_equal(ctx.atom_contacts_fetch(c4['atom_atom']), oc.atom_contacts(4.0, 0.2, True))


def test_known_answer_packs_on_gpu(ctx):
    """Every branch / quirk pack (tests/helpers.known_answer_packs): HIP == oracle, canonical orientation."""
    import oracle
    from helpers import known_answer_packs
    packs = known_answer_packs()
    assert len(packs) > 50
    for name, pc in packs:
        ctx.set_complex(pc)
        ctx.make_selection(None)
        oc = oracle.OracleComplex(pc)
        oc.make_selection(None)
        exp = oc.atom_contacts(5.0, 0.1, False, use_grid=False)
        if exp['err'] == -4:
            with pytest.raises(AttributeError):
                ctx.atom_contacts(5.0, 0.1, False)
            continue
        got = ctx.atom_contacts(5.0, 0.1, False)
        assert len(got['i']) == len(exp['i']), name
        for k in ('i', 'j', 'sift', 'ctype'):
            assert np.array_equal(got[k], exp[k]), (name, k, got[k], exp[k])
        assert np.array_equal(got['dist'].view(np.uint32), exp['dist'].view(np.uint32)), name


@pytest.mark.parametrize('seed', [1, 2, 3, 4, 5, 6])
def test_random_dense_soup(ctx, seed):
    """Dense random packs with every type/flag combination, partial selections and both filter settings."""
    import oracle
    from helpers import random_dense_pack
    pc = random_dense_pack(seed)
    rng = np.random.default_rng(seed)
    sel = (rng.random(pc.n_atoms) < 0.3).astype(np.uint8)
    sel[0] = 1
    ctx.set_complex(pc)
    masks = ctx.make_selection(sel)
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel, use_grid=False)
    assert np.array_equal(masks['plus'], plus)
    for seq_adj, comp in ((False, 0.1), (True, 0.0), (False, 0.37)):
        got = ctx.atom_contacts(5.0, comp, seq_adj)
        exp = oc.atom_contacts(5.0, comp, seq_adj, use_grid=False)
        assert exp['err'] == 0
        _assert_contacts_equal(got, exp)
    assert len(np.unique(exp['ctype'])) == 6


def test_interaction_complex_drop_in(ctx):
    """The reference's call sequence (process_protein_cli.py:159-182) on the mirror class; JSON schema of README.md:127-241."""
    import oracle
    from arpeggio_amd import synth
    from arpeggio_amd.core import InteractionComplex, config
    pc = synth.config3(8000, seed=21)
    ic = InteractionComplex(pc, 0.1, 5.0, 7.4)
    ic.structure_checks()
    ic.initialize()
    ic.run_arpeggio(['/A/5/', '/A/6/', 'RESNAME:BNZ'], 5.0, 0.1, False)
    contacts = ic.get_contacts()
    s = json.dumps(contacts, indent=4, sort_keys=True)
    assert json.loads(s) == contacts
    types = [c['type'] for c in contacts]
    order = ['atom-atom', 'plane-plane', 'atom-plane', 'group-group', 'group-plane']
    assert [t for t in order if t in types] == sorted(set(types), key=order.index)
    assert types == sorted(types, key=order.index)          # bags in the reference's order (I:183-210)
    for c in contacts:
        assert set(c) == {'bgn', 'end', 'type', 'distance', 'contact', 'interacting_entities'}
        assert set(c['bgn']) == {'label_comp_id', 'auth_seq_id', 'auth_asym_id', 'auth_atom_id', 'pdbx_PDB_ins_code', 'label_comp_type'}
        assert set(c['end']) == set(c['bgn'])
        assert isinstance(c['distance'], float) and round(c['distance'], 2) == c['distance']
        assert isinstance(c['contact'], list) and c['interacting_entities'] in config.CONTACT_TYPE_NAMES
    aa = [c for c in contacts if c['type'] == 'atom-atom']
    assert all(set(c['contact']) <= set(config.SIFT_NAMES) for c in aa)
    # same selection through the oracle
    from arpeggio_amd.core import utils
    idx = utils.selection_parser(['/A/5/', '/A/6/', 'RESNAME:BNZ'], pc)
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[idx] = 1
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel)
    exp = oc.atom_contacts()
    assert len(aa) == len(exp['i'])
    assert np.array_equal(ic.selection_plus, np.nonzero(plus)[0])
    assert ic.selection_plus_ring_ids == set(np.nonzero(oc.ring_plus)[0].tolist())
    first = ic.atom_contacts[0]
    assert (first.bgn_atom, first.end_atom) == (int(exp['i'][0]), int(exp['j'][0]))
    assert first.sifts == [(int(exp['sift'][0]) >> k) & 1 for k in range(15)]
    from arpeggio_amd.core import SelectionError
    with pytest.raises(SelectionError):
        ic.run_arpeggio(['/A/999999/'], 5.0, 0.1, False)


def test_initialize_geometry_rings_amides_and_ring_residues(ctx):
    """ring centre / normal (I:1697-1733), amide centre / normal (I:1531-1589) and the ring ->
    residue assignment (I:1453-1492) on the GPU against the NumPy restatement (oracle/ref_py.py)."""
    from oracle import ref_py
    from arpeggio_amd import synth
    pc = synth.proteinlike(n_res=200, seed=6, n_waters=80)
    ctx.set_complex(pc)
    assert pc.n_rings > 10 and pc.n_amides > 100
    rings = [np.asarray(a, np.int32) for a in pc.ring_atoms]
    ctr, nrm = ctx.ring_geometry(rings)
    ectr, enrm = ref_py.ring_geometry(pc.xyz, rings)
    assert np.array_equal(ctr, ectr)                                        # bit-identical float64
    assert np.array_equal(nrm, enrm)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
    # the generator's own centres are the same points (it averages the same atoms)
    assert np.allclose(ctr, pc.ring_center, atol=1e-5)
    res, dist = ctx.ring_residues(ctr)
    eres, edist = ref_py.ring_residues(pc.xyz, pc.res_id, ctr)
    assert np.array_equal(res, eres) and np.array_equal(dist, edist)
    assert (res >= 0).all() and (res == pc.ring_res).mean() > 0.8     # (the generator assigns rings by construction, not by distance)
    far = ctr + 500.0                                                       # nothing within 3 A
    res2, dist2 = ctx.ring_residues(far)
    assert (res2 == -1).all() and (dist2 == -1.0).all()
    # amides: centre bit-identical (float32 mean of C and N); normal = the SVD's plane normal up to sign and ~1e-6
    am = pc.amide_atoms
    actr, anrm = ctx.amide_geometry(am)
    ectr, enrm = ref_py.amide_geometry(pc.xyz, am)
    assert np.array_equal(actr, ectr)
    sign = np.sign(np.sum(anrm * enrm, axis=1, keepdims=True))
    assert np.abs(anrm * sign - enrm).max() < 5e-6
    # through the mirror class: a pack whose ring / amide geometry is blank gets it from the GPU, results unchanged
    from arpeggio_amd.core import InteractionComplex
    import copy
    blank = copy.deepcopy(pc)
    blank.ring_center[:] = 0
    blank.ring_normal[:] = 0
    blank.amide_center[:] = 0
    blank.amide_normal[:] = 0
    ic = InteractionComplex(blank, 0.1, 5.0, 7.4)
    ic.initialize()
    ic.compute_plane_geometry(assign_ring_residues=False)
    assert np.array_equal(blank.ring_center, ctr) and np.array_equal(blank.amide_center, actr)
    ic.run_arpeggio([], 5.0, 0.1, False)
    ref_ic = InteractionComplex(pc, 0.1, 5.0, 7.4)
    ref_ic.initialize()
    ref_ic.run_arpeggio([], 5.0, 0.1, False)
    for bag in ('atom_plane', 'plane_plane', 'group_group', 'group_plane'):
        a, b = ic._bags[bag], ref_ic._bags[bag]
        assert len(a['dist']) == len(b['dist']) and np.allclose(a['dist'], b['dist'], atol=1e-5), bag
    assert len(ic._bags['atom_plane']['dist']) > 0 and len(ic._bags['group_group']['dist']) > 0
    # degenerate ring (all atoms on one point): the normal stays (0, 0, 0) as vector3::normalize leaves it
    c0, n0 = ctx.ring_geometry([np.array([5, 5, 5], np.int32)])
    assert np.array_equal(n0, np.zeros((1, 3))) and np.allclose(c0[0], pc.xyz[5], atol=1e-6)
    with pytest.raises(Exception):
        ctx.ring_geometry([np.array([0, 1], np.int32)])                     # fewer than three atoms
    with pytest.raises(Exception):
        ctx.ring_geometry([np.array([0, 1, pc.n_atoms], np.int32)])         # index out of range


def test_atom_and_residue_sifts_and_csv(tmp_path):
    """per-atom sifts (I:923-934), their per-residue flattening (I:471-560) and write_atom_sifts
    (I:349-366) through the mirror class, against the oracle's accumulators."""
    import csv
    import oracle
    from arpeggio_amd import synth
    from arpeggio_amd.core import InteractionComplex, config, utils
    pc = synth.proteinlike(n_res=120, seed=4, n_waters=60, id='plike')
    ic = InteractionComplex(pc, 0.1, 5.0, 7.4)
    ic.structure_checks()
    ic.initialize()
    ic.run_arpeggio(['/A/30/', '/A/31/', '/A/64/'], 5.0, 0.1, False)
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[utils.selection_parser(['/A/30/', '/A/31/', '/A/64/'], pc)] = 1
    oc = oracle.OracleComplex(pc)
    oc.make_selection(sel)
    exp = oracle.atom_accumulators(pc.n_atoms, oc.atom_contacts())
    got = ic.atom_sifts()
    names = ('sift', 'sift_inter_only', 'sift_intra_only', 'sift_water_only')
    for k, n in enumerate(names):
        bits = ((exp['sift'][:, k, None] >> np.arange(15)[None, :]) & 1).astype(np.uint8)
        assert np.array_equal(got[n], bits), n
    assert np.array_equal(got['counts'], exp['counts'])
    assert got['sift'].any() and got['sift_inter_only'].any() and got['sift_intra_only'].any()
    # residues: OR over the atoms, main chain / side chain split for polypeptide residues
    rs = ic.residue_sifts()
    poly = (pc.res_flags & config.R_POLYPEPTIDE) != 0
    for r in np.unique(pc.res_id[ic.selection_plus])[:40].tolist():
        atoms = np.nonzero(pc.res_id == r)[0]
        assert np.array_equal(rs['sift'][r], got['sift'][atoms].max(0))
        mc = [a for a in atoms if pc.atom_name[a] in config.MAINCHAIN_ATOMS]
        sc = [a for a in atoms if pc.atom_name[a] not in config.MAINCHAIN_ATOMS]
        for pre, sub in (('mc_', mc), ('sc_', sc)):
            want = got['sift_inter_only'][sub].max(0) if (poly[r] and sub) else np.zeros(15, np.uint8)
            assert np.array_equal(rs[pre + 'sift_inter_only'][r], want)
    assert rs['mc_sift'].any() and rs['sc_sift'].any()
    # the two CSV files
    ic.write_atom_sifts(str(tmp_path))
    rows = list(csv.reader(open(tmp_path / 'plike_sifts.csv')))
    assert rows[0] == ['atom'] + list(config.SIFT_NAMES) + ['interacting_entities'] and len(rows) == 1 + len(ic.selection_plus)
    a0 = int(ic.selection_plus[0])
    assert rows[1] == [utils.make_pymol_string(pc, atom=a0)] + [str(int(v)) for v in got['sift'][a0]]
    spec = list(csv.reader(open(tmp_path / 'plike_specific_sifts.csv')))
    assert len(spec) == len(rows) and len(spec[1]) == 46


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_union_on_one_gpu(ctx, capi, world):
    """The ownership / global-id logic of the kernels: shards run one after the other on one GPU,
    the union of what each rank owns == the unsharded result (ids, SIFt, bit-identical distances)."""
    from arpeggio_amd import sharding, synth
    full = synth.slab_config(6000, 3, seed=8)
    rng = np.random.default_rng(5)
    sel = np.zeros(full.n_atoms, np.uint8)
    sel[np.isin(full.res_id, rng.choice(full.n_residues, full.n_residues // 10, replace=False))] = 1
    ctx.set_complex(full)
    gm = ctx.make_selection(sel)
    ref = ctx.atom_contacts()
    ref_bags = {k: getattr(ctx, k)() for k in ('plane_plane', 'atom_plane', 'group_group', 'group_plane')}
    ref_cand = ref['stats']['candidates']
    c2 = capi.Context(0)
    parts, bags, cand = [], {k: [] for k in ref_bags}, 0
    for rank in range(world):
        sh = sharding.make_shard_local(full, rank, world, sel)
        sharding.upload_shard(c2, sh)
        # local expansion is exact for the home atoms
        loc = c2.make_selection(sh.sel)
        hm = sh.is_home == 1
        assert np.array_equal(loc['plus'][hm], gm['plus'][sh.global_id][hm])
        st = sharding.combine_selection(sh, gm['plus'][sh.global_id])     # single process: masks taken from the global run
        assert np.array_equal(st['ring_plus'][sh.ring_home == 1], gm['ring_plus'][sh.ring_gid][sh.ring_home == 1]) or world > 1
        c2.set_selection_state(sel[sh.global_id], gm['plus'][sh.global_id], gm['ring_sel'][sh.ring_gid], gm['ring_plus'][sh.ring_gid],
                               gm['amide_sel'][sh.amide_gid], gm['amide_plus'][sh.amide_gid])
        n = c2.atom_contacts_launch()
        parts.append(c2.atom_contacts_fetch(n))
        cand += c2.stats()['candidates']
        for k in bags:
            c2.launch_bag(k)
            bags[k].append(c2.fetch_bag(k))
    c2.close()
    got = {k: np.concatenate([p[k] for p in parts]) for k in ('i', 'j', 'dist', 'sift', 'ctype')}
    o = np.lexsort((got['j'], got['i']))
    got = {k: v[o] for k, v in got.items()}
    _assert_contacts_equal(got, ref)
    # owned-candidate counting: boundary pairs are not counted twice (the count still depends on how each
    # shard's grid is aligned, so it matches the unsharded count only approximately)
    assert abs(cand - ref_cand) < 0.02 * ref_cand
    order = {'plane_plane': ('bgn', 'end'), 'atom_plane': ('ring', 'atom'), 'group_group': ('bgn', 'end'), 'group_plane': ('amide', 'ring')}
    for k, (k1, k2) in order.items():
        g = {f: np.concatenate([b[f] for b in bags[k]]) for f in ref_bags[k]}
        o = np.lexsort((g[k2], g[k1]))
        for f in ref_bags[k]:
            a, b = g[f][o], ref_bags[k][f]
            assert np.array_equal(a, b) or (a.dtype.kind == 'f' and np.array_equal(np.isnan(a), np.isnan(b))
                                            and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])), (k, f)


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_whole_structure_needs_no_exchange(ctx, capi, world):
    """No selection = whole structure (I:1395): with Context.set_whole_structure every shard runs the plain single-GPU
    pass (one launch sequence, no selection exchange) and the union of what the ranks own == the unsharded result."""
    from arpeggio_amd import sharding, synth
    full = synth.slab_config(6000, 3, seed=8)
    ctx.set_complex(full)
    n_ref = ctx.run_launch()
    ref = ctx.atom_contacts_fetch(n_ref['atom_atom'])
    names = ('plane_plane', 'atom_plane', 'group_group', 'group_plane')
    ref_bags = {k: ctx.fetch_bag(k) for k in names}
    assert n_ref['atom_atom'] > 10_000 and n_ref['plane_plane'] > 0 and n_ref['atom_plane'] > 0
    c2 = capi.Context(0)
    parts, bags = [], {k: [] for k in names}
    for rank in range(world):
        sh = sharding.make_shard_local(full, rank, world, None)
        sharding.upload_shard(c2, sh, whole_structure=True)
        n = sharding.run_shard_whole_structure(c2)
        parts.append(c2.atom_contacts_fetch(n['atom_atom']))
        for k in names:
            bags[k].append(c2.fetch_bag(k))
    # a partial selection under the assertion is refused
    part = np.ones(sh.pc.n_atoms, np.uint8)
    part[0] = 0
    c2.set_selection(part)
    with pytest.raises(Exception):
        c2.run_launch()
    c2.close()
    got = {k: np.concatenate([p[k] for p in parts]) for k in ('i', 'j', 'dist', 'sift', 'ctype')}
    o = np.lexsort((got['j'], got['i']))
    _assert_contacts_equal({k: v[o] for k, v in got.items()}, ref)
    order = {'plane_plane': ('bgn', 'end'), 'atom_plane': ('ring', 'atom'), 'group_group': ('bgn', 'end'), 'group_plane': ('amide', 'ring')}
    for k, (k1, k2) in order.items():
        g = {f: np.concatenate([b[f] for b in bags[k]]) for f in ref_bags[k]}
        o = np.lexsort((g[k2], g[k1]))
        for f in ref_bags[k]:
            a, b = g[f][o], ref_bags[k][f]
            assert np.array_equal(a, b) or (a.dtype.kind == 'f' and np.array_equal(np.isnan(a), np.isnan(b))
                                            and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])), (k, f)


def test_atom_accumulators(ctx):
    """per-atom sift masks and hbond/polar counters (I:821-852, 923-934; U:182-221)."""
    import oracle
    from helpers import random_dense_pack
    for seed in (11, 12):
        pc = random_dense_pack(seed, n=600, box=16.0)
        sel = (np.arange(pc.n_atoms) % 3 == 0).astype(np.uint8)
        ctx.set_complex(pc)
        ctx.make_selection(sel)
        got_c = ctx.atom_contacts()
        got = ctx.atom_accumulators()
        oc = oracle.OracleComplex(pc)
        oc.make_selection(sel, use_grid=False)
        exp_c = oc.atom_contacts(use_grid=False)
        _assert_contacts_equal(got_c, exp_c)
        exp = oracle.atom_accumulators(pc.n_atoms, exp_c)
        assert np.array_equal(got['sift'], exp['sift'])
        assert np.array_equal(got['counts'], exp['counts'])
        assert exp['counts'][:, 0].sum() > 0 and exp['counts'][:, 3].sum() > 0 and (exp['sift'][:, 1] != 0).any()


def test_config5_full_size(ctx):
    """BASELINE configs[4] at full size: 10k aromatic rings + 10k amides, every ring/amide kernel vs the oracle."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config5()
    assert pc.n_rings == 10_000 and pc.n_amides == 10_000
    ctx.set_complex(pc)
    ctx.make_selection(None)
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None)
    epp = oc.plane_plane()
    o = np.lexsort((epp['end'], epp['bgn']))
    epp = {k: v[o] for k, v in epp.items()}
    gpp = ctx.plane_plane()
    assert len(gpp['bgn']) > 40_000
    _assert_planes_equal(gpp, epp, ('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end'))
    assert set(np.unique(gpp['type1'])) == set(range(9))          # all nine FF..EF classes occur
    _assert_planes_equal(ctx.group_group(), oc.group_group(), ('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta'), tol=1e-4)
    _assert_planes_equal(ctx.group_plane(), oc.group_plane(), ('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta'))
    _assert_planes_equal(ctx.atom_plane(), oc.atom_plane(), ('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',))
    # properties of the plane-plane bag: one record per unordered pair, centroid distance <= 6
    key = np.minimum(gpp['bgn'], gpp['end']).astype(np.int64) * pc.n_rings + np.maximum(gpp['bgn'], gpp['end'])
    assert len(np.unique(key)) == len(key) and gpp['dist'].max() <= 6.0


def test_whole_structure_grid_is_kept_only_while_nothing_it_depends_on_changes(capi):
    """A whole-structure pass keeps its contact grid for the next one (arp_set_grid_reuse).  Every pass of a sequence that changes
    the selection, the cutoff, the structure, or overwrites the grid's buffers in between must equal the same pass on a context
    that builds its grid every time — all five bags, bit for bit — and the statistics must report the same atom count."""
    from arpeggio_amd import synth
    pcs = [synth.config3(20_000, seed=31), synth.proteinlike(seed=5)]
    keep, rebuild = capi.Context(0), capi.Context(0)
    rebuild.set_grid_reuse(False)

    def everything(cx, counts):
        out = {'atom_atom': cx.atom_contacts_fetch(counts['atom_atom'])}
        for k in ('atom_plane', 'plane_plane', 'group_group', 'group_plane'):
            out[k] = cx.fetch_bag(k)
        return out

    def same(step):
        a, b = step(keep), step(rebuild)
        assert dict(a[0]) == dict(b[0]), (dict(a[0]), dict(b[0]))
        for bag in a[1]:
            for col in a[1][bag]:
                x, y = a[1][bag][col], b[1][bag][col]
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (bag, col)
        assert a[2]['binned'] == b[2]['binned'] and a[2]['cells'] == b[2]['cells']

    def run(cutoff=5.0, comp=0.1, seq=False):
        def step(cx):
            c = cx.run_launch(cutoff, comp, seq)
            return c, everything(cx, c), cx.stats()
        return step

    for pc in pcs:
        part = (pc.res_id % 7 == 3).astype(np.uint8)
        for cx in (keep, rebuild):
            cx.set_complex(pc)
        same(run()); same(run()); same(run(5.0, 0.3, True))          # built, kept, kept (other per-pair parameters)
        same(run(4.0)); same(run(4.0)); same(run(5.0))                 # another cell edge, and back
        for cx in (keep, rebuild):
            cx.set_selection(part)
        same(run()); same(run())                                       # a partial selection compacts every time ...
        for cx in (keep, rebuild):
            cx.set_selection(np.ones(pc.n_atoms, np.uint8))
        same(run()); same(run())                                       # ... and selection_plus is whole again afterwards
        for cx in (keep, rebuild):
            cx.search_all(4.5)                                         # writes its own grid into the same buffers
        same(run()); same(run())
    for cx in (keep, rebuild):                                         # back to a structure seen before
        cx.set_complex(pcs[0])
    same(run()); same(run())
    launches = []
    for cx in (keep, rebuild):                                         # ... and the kept grid really is not built again
        cx.set_profiling(True)
        cx.kernel_times(reset=True)
        cx.run_launch()
        launches.append(cx.kernel_times(reset=True).get('bin', {}).get('launches', 0))
    assert launches[0] == 0 and launches[1] >= 1, launches
    keep.close(); rebuild.close()


def test_quarter_million_atoms_centre_grids(ctx):
    """The per-GPU size of BASELINE configs[3]: the ring / amide centre grids have 24 k cells here — k_point_grids keeps their
    histogram in global memory (above 12 288 cells; below, in LDS: every smaller test) — and the candidate lists are built on the
    second stream beside the first pass's search.  Ring / amide bags of run_launch against the oracle."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(250_000, seed=6)
    ctx.set_complex(pc)
    counts = ctx.run_launch()
    assert counts['plane_plane'] > 0 and counts['group_group'] > 0 and counts['group_plane'] > 0
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None)
    epp = oc.plane_plane()
    o = np.lexsort((epp['end'], epp['bgn']))
    epp = {k: v[o] for k, v in epp.items()}
    _assert_planes_equal(ctx.fetch_bag('plane_plane'), epp, ('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end'))
    _assert_planes_equal(ctx.fetch_bag('group_group'), oc.group_group(), ('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta'), tol=1e-4)
    _assert_planes_equal(ctx.fetch_bag('group_plane'), oc.group_plane(), ('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta'))
    again = ctx.run_launch()             # the resident pass (lists and grids in place) finds the same
    assert dict(again) == dict(counts)


def test_one_million_atoms_single_gpu(ctx):
    """Half of BASELINE configs[3] (2M atoms over 8 GPUs = 250k per GPU) times four on ONE GPU: parity with the
    grid oracle and the size-independent properties of the contact list."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(1_000_000, seed=4)
    ctx.set_complex(pc)
    counts = ctx.run_launch()
    got = ctx.atom_contacts_fetch(counts['atom_atom'])
    assert np.all(got['i'] < got['j'])
    key = got['i'].astype(np.int64) * pc.n_atoms + got['j']
    assert len(np.unique(key)) == len(key)
    ladder = got['sift'] & 0x1F
    assert np.all((ladder & (ladder - 1)) == 0) and np.all(ladder != 0)
    assert np.all(pc.res_id[got['i']] != pc.res_id[got['j']])       # I:729
    assert got['dist'].max() <= np.float32(5.0) * np.float32(1.000001)
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None)
    _assert_contacts_equal(got, oc.atom_contacts())


def test_staged_run_equals_run_launch(ctx):
    """arp_run_stage 0/1/2 (the sharded protocol, here without neighbours) == arp_run_launch."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(15000, seed=17)
    sel = (pc.res_id % 9 == 2).astype(np.uint8)
    ctx.set_complex(pc)
    ctx.set_selection(sel)
    ref_counts = ctx.run_launch()
    ref = ctx.atom_contacts_fetch(ref_counts['atom_atom'])
    ref_bags = {k: ctx.fetch_bag(k) for k in ('plane_plane', 'atom_plane', 'group_group', 'group_plane')}
    ctx.set_selection(sel)
    ctx.run_stage(0)
    ptr, nb = ctx.device_buffer(ctx.BUF_PLUS)
    assert ptr != 0 and nb == pc.n_atoms
    ctx.run_stage(1)
    ptr, nb = ctx.device_buffer(ctx.BUF_RES_SETS)
    assert nb == 2 * pc.n_residues
    counts = ctx.run_stage(2)
    assert counts == ref_counts
    _assert_contacts_equal(ctx.atom_contacts_fetch(counts['atom_atom']), ref)
    for k, b in ref_bags.items():
        g = ctx.fetch_bag(k)
        for f in b:
            assert np.array_equal(g[f], b[f], equal_nan=True) if b[f].dtype.kind == 'f' else np.array_equal(g[f], b[f]), (k, f)
    assert ctx.stats()['expand_candidates'] > 0


def test_device_exchange_over_rccl_world1():
    """DeviceExchange on the real transport (RCCL behind the C ABI, a one-rank communicator) with a HOST-assembled shard:
    the per-pass exchange calls run on the context's stream between the stages (gather / grouped send-recv / scatter,
    in-place ncclAllReduce of the residue sets), staged pass == arp_run_launch, repeatedly."""
    from arpeggio_amd import synth, sharding, _capi
    full = synth.slab_config(6000, 2, seed=8)
    sel = (full.res_id % 7 == 1).astype(np.uint8)
    sh = sharding.make_shard_distributed(full, 0, 1, None, sel=sel)
    ctx = _capi.Context(0)
    ctx.comm_init(0, 1, _capi.Context.comm_unique_id())
    sharding.upload_shard(ctx, sh)
    ex = sharding.DeviceExchange(ctx, sh)
    for _ in range(3):
        c1 = sharding.run_shard_device(ctx, ex)
    a = ctx.atom_contacts_fetch(c1['atom_atom'])
    ref = _capi.Context(0)
    ref.set_complex(full)
    ref.set_selection(sel)
    c2 = ref.run_launch()
    b = ref.atom_contacts_fetch(c2['atom_atom'])
    assert c1 == c2, (c1, c2)
    for k in ('i', 'j', 'sift', 'ctype'):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a['dist'].view(np.uint32), b['dist'].view(np.uint32))
    ctx.comm_destroy()
    ctx.close(); ref.close()


@pytest.mark.parametrize('selectors', [['/A/508/'], [], ['RESNAME:PHE'], ['LIGANDS']])
def test_proteinlike_stand_in_for_1tqn(ctx, selectors):
    """BASELINE configs[0]/[1] stand-in (`1tqn_h.cif` itself is unavailable): hydrogenated protein-like structure,
    `-s /A/508/` and whole-structure runs through the drop-in class, every bag against the oracle."""
    import oracle
    from arpeggio_amd import synth
    from arpeggio_amd.core import InteractionComplex, config, utils
    pc = synth.proteinlike()
    assert (pc.flags & config.F_HYDROGEN).astype(bool).sum() > 2000          # explicit hydrogens are atoms too
    ic = InteractionComplex(pc)
    ic._ctx = ctx
    ic.initialize()
    ic.run_arpeggio(selectors, 5.0, 0.1, False)
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[utils.selection_parser(selectors, pc) if selectors else slice(None)] = 1
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel, use_grid=False)
    assert np.array_equal(ic.selection_plus, np.nonzero(plus)[0])
    exp = oc.atom_contacts(use_grid=False)
    _assert_contacts_equal(ic._bags['atom_atom'], exp)
    from helpers import boundary_sensitive_pairs, report_boundary_pairs
    report_boundary_pairs('standin_' + ('whole' if not selectors else selectors[0].strip('/').replace('/', '_')),
                          boundary_sensitive_pairs(pc, ic._bags['atom_atom']))
    assert not (pc.flags[exp['i']] & config.F_HYDROGEN).any() and not (pc.flags[exp['j']] & config.F_HYDROGEN).any()
    epp = oc.plane_plane()
    o = np.lexsort((epp['end'], epp['bgn']))
    epp = {k: v[o] for k, v in epp.items()}
    _assert_planes_equal(ic._bags['plane_plane'], epp, ('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end'))
    _assert_planes_equal(ic._bags['atom_plane'], oc.atom_plane(), ('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',))
    _assert_planes_equal(ic._bags['group_group'], oc.group_group(), ('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta'), tol=1e-4)
    _assert_planes_equal(ic._bags['group_plane'], oc.group_plane(), ('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta'))
    contacts = ic.get_contacts()
    assert len(contacts) == len(exp['i']) + len(epp['bgn']) + len(ic._bags['atom_plane']['atom']) + \
        len(ic._bags['group_group']['bgn']) + len(ic._bags['group_plane']['amide'])
    if selectors == ['/A/508/']:
        ents = {c['interacting_entities'] for c in contacts}
        assert 'INTER' in ents and 'INTRA_NON_SELECTION' in ents
        hem = [c for c in contacts if c['type'] == 'atom-atom' and 'HEM' in (c['bgn']['label_comp_id'], c['end']['label_comp_id'])]
        assert hem and all(c['bgn']['auth_seq_id'] == 508 or c['end']['auth_seq_id'] == 508 for c in hem)
    ic._ctx = None     # the fixture owns the context


def test_config4_two_million_atoms_sharded_equals_single_gpu(capi):
    """BASELINE configs[3] at full size: 2 M atoms in 8 x-slabs.  Run once unsharded on one GPU and once as the 8 shards
    the ranks of `bench.py --gpus 8` would hold (one after the other on this GPU, whole-structure path, no exchange):
    the union of what the shards own is the single-GPU contact list — ids, SIFts, contact types, float32 distances —
    plus the size-independent properties of the list."""
    from arpeggio_amd import sharding, synth
    full = synth.slab_config(250_000, 8, seed=4)
    assert full.n_atoms == 2_000_000
    c1 = capi.Context(0)
    c1.set_complex(full)
    counts = c1.run_launch()
    ref = c1.atom_contacts_fetch(counts['atom_atom'])
    ref_pp = c1.fetch_bag('plane_plane')
    ref_ap = c1.fetch_bag('atom_plane')
    again = c1.run_launch()
    assert again == counts                                                    # idempotent
    c1.close()
    n = len(ref['i'])
    assert n > 20_000_000 and np.all(ref['i'] < ref['j'])
    key = ref['i'].astype(np.int64) * full.n_atoms + ref['j']
    assert np.all(np.diff(key) > 0)                                           # sorted, no duplicate pair
    ladder = ref['sift'] & 0x1F
    assert np.all((ladder & (ladder - 1)) == 0) and np.all(ladder != 0)       # exactly one of clash .. proximal
    assert np.all(full.res_id[ref['i']] != full.res_id[ref['j']])             # I:729
    assert ref['dist'].max() <= np.float32(5.0) * np.float32(1.000001)
    d = np.linalg.norm(full.xyz[ref['i'][::97]].astype(np.float64) - full.xyz[ref['j'][::97]].astype(np.float64), axis=1)
    assert np.abs(d - ref['dist'][::97]).max() < 1e-5                         # the north star's distance bound
    # the full contact list against the C oracle (about ten seconds of CPU), bit for bit
    import oracle
    from helpers import boundary_sensitive_pairs, report_boundary_pairs
    exp = oracle.OracleComplex(full).atom_contacts(5.0, 0.1, False)
    for f in ('i', 'j', 'sift', 'ctype'):
        assert np.array_equal(ref[f], exp[f]), f
    assert np.array_equal(ref['dist'].view(np.uint32), exp['dist'].view(np.uint32))
    del exp
    report_boundary_pairs('config4_2M_atoms', boundary_sensitive_pairs(full, ref))
    parts, pp_parts, ap_parts = [], [], []
    c2 = capi.Context(0)
    for rank in range(8):
        sh = sharding.make_shard_local(full, rank, 8, None)
        sharding.upload_shard(c2, sh, whole_structure=True)
        k = sharding.run_shard_whole_structure(c2)
        parts.append(c2.atom_contacts_fetch(k['atom_atom'], sort=False))
        pp_parts.append(c2.fetch_bag('plane_plane'))
        ap_parts.append(c2.fetch_bag('atom_plane'))
    c2.close()
    got = {f: np.concatenate([p[f] for p in parts]) for f in ('i', 'j', 'dist', 'sift', 'ctype')}
    assert len(got['i']) == n
    o = np.argsort(got['i'].astype(np.int64) * full.n_atoms + got['j'], kind='stable')
    for f in ('i', 'j', 'sift', 'ctype'):
        assert np.array_equal(got[f][o], ref[f]), f
    assert np.array_equal(got['dist'][o].view(np.uint32), ref['dist'].view(np.uint32))
    for bags, refbag, k1, k2 in ((pp_parts, ref_pp, 'bgn', 'end'), (ap_parts, ref_ap, 'ring', 'atom')):
        g = {f: np.concatenate([b[f] for b in bags]) for f in refbag}
        o = np.lexsort((g[k2], g[k1]))
        assert np.array_equal(g[k1][o], refbag[k1]) and np.array_equal(g[k2][o], refbag[k2])
        assert np.array_equal(g['dist'][o], refbag['dist'])


@pytest.mark.parametrize('n_sel_res', [1, 6, 100, 400])
def test_run_launch_selection_plus_on_both_sides_of_the_small_selection_threshold(ctx, n_sel_res):
    """arp_run_launch computes selection_plus three ways (whole structure: nothing; few atoms: k_expand_small; otherwise
    the 6 A grid search): masks, ring / amide sets and contacts of each against the oracle."""
    import oracle
    from arpeggio_amd import synth
    pc = synth.config3(30_000, seed=23)
    sel = np.isin(pc.res_id, 37 + 11 * np.arange(n_sel_res)).astype(np.uint8)
    ctx.set_complex(pc)
    ctx.set_selection(sel)
    counts = ctx.run_launch()
    masks = ctx.make_selection_masks()
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel)
    assert np.array_equal(masks['plus'], plus)
    assert np.array_equal(masks['ring_plus'], oc.ring_plus) and np.array_equal(masks['amide_plus'], oc.amide_plus)
    assert np.array_equal(masks['ring_sel'], oc.ring_sel) and np.array_equal(masks['amide_sel'], oc.amide_sel)
    _assert_contacts_equal(ctx.atom_contacts_fetch(counts['atom_atom']), oc.atom_contacts())
    ap, eap = ctx.fetch_bag('atom_plane'), oc.atom_plane()
    assert np.array_equal(ap['atom'], eap['atom']) and np.array_equal(ap['ring'], eap['ring']) and np.array_equal(ap['mask'], eap['mask'])


@pytest.mark.parametrize('world', [2, 3])
def test_staged_protocol_between_contexts_on_one_gpu(capi, world):
    """The general sharded protocol (partial selection) with real data flow on one GPU: one context per shard,
    arp_run_stage 0 / 1 / 2, and between the stages exactly what DeviceExchange does over RCCL — every shard's halo atoms
    take their selection_plus bit from the owner's buffer, the residue sets are OR-ed over the shards — here with plain
    hipMemcpy on the contexts' device buffers (arp_device_buffer; torch is not used: its bundled HIP runtime cannot be
    initialised after the system one the library runs on).  The union of what the shards own == the single-context result."""
    from arpeggio_amd import sharding, synth
    from shard_cases import staged_exchange
    full = synth.slab_config(6000, 3, seed=8)
    rng = np.random.default_rng(11)
    sel = np.zeros(full.n_atoms, np.uint8)
    sel[np.isin(full.res_id, rng.choice(full.n_residues, full.n_residues // 12, replace=False))] = 1
    c0 = capi.Context(0)
    c0.set_complex(full)
    c0.set_selection(sel)
    k0 = c0.run_launch()
    ref = c0.atom_contacts_fetch(k0['atom_atom'])
    names = ('plane_plane', 'atom_plane', 'group_group', 'group_plane')
    ref_bags = {k: c0.fetch_bag(k) for k in names}
    c0.close()

    shards = [sharding.make_shard_local(full, r, world, sel) for r in range(world)]
    ctxs = [capi.Context(0) for _ in range(world)]
    for c, sh in zip(ctxs, shards):
        sharding.upload_shard(c, sh)
    parts, bags, _ = staged_exchange(ctxs, shards, names)
    for c in ctxs:
        c.close()
    got = {f: np.concatenate([p[f] for p in parts]) for f in ('i', 'j', 'dist', 'sift', 'ctype')}
    o = np.lexsort((got['j'], got['i']))
    _assert_contacts_equal({f: v[o] for f, v in got.items()}, ref)
    order = {'plane_plane': ('bgn', 'end'), 'atom_plane': ('ring', 'atom'), 'group_group': ('bgn', 'end'), 'group_plane': ('amide', 'ring')}
    for b, (k1, k2) in order.items():
        g = {f: np.concatenate([x[f] for x in bags[b]]) for f in ref_bags[b]}
        o = np.lexsort((g[k2], g[k1]))
        for f in ref_bags[b]:
            a, e = g[f][o], ref_bags[b][f]
            assert np.array_equal(a, e) or (a.dtype.kind == 'f' and np.array_equal(np.isnan(a), np.isnan(e))
                                            and np.array_equal(a[~np.isnan(a)], e[~np.isnan(e)])), (b, f)
    assert len(ref['i']) > 5_000 and len(ref_bags['plane_plane']['bgn']) > 0


@pytest.mark.parametrize('seed', range(48))
def test_random_parameters_and_selections(ctx, seed):
    """run_arpeggio with parameters off the defaults — cutoff 3 .. 8 A (incl. beyond the 6 A expansion radius), vdw_comp 0 .. 0.4,
    sequence-adjacent pairs on / off, selections from one residue to nearly everything — on structures of different kinds and
    sizes, every result bag against the oracle."""
    import oracle
    from arpeggio_amd import synth
    from helpers import random_dense_pack
    rng = np.random.default_rng(1000 + seed)
    kind = seed % 3
    if kind == 0:
        pc = synth.config3(int(rng.integers(1500, 30000)), seed=int(rng.integers(1, 1000)))
    elif kind == 1:
        pc = synth.proteinlike(n_res=int(rng.integers(40, 400)), n_waters=int(rng.integers(0, 120)), seed=int(rng.integers(1, 50)))
    else:
        pc = random_dense_pack(int(rng.integers(1, 1000)), n=int(rng.integers(200, 900)))
    cutoff = float(rng.choice([3.0, 4.0, 4.5, 5.0, 5.5, 6.5, 8.0]))
    comp = float(rng.choice([0.0, 0.1, 0.25, 0.4]))
    seq_adj = bool(rng.integers(0, 2))
    frac = float(rng.choice([0.0, 0.02, 0.3, 0.95, 1.0]))
    sel_res = rng.random(pc.n_residues) < frac
    if frac == 0.0:
        sel_res[int(rng.integers(0, pc.n_residues))] = True
    sel = sel_res[pc.res_id].astype(np.uint8)
    ctx.set_complex(pc)
    ctx.set_selection(sel)
    counts = ctx.run_launch(cutoff, comp, seq_adj, 6.0)
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel)
    masks = ctx.make_selection_masks()
    assert np.array_equal(masks['plus'], plus) and np.array_equal(masks['ring_plus'], oc.ring_plus) and np.array_equal(masks['amide_plus'], oc.amide_plus)
    tag = (seed, kind, pc.n_atoms, cutoff, comp, seq_adj, frac)
    try:
        exp = oc.atom_contacts(cutoff, comp, seq_adj)
    except Exception:
        exp = None
    if exp is not None and exp.get('err', 0) == 0:
        _assert_contacts_equal(ctx.atom_contacts_fetch(counts['atom_atom']), exp)
    epp = oc.plane_plane()
    o = np.lexsort((epp['end'], epp['bgn']))
    epp = {k: v[o] for k, v in epp.items()}
    _assert_planes_equal(ctx.fetch_bag('plane_plane'), epp, ('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end'))
    _assert_planes_equal(ctx.fetch_bag('atom_plane'), oc.atom_plane(), ('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',))
    _assert_planes_equal(ctx.fetch_bag('group_group'), oc.group_group(), ('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta'))
    _assert_planes_equal(ctx.fetch_bag('group_plane'), oc.group_plane(), ('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta'))
    assert counts['atom_atom'] >= 0, tag


def test_search_around_centres_equals_brute_force(ctx):
    """arp_search = NeighborSearch.search(center, radius) (I:960, 1463) for many centres: inclusive float64 test on the float32
    coordinates widened to float64, all atoms (hydrogens too), centres inside, on the border of and far outside the box."""
    from arpeggio_amd import synth
    pc = synth.proteinlike(n_res=200, n_waters=80, seed=4)
    ctx.set_complex(pc)
    rng = np.random.default_rng(3)
    x = pc.xyz.astype(np.float64)
    lo, hi = x.min(axis=0), x.max(axis=0)
    centers = np.concatenate([lo + rng.random((300, 3)) * (hi - lo), x[rng.choice(len(x), 50)], [lo - 2.0, hi + 3.9, hi + 500.0],
                              x[:5] + [3.0, 0.0, 0.0]])
    for radius in (3.0, 4.0, 6.0, 9.5):
        oc, oa = ctx.search(centers, radius)
        d = x[None, :, :] - centers[:, None, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        ec, ea = np.nonzero(d2 <= radius * radius)
        assert np.array_equal(oc, ec) and np.array_equal(oa, ea), radius
        assert len(oc) > 1000
    oc, oa = ctx.search(np.zeros((0, 3)), 4.0)
    assert len(oc) == 0
    with pytest.raises(Exception):
        ctx.search([[np.nan, 0, 0]], 4.0)
    # the resident pass is not disturbed by the query's grid
    n1 = ctx.run_launch()
    ctx.search(centers[:10], 7.0)
    assert ctx.run_launch() == n1
