"""Ligand poses on a resident receptor (arp_poses_contacts_launch / _fetch / _info, Context.poses_contacts / poses_summary,
InteractionComplex.run_poses, arpeggio_amd.poses, synth.poses_of).

The yardstick is the ensemble route, which the new code does not touch: ``EnsembleComplex`` on ``poses.as_models(...)`` with the
same selection and parameters evaluates every pose as a whole model (each model pinned to its single run and to the oracle by
tests/test_models.py); of each model's atom-atom bag the rows with exactly one selected atom are what the pose must give.  For
one parameter set the oracle itself (``oracle.OracleComplex`` on the pose's pack) is held against the device as well.  Every
comparison is exact: ids, SIFt and contact type as integers, distances as bytes.  No tolerance anywhere, no time asserted."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, ligand_library, poses, synth
from arpeggio_amd.core import config, utils
from arpeggio_amd.core.interactions import EnsembleComplex, InteractionComplex
from helpers import concat_packs, tiny_complex

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
NEEDED = ('clash', 'covalent', 'hbond', 'weak_hbond', 'xbond', 'ionic', 'metal_complex', 'aromatic', 'hydrophobic', 'carbonyl', 'polar',
          'weak_polar')
PARAMS = ((5.0, 0.1, False), (4.0, 0.25, True), (6.0, 0.1, False))


# ------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def protein():
    return synth.proteinlike(n_res=40, seed=21, n_waters=20)


def _mask(pc, idx):
    m = np.zeros(pc.n_atoms, np.uint8)
    m[idx] = 1
    return m


def _residue_selector(pc, r):
    return '/%s/%d/' % (pc.res_chain[r], int(pc.res_seq[r]))


def _heavy_partners(pc, idx, radius=4.5):
    """Heavy atoms outside ``idx`` within ``radius`` of a heavy atom of ``idx`` (how busy a movable set's surroundings are)."""
    heavy = (np.asarray(pc.flags) & config.F_HYDROGEN) == 0
    mine = np.zeros(pc.n_atoms, bool)
    mine[idx] = True
    a, b = pc.xyz[mine & heavy].astype(np.float64), pc.xyz[~mine & heavy].astype(np.float64)
    return int((np.linalg.norm(a[:, None] - b[None], axis=2) <= radius).any(axis=0).sum())


def case_main():
    """HEM in the small protein, 70 poses (not a multiple of 64) with noise on atoms."""
    pc = protein()
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    x, h = synth.poses_of(pc, idx, 70, seed=11, shift=3.0, jitter=0.2)
    return pc, idx, x, h


def lys_residue(pc):
    """The mid-chain LYS (both sequence neighbours present) whose NZ is nearest to a negatively ionisable atom: the one whose
    poses reach an ionic contact."""
    neg = pc.xyz[(np.asarray(pc.type_mask) & config.ATOM_TYPE_BIT['neg ionisable']) != 0].astype(np.float64)

    def reach(r):
        nz = next(a for a in np.nonzero(pc.res_id == r)[0] if pc.atom_name[a] == 'NZ')
        return np.linalg.norm(neg - pc.xyz[nz], axis=1).min()
    return min((r for r in range(2, 38) if pc.res_name[r] == 'LYS'), key=reach)


def case_lys():
    """One LYS in mid-chain: hydrogens (as atoms and as rows), two peptide links, the sequence-adjacent gate.  32 turned poses with
    X-H stretched by 0.6, and pose 32 = the resident residue shifted by exactly 3 A along x with N-H stretched likewise."""
    pc = protein()
    r = lys_residue(pc)
    idx = utils.selection_parser([_residue_selector(pc, r)], pc)
    x, h = synth.poses_of(pc, idx, 32, seed=5, shift=3.0, jitter=0.0, stretch=0.6)
    atoms, rows = poses.movable(pc, idx)
    owner = np.repeat(np.arange(pc.n_atoms), np.diff(pc.h_off))[rows]
    d = np.array([3.0, 0.0, 0.0])
    x_last = (pc.xyz[atoms].astype(np.float64) + d).astype(np.float32)
    par = x_last[np.searchsorted(atoms, owner)].astype(np.float64)
    h_last = par + 1.6 * (pc.h_xyz[rows] + d - par)
    return pc, idx, np.concatenate([x, x_last[None]]), np.concatenate([h, h_last[None]])


def water_residue(pc):
    waters = [r for r in range(pc.n_residues) if pc.res_name[r] == 'HOH']
    return max(waters, key=lambda r: _heavy_partners(pc, np.nonzero(pc.res_id == r)[0]))


def case_water():
    """A single water (one heavy atom) walking through the protein: the contact types with a selected water."""
    pc = protein()
    idx = utils.selection_parser([_residue_selector(pc, water_residue(pc))], pc)
    x, h = synth.poses_of(pc, idx, 40, seed=3, shift=6.0, jitter=0.0)
    return pc, idx, x, h


def case_two_residues():
    pc = protein()
    idx = utils.selection_parser(['RESNAME:HEM', _residue_selector(pc, water_residue(pc))], pc)
    x, h = synth.poses_of(pc, idx, 8, seed=9, shift=2.0, jitter=0.1)
    return pc, idx, x, h


@functools.lru_cache(maxsize=None)
def soup():
    return synth.make_synthetic(3000, seed=5, box=(45, 45, 45), n_rings=30, n_amides=40)


def case_spread():
    """A movable set spread over the whole box: every benzene of the soup at once."""
    pc = soup()
    idx = utils.selection_parser(['RESNAME:BNZ'], pc)
    x, h = synth.poses_of(pc, idx, 16, seed=2, shift=2.0, jitter=0.3)
    return pc, idx, x, h


def case_seams():
    """HEM far away (100 A), half outside each face of the receptor's box, and back home."""
    pc = protein()
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    atoms, _ = poses.movable(pc, idx)
    x0 = pc.xyz[atoms].astype(np.float64)
    c = x0.mean(axis=0)
    lo, hi = pc.xyz.min(axis=0).astype(np.float64), pc.xyz.max(axis=0).astype(np.float64)
    moves = [np.array([100.0, 0.0, 0.0]), np.array([-100.0, -100.0, -100.0])]
    for ax in range(3):
        for face in (lo, hi):
            d = np.zeros(3)
            d[ax] = face[ax] - c[ax]
            moves.append(d)
    moves.append(np.zeros(3))
    x = np.stack([(x0 + d).astype(np.float32) for d in moves])
    return pc, idx, x, np.zeros((len(x), 0, 3))


def metal_partner_pack():
    """The small protein with one hand-made acceptor oxygen 2.3 A above the haem's iron (its own residue): proteinlike's chain
    keeps its acceptors further from the metal than the 2.8 A of a metal complex."""
    pc = protein()
    fe = int(np.nonzero((np.asarray(pc.flags) & config.F_METAL) != 0)[0][0])
    T = config.ATOM_TYPE_BIT
    q = tiny_complex([pc.xyz[fe].astype(np.float64) + np.array([0.0, 0.0, 2.3])], vdw=1.52, cov=0.66, type_mask=T['hbond acceptor'])
    both = concat_packs(pc, q)
    both.ring_atoms, both.amide_atoms = list(pc.ring_atoms), pc.amide_atoms      # (the protein comes first: its ids stand)
    return both, fe


def case_metal():
    pc, fe = metal_partner_pack()
    idx = np.nonzero(pc.res_id == pc.res_id[fe])[0]
    x, h = synth.poses_of(pc, idx, 4, seed=1, shift=0.3, jitter=0.0)
    return pc, idx, x, h


CASES = dict(main=case_main, lys=case_lys, water=case_water, two=case_two_residues, spread=case_spread, seams=case_seams, metal=case_metal)
CASE_PARAMS = dict(main=PARAMS, lys=((5.0, 0.1, False), (5.0, 0.1, True)), water=((5.0, 0.1, False),), two=((5.0, 0.1, False),),
                   spread=((5.0, 0.1, False),), seams=((5.0, 0.1, False),), metal=((5.0, 0.1, False),))


# ------------------------------------------------------------------------------------------------------------- yardsticks
def pose_pack(pc, X, H, p):
    q = copy.copy(pc)
    q.xyz, q.h_xyz = np.ascontiguousarray(X[p]), np.ascontiguousarray(H[p])
    return q


def oracle_rows(pc, idx, x, h, params):
    """Per pose: the oracle's pass over the pose's pack, its rows with exactly one selected atom."""
    X, H = poses.as_models(pc, idx, x, h)
    m = _mask(pc, idx)
    out = []
    for p in range(len(X)):
        oc = oracle.OracleComplex(pose_pack(pc, X, H, p))
        oc.make_selection(m)
        bag = oc.atom_contacts(*params)
        assert bag['err'] == 0
        out.append(poses.reference_rows(bag, m))
    return out


@functools.lru_cache(maxsize=None)
def ensemble_rows(name, params):
    """Per pose: the ensemble route's atom-atom bag of the pose as a model, its rows with exactly one selected atom."""
    pc, idx, x, h = CASES[name]()
    X, H = poses.as_models(pc, idx, x, h)
    ens = EnsembleComplex((copy.copy(pc), X, H))
    ens.run_arpeggio(np.asarray(idx), *params)
    m = _mask(pc, idx)
    rows = [poses.reference_rows(ens._results[f]['bags']['atom_atom'], m) for f in range(len(X))]
    ens._ctx.close()
    return rows


def as_table(rows, movable_atoms):
    """Per-pose rows as the table the device must return."""
    t = {k: np.concatenate([r[k] for r in rows]).astype(poses.DTYPES[k]) for k in poses.COLUMNS}
    t['pose_off'] = np.concatenate([[0], np.cumsum([len(r['i']) for r in rows])]).astype(np.uint64)
    t['summary'] = np.stack([poses.summarise(r['sift']) for r in rows]) if rows else np.zeros((0, 16), np.uint32)
    t['movable'] = np.asarray(movable_atoms, np.int32)
    return t


def differences(got, want):
    """The names of what differs: columns as integers, distances as bytes, offsets, summary."""
    bad = [k for k in ('i', 'j', 'sift', 'ctype') if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    if got['dist'].dtype != np.float32 or got['dist'].tobytes() != want['dist'].tobytes():
        bad.append('dist')
    bad += [k for k in ('pose_off', 'summary', 'movable') if not np.array_equal(got[k], want[k])]
    return bad


def check_consistent(t, info=None):
    """pose_off, summary and info against the records themselves, and the canonical order."""
    off = t['pose_off'].astype(np.int64)
    P = len(off) - 1
    assert off[0] == 0 and off[-1] == len(t['i']) and (np.diff(off) >= 0).all()
    assert t['summary'].shape == (P, 16) and np.array_equal(t['summary'][:, 15].astype(np.int64), np.diff(off))
    for p, r in enumerate(poses.split(t)):
        assert np.array_equal(t['summary'][p], poses.summarise(r['sift'])), p
        key = r['i'].astype(np.int64) << 32 | r['j'].astype(np.int64)
        assert (r['i'] < r['j']).all() and (np.diff(key) > 0).all(), p
    sel = np.isin(t['i'], t['movable']).astype(int) + np.isin(t['j'], t['movable']).astype(int)
    assert (sel == 1).all()
    if info is not None:
        assert info['poses'] == P and info['records'] == len(t['i']) and info['atoms'] == len(t['movable'])


def index_bits(count):
    """The bits of the ids 0 ... count - 1 in a sort key (index_bits of csrc/arp_api.hip)."""
    return max(int(count - 1).bit_length(), 1)


def most_records_of_a_wave(t):
    """The most records one wave of k_poses_contacts queues within one pose: wave w takes the movable atoms at positions
    s = w (mod 4) of the ascending movable set.  More than POSES_QCAP - 64 = 192 of them: the wave flushed its queue inside the pose."""
    wave = np.searchsorted(t['movable'], poses.partners(t)[0]) % 4
    return int(np.bincount(poses.pose_of(t) * 4 + wave).max()) if len(wave) else 0


def device_table(ctx, pc, idx, x, h, params):
    ctx.set_selection(_mask(pc, idx))
    return ctx.poses_contacts(x, h, *params)


def _ctx(pc):
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    return ctx


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_table():
    """Three poses over the small protein's HEM: 2, 0 and 3 records, written by hand."""
    pc = protein()
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    lig, rec = int(idx[0]), [int(a) for a in np.nonzero(pc.res_id == 3)[0][:3]]
    rows = [dict(i=[rec[0], rec[1]], j=[lig, lig], dist=[3.0, 4.004], sift=[BIT['vdw'] | BIT['hbond'], BIT['proximal']], ctype=[CT['INTER']] * 2),
            dict(i=[], j=[], dist=[], sift=[], ctype=[]),
            dict(i=[rec[0], rec[2], rec[2]], j=[lig, lig, lig + 1], dist=[2.5, 3.5, 3.25],
                 sift=[BIT['clash'], BIT['proximal'] | BIT['hydrophobic'], BIT['vdw_clash'] | BIT['polar']], ctype=[CT['INTER']] * 3)]
    rows = [{k: np.asarray(v, poses.DTYPES[k]) for k, v in r.items()} for r in rows]
    return pc, idx, rows, as_table(rows, idx)


def test_movable_lists_atoms_and_hydrogen_rows():
    pc = protein()
    r = lys_residue(pc)
    idx = utils.selection_parser([_residue_selector(pc, r)], pc)
    atoms, rows = poses.movable(pc, idx)
    assert np.array_equal(atoms, np.nonzero(pc.res_id == r)[0]) and (np.diff(atoms) > 0).all()
    owner = np.repeat(np.arange(pc.n_atoms), np.diff(pc.h_off))
    assert np.array_equal(rows, np.nonzero(pc.res_id[owner] == r)[0]) and len(rows) == 7      # H, HA, 2 HB, 3 HZ as rows of N, CA, CB, NZ
    a2, r2 = poses.movable(pc, _mask(pc, idx))                       # a mask selects the same
    assert np.array_equal(a2, atoms) and np.array_equal(r2, rows)
    with pytest.raises(ValueError):
        poses.movable(pc, np.ones(3, np.uint8))


def test_as_models_scatters_and_movable_reads_back():
    pc, idx, x, h = case_lys()
    atoms, rows = poses.movable(pc, idx)
    X, H = poses.as_models(pc, idx, x, h)
    assert X.shape == (33, pc.n_atoms, 3) and X.dtype == np.float32 and H.shape == (33, len(pc.h_xyz), 3) and H.dtype == np.float64
    assert np.array_equal(X[:, atoms], x) and np.array_equal(H[:, rows], h)           # the round trip
    rest, hrest = np.setdiff1d(np.arange(pc.n_atoms), atoms), np.setdiff1d(np.arange(len(pc.h_xyz)), rows)
    assert all(np.array_equal(X[p, rest], pc.xyz[rest]) and np.array_equal(H[p, hrest], pc.h_xyz[hrest]) for p in range(33))
    with pytest.raises(ValueError):
        poses.as_models(pc, idx, x[:, :-1], h)


def test_poses_of_starts_at_home_and_moves_rigidly():
    pc = protein()
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    atoms, rows = poses.movable(pc, idx)
    x, h = synth.poses_of(pc, idx, 6, seed=4, shift=3.0)
    assert x.shape == (6, len(atoms), 3) and h.shape == (6, len(rows), 3)
    assert np.array_equal(x[0], pc.xyz[atoms]) and np.array_equal(h[0], pc.h_xyz[rows])
    pos = {int(a): k for k, a in enumerate(atoms)}
    bonds = [(pos[i], pos[int(j)]) for i in atoms.tolist() for j in pc.bond_idx[pc.bond_off[i]:pc.bond_off[i + 1]] if int(j) in pos and i < j]
    assert len(bonds) >= 20
    b = np.array(bonds)
    length = np.linalg.norm(x[:, b[:, 0]].astype(np.float64) - x[:, b[:, 1]], axis=2)
    assert np.abs(length - length[0]).max() < 1e-4                      # (float32 coordinates of ~30 A: 4e-6 each)
    assert np.abs(x[1:] - x[0]).max() > 0.5                             # ... and the poses do move
    # stretch scales parent - hydrogen vectors, jitter breaks rigidity
    pc2, idx2, x2, h2 = case_lys()
    at2, rows2 = poses.movable(pc2, idx2)
    owner = np.searchsorted(at2, np.repeat(np.arange(pc2.n_atoms), np.diff(pc2.h_off))[rows2])
    xh = np.linalg.norm(h2 - x2[:, owner].astype(np.float64), axis=2)
    assert np.allclose(xh[1:], 1.6 * xh[0], atol=1e-4) and xh[0].max() < 1.01


def test_split_concat_and_summary_on_the_hand_made_table():
    pc, idx, rows, t = hand_table()
    assert t['pose_off'].tolist() == [0, 2, 2, 5] and poses.n_poses(t) == 3 and poses.pose_of(t).tolist() == [0, 0, 2, 2, 2]
    assert t['summary'][0].tolist() == [0, 0, 0, 1, 1, 1] + [0] * 9 + [2] and t['summary'][1].tolist() == [0] * 16
    parts = poses.split(t)
    assert len(parts) == 3 and all(np.array_equal(parts[p][k], rows[p][k]) for p in range(3) for k in poses.COLUMNS)
    check_consistent(t)
    joined = poses.concat([as_table(rows[:1], idx), as_table(rows[1:], idx)])
    assert differences(joined, t) == []
    assert differences(poses.concat([t]), t) == [] and poses.n_poses(poses.concat([])) == 0
    with pytest.raises(ValueError):
        poses.concat([t, as_table(rows, idx[:-1])])


def test_the_library_module_shares_these_names_and_the_join_of_concat():
    """ligand_library re-exports the objects of poses, and the helper both ``concat`` functions share reproduces them on the
    hand-made tables of the two modules' tests."""
    for name in ('SUMMARY', 'N_BITS', 'n_poses', 'pose_of', 'summarise'):
        assert getattr(ligand_library, name) is getattr(poses, name), name
    pc, idx, rows, t = hand_table()
    off, summary = poses.join_poses([as_table(rows[:1], idx), as_table(rows[1:], idx)])
    assert off.dtype == np.uint64 and np.array_equal(off, t['pose_off']) and summary.dtype == np.uint32 and np.array_equal(summary, t['summary'])
    assert np.array_equal(poses.join_pose_off([[0, 2], [0], [0, 0, 3]]), [0, 2, 2, 5])
    from test_ligand_library import hand_table as library_hand_table
    r, lt = library_hand_table()
    chunks = [ligand_library.from_rows([r[0], [], r[2][:1]]), ligand_library.from_rows([[], [], r[2][1:]])]
    off, summary = poses.join_poses(chunks)
    assert np.array_equal(off, lt['pose_off']) and np.array_equal(summary, lt['summary'])
    joined = ligand_library.concat(chunks)
    assert np.array_equal(joined['pose_off'], off) and np.array_equal(joined['summary'], summary) and joined['pose_off'].dtype == np.uint64


def test_fingerprints_records_and_csv_of_the_hand_made_table(tmp_path):
    pc, idx, rows, t = hand_table()
    lig_atoms, rec_atoms = poses.partners(t)
    assert set(lig_atoms.tolist()) <= set(idx.tolist()) and not set(rec_atoms.tolist()) & set(idx.tolist())
    bits, res = poses.fingerprints(t, pc)
    assert res.tolist() == [3] and bits.shape == (3, 1, 15)
    on = lambda *names: [n in names for n in config.SIFT_NAMES]
    assert bits[0, 0].tolist() == on('vdw', 'hbond', 'proximal') and not bits[1].any()
    assert bits[2, 0].tolist() == on('clash', 'proximal', 'hydrophobic', 'vdw_clash', 'polar')
    abits, at = poses.fingerprints(t, pc, level='atom')
    assert at.tolist() == sorted(set(rec_atoms.tolist())) and abits.shape == (3, 3, 15) and abits[2, 2].tolist() == on('proximal', 'hydrophobic', 'vdw_clash', 'polar')
    with pytest.raises(ValueError):
        poses.fingerprints(t, pc, level='chain')
    recs = poses.to_records(t, pc)
    assert [r['pose'] for r in recs] == [0, 0, 2, 2, 2] and recs[0]['contact'] == ['vdw', 'hbond'] and recs[0]['type'] == 'atom-atom'
    assert recs[0]['end']['label_comp_id'] == 'HEM' and recs[0]['bgn']['auth_seq_id'] == 4 and recs[1]['distance'] == 4.0
    assert recs[0]['interacting_entities'] == 'INTER' and sorted(recs[0]) == ['bgn', 'contact', 'distance', 'end', 'interacting_entities', 'pose', 'type']
    ic = InteractionComplex(pc)
    ic.poses = t
    path = ic.write_poses(str(tmp_path))
    lines = open(path).read().splitlines()
    assert path.endswith('proteinlike.poses') and lines[0] == ','.join(poses.CSV_HEADER) and len(lines) == 6
    assert lines[1].split(',')[:3] == ['0', 'A/4/' + pc.atom_name[int(t['i'][0])], 'A/508/' + pc.atom_name[int(idx[0])]] and lines[1].split(',')[4] == 'vdw|hbond'


def test_the_oracle_alone_meets_the_coverage_condition():
    """What the GPU coverage test asserts of the ensemble route's rows, asserted here of the oracle's: the cases reach every
    contact the feature must get right (seeds and shifts were chosen for it; the metal complex needs the hand-made partner)."""
    seen = 0
    ctypes = set()
    for name in ('main', 'lys', 'water', 'metal'):
        pc, idx, x, h = CASES[name]()
        for r in oracle_rows(pc, idx, x, h, CASE_PARAMS[name][-1]):
            seen |= int(np.bitwise_or.reduce(r['sift'])) if len(r['sift']) else 0
            ctypes |= set(r['ctype'].tolist())
    assert [n for n in NEEDED if not seen & BIT[n]] == []
    assert {CT['INTER'], CT['SELECTION_WATER']} <= ctypes


# ------------------------------------------------------------------------------------------------------------- GPU: parity
@pytest.mark.gpu
@pytest.mark.parametrize('params', PARAMS, ids=[f'{c}-{v}-{int(s)}' for c, v, s in PARAMS])
def test_main_parity_with_the_ensemble_route(params):
    pc, idx, x, h = case_main()
    want = as_table(ensemble_rows('main', params), idx)
    ctx = _ctx(pc)
    got = device_table(ctx, pc, idx, x, h, params)
    # both id columns are packed atom ids: one width for both (k_pose_columns with hi_bits == lo_bits), and neither outgrows it
    assert max(int(got['i'].max()), int(got['j'].max())).bit_length() <= index_bits(pc.n_atoms)
    assert differences(got, want) == []
    check_consistent(got, ctx.poses_info())
    assert ctx.poses_info()['hydrogens'] == 0 and len(got['i']) > 70 * 100
    if params == PARAMS[0]:      # ... and against the oracle itself
        assert differences(got, as_table(oracle_rows(pc, idx, x, h, params), idx)) == []
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('seq_adjacent', (False, True))
def test_a_mid_chain_lysine_with_hydrogens_links_and_the_gate(seq_adjacent):
    pc, idx, x, h = case_lys()
    params = (5.0, 0.1, seq_adjacent)
    rows = ensemble_rows('lys', params)
    want = as_table(rows, idx)
    ctx = _ctx(pc)
    got = device_table(ctx, pc, idx, x, h, params)
    assert differences(got, want) == []
    check_consistent(got, ctx.poses_info())
    assert ctx.poses_info()["hydrogens"] == 7
    r = int(pc.res_id[idx[0]])
    name = {int(a): pc.atom_name[int(a)] for a in range(pc.n_atoms)}
    links = {(r - 1, 'C', 'N'), (r + 1, 'N', 'C')}       # (neighbour residue, its atom, the lysine's atom)

    def covalent_links(t):
        lig, rec = poses.partners(t)
        cov = (t['sift'] & BIT['covalent']) != 0
        return {(int(pc.res_id[b]), name[int(b)], name[int(a)]) for a, b in zip(lig[cov].tolist(), rec[cov].tolist())}
    per_pose = poses.split(got)
    home, shifted = dict(per_pose[0], movable=got['movable']), dict(per_pose[32], movable=got['movable'])
    if seq_adjacent:
        # pose 0 is the resident residue: both peptide bonds; pose 32 is 3 A away, its peptide bonds longer than any resident
        # bond, and still COVALENT (membership in the bond list, I:748-757)
        assert covalent_links(home) == links and covalent_links(shifted) == links
        atoms, _ = poses.movable(pc, idx)
        pos = {name[int(a)]: k for k, a in enumerate(atoms)}
        prev_c = next(a for a in np.nonzero(pc.res_id == r - 1)[0] if name[int(a)] == 'C')
        stretched = np.linalg.norm(x[32, pos['N']].astype(np.float64) - pc.xyz[prev_c])
        longest = max(np.linalg.norm(pc.xyz[i].astype(np.float64) - pc.xyz[j]) for i in range(pc.n_atoms) for j in pc.bond_idx[pc.bond_off[i]:pc.bond_off[i + 1]])
        assert stretched > longest + 0.5      # (3.91 A against 3.11 A, the haem's Fe-C bond: the longest of the structure)
    else:
        assert covalent_links(home) == set() and covalent_links(shifted) == set()      # the gate drops the neighbours' records
    # hydrogens 1.6 A from their parents — beyond the longest resident X-H distance — still give the reference's hbond bits
    hb = sum(int(((rw['sift'] & BIT['hbond']) != 0).sum()) for rw in rows[1:])
    assert hb > 0 and int(got['summary'][1:, 5].sum()) == hb
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ('water', 'two', 'spread', 'metal'))
def test_other_movable_sets_equal_the_ensemble_route(name):
    pc, idx, x, h = CASES[name]()
    params = CASE_PARAMS[name][0]
    rows = ensemble_rows(name, params)
    ctx = _ctx(pc)
    got = device_table(ctx, pc, idx, x, h, params)
    assert differences(got, as_table(rows, idx)) == []
    check_consistent(got, ctx.poses_info())
    if name == 'water':       # one heavy atom: every record is the water's oxygen with a receptor atom
        heavy = [int(a) for a in idx if not pc.flags[a] & config.F_HYDROGEN]
        assert len(heavy) == 1 and (poses.partners(got)[0] == heavy[0]).all()
        # fewer than 4 movable atoms: a wave of every block has no atom, and its empty queue goes through the drain at the end
        assert len(idx) == 3 and len(got['i']) > 0
        # (a selected water beside an unselected atom that is no water is NON_SELECTION_WATER: the fifth assignment of I:643-691 overrides the fourth)
        assert set(got['ctype'].tolist()) == {CT['NON_SELECTION_WATER'], CT['WATER_WATER']} and len(got['i']) > 100
    if name == 'two':         # HEM and a water selected at once: no row joins the two
        both = np.isin(got['i'], idx) & np.isin(got['j'], idx)
        assert not both.any() and len(set(pc.res_id[poses.partners(got)[0]].tolist())) == 2
    if name == 'spread':
        assert len(idx) == 180 and len(set(pc.res_id[idx].tolist())) == 30 and len(got['i']) > 16 * 500
    if name == 'metal':
        assert (got['sift'] & BIT['metal_complex']).any()
    ctx.close()


@pytest.mark.gpu
def test_box_seams_far_away_half_outside_and_one_pose():
    pc, idx, x, h = case_seams()
    params = (5.0, 0.1, False)
    rows = ensemble_rows('seams', params)
    want = as_table(rows, idx)
    ctx = _ctx(pc)
    got = device_table(ctx, pc, idx, x, None, params)
    assert differences(got, want) == []
    off = got['pose_off'].astype(np.int64)
    assert off[0] == off[1] == off[2] == 0 and not got['summary'][:2].any()              # 100 A away: nothing, equal offsets
    per = np.diff(off)
    assert (per[2:8] > 0).sum() >= 4 and per[8] == per.max() > 300                       # most faces have partners, home has most
    for p in (8, 0, 4):                                                                  # P = 1
        one = ctx.poses_contacts(x[p:p + 1], None, *params)
        assert (len(one['i']) == 0) == (p == 0)                                          # pose 0 alone: a result of no record at all
        assert differences(one, as_table(rows[p:p + 1], idx)) == [] and ctx.poses_info()['poses'] == 1
    ctx.close()


@pytest.mark.gpu
def test_the_reference_rows_cover_every_contact_the_feature_must_get_right():
    """Asserted on the REFERENCE side: the ensemble route's rows over the cases above hold every one of these bits."""
    seen = 0
    for name, plist in CASE_PARAMS.items():
        for params in plist:
            for r in ensemble_rows(name, params):
                seen |= int(np.bitwise_or.reduce(r['sift'])) if len(r['sift']) else 0
    assert [n for n in NEEDED if not seen & BIT[n]] == []


# ------------------------------------------------------------------------------------------------------------- GPU: state
def _fetch_everything(ctx):
    packed, _ = ctx.fetch_packed()
    bags = {name: {k: np.array(v) for k, v in bag.items()} for name, bag in packed.items()}      # (copies: the buffer is the context's)
    assert sorted(bags) == ['atom_atom', 'atom_plane', 'group_group', 'group_plane', 'plane_plane']
    return bags, ctx.residue_pairs(), ctx.networks()


def _same_bytes(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bytes(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_a_launch_voids_nothing_of_the_last_pass():
    pc, idx, x, h = case_main()
    ctx = _ctx(pc)
    ctx.set_selection(_mask(pc, idx))
    counts = ctx.run_launch(5.0, 0.1, False)
    assert counts['atom_atom'] > 0
    before = _fetch_everything(ctx)
    t = ctx.poses_contacts(x[:9], h[:9], 4.0, 0.25, True)         # (another cutoff: the static columns change their cell order)
    assert len(t['i']) > 0
    after = _fetch_everything(ctx)
    assert _same_bytes(before, after)
    # ... and the pass after it is the pass it was
    assert ctx.run_launch(5.0, 0.1, False) == counts and _same_bytes(_fetch_everything(ctx), before)
    ctx.close()


def _fetch_fails(ctx):
    n = C.c_int64(0)
    s = np.zeros((4096, 16), np.uint32)
    rc = ctx._L.arp_poses_contacts_fetch(ctx._h, 0, None, None, None, None, None, None, s.ctypes.data_as(C.c_void_p), C.byref(n))
    return rc == _capi.ARP_E_ARG


@pytest.mark.gpu
def test_the_result_goes_with_the_inputs_and_the_selection():
    pc, idx, x, h = case_main()
    m = _mask(pc, idx)
    ctx = _ctx(pc)
    assert _fetch_fails(ctx) and ctx.poses_info() == dict(poses=0, atoms=0, hydrogens=0, records=0)
    t = device_table(ctx, pc, idx, x[:5], h[:5], (5.0, 0.1, False))
    assert not _fetch_fails(ctx) and ctx.poses_info()['records'] == len(t['i'])
    ctx.set_selection(m)                                             # the same selection, uploaded again
    assert _fetch_fails(ctx) and ctx.poses_info()['poses'] == 0
    device_table(ctx, pc, idx, x[:5], h[:5], (5.0, 0.1, False))
    ctx.set_complex(pc)                                              # a new structure
    assert _fetch_fails(ctx)
    ctx.set_selection(m)
    device_table(ctx, pc, idx, x[:5], h[:5], (5.0, 0.1, False))
    ctx.set_topology(pc)
    assert not _fetch_fails(ctx)                                     # (the kept topology is not the resident structure)
    X, H = poses.as_models(pc, idx, x[:2], h[:2])
    ctx.set_models(X, H)
    assert _fetch_fails(ctx)
    ctx.close()


@pytest.mark.gpu
def test_every_refusal_names_its_cause():
    pc, idx, x, h = case_main()
    m = _mask(pc, idx)
    x, h = x[:3], h[:3]
    ctx = _capi.Context(0)
    L, hd = ctx._L, ctx._h
    n = C.c_int64(0)

    def launch(P=3, cutoff=5.0, xs=x):
        xs = np.ascontiguousarray(xs, np.float32)
        rc = L.arp_poses_contacts_launch(hd, P, xs.ctypes.data_as(C.c_void_p), None, cutoff, 0.1, 0, C.byref(n))
        return rc, L.arp_last_error(hd).decode()

    def refused(word, **kw):
        rc, msg = launch(**kw)
        assert rc == _capi.ARP_E_ARG and word in msg, (word, rc, msg)
    refused('no structure resident')
    ctx.set_complex(pc)
    refused('no uploaded selection')
    ctx.set_selection(np.ones(pc.n_atoms, np.uint8))
    refused('whole structure')
    ctx.set_selection(np.zeros(pc.n_atoms, np.uint8))
    refused('ARP_POSES_MAX_ATOMS')
    big = soup()
    ctx.set_complex(big)
    ctx.set_selection((np.arange(big.n_atoms) < 1025).astype(np.uint8))
    refused('ARP_POSES_MAX_ATOMS')
    ctx.set_complex(pc)
    ctx.set_selection(m)
    refused('ARP_POSES_MAX_POSES', P=0)
    refused('ARP_POSES_MAX_POSES', P=(1 << 20) + 1)
    refused('cutoff', cutoff=6.0000001)
    refused('cutoff', cutoff=0.0)
    refused('cutoff', cutoff=float('nan'))
    assert launch()[0] == _capi.ARP_OK and n.value > 0
    # single-bond neighbours as coordinates only: which atom moves with a pose is not known
    sb = np.where(pc.sb_nbr[:, None] >= 0, pc.xyz[np.maximum(pc.sb_nbr, 0)], 0).astype(np.float32)
    ctx._check(L.arp_set_single_bond_neighbour_coords(hd, sb.ctypes.data_as(C.c_void_p), (pc.sb_nbr >= 0).astype(np.uint8).ctypes.data_as(C.c_void_p)),
               'arp_set_single_bond_neighbour_coords')
    ctx.set_selection(m)
    refused('coordinates only')
    # a batch, models, shard ownership
    ctx.set_batch([pc, pc], [m, m])
    refused('batch')
    ctx.set_topology(pc)
    X, H = poses.as_models(pc, idx, x[:2], h[:2])
    ctx.set_models(X, H)
    ctx.set_selection(np.tile(m, 2))
    refused('models')
    ctx.set_complex(pc)
    ctx.set_selection(m)
    ctx._check(L.arp_set_ownership(hd, np.ones(pc.n_atoms, np.uint8).ctypes.data_as(C.c_void_p), np.arange(pc.n_atoms, dtype=np.int32).ctypes.data_as(C.c_void_p)),
               'arp_set_ownership')
    refused('shard')
    ctx.close()
    # the Python layer checks the shapes the library cannot see
    ctx = _ctx(pc)
    with pytest.raises(ValueError):
        ctx.poses_contacts(x, h)                                     # no selection yet
    ctx.set_selection(m)
    with pytest.raises(ValueError):
        ctx.poses_contacts(x[:, :-1], h)
    with pytest.raises(ValueError):
        ctx.poses_contacts(x, np.zeros((3, 1, 3)))
    ctx.close()


@pytest.mark.gpu
def test_a_nan_coordinate_is_found_on_the_device_and_leaves_no_result():
    pc, idx, x, h = case_lys()
    ctx = _ctx(pc)
    good = device_table(ctx, pc, idx, x[:4], h[:4], (5.0, 0.1, True))
    for where in ('atom', 'hydrogen', 'inf'):
        bx, bh = x[:4].copy(), h[:4].copy()
        if where == 'atom':
            bx[2, 3, 1] = np.nan
        elif where == 'inf':
            bx[3, 0, 0] = np.inf
        else:
            bh[1, 6, 2] = np.nan
        with pytest.raises(ValueError, match='non-finite'):
            ctx.poses_contacts(bx, bh, 5.0, 0.1, True)
        # documented: a launch that has passed its argument checks voids the result before it: nothing is resident now
        assert _fetch_fails(ctx) and ctx.poses_info()['poses'] == 0
        again = ctx.poses_contacts(x[:4], h[:4], 5.0, 0.1, True)
        assert differences(again, good) == []
    # a refusal on the arguments leaves the resident result alone
    with pytest.raises(ValueError):
        ctx.poses_contacts(x[:4], h[:4], 7.0, 0.1, True)
    assert not _fetch_fails(ctx) and ctx.poses_info()['poses'] == 4
    ctx.close()


@pytest.mark.gpu
def test_capacity_null_pointers_and_the_summary_alone():
    pc, idx, x, h = case_main()
    ctx = _ctx(pc)
    t = device_table(ctx, pc, idx, x[:6], h[:6], (5.0, 0.1, False))
    k = len(t['i'])
    L, hd = ctx._L, ctx._h
    n = C.c_int64(0)
    i = np.full(k, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.arp_poses_contacts_fetch(hd, k - 1, None, p(i), None, None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_E_CAPACITY and n.value == k and (i == -7).all()          # the needed count, nothing written
    rc = L.arp_poses_contacts_fetch(hd, k, None, p(i), None, None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_OK and n.value == k and np.array_equal(i, t['i'])          # one column alone
    off = np.zeros(7, np.uint64)
    rc = L.arp_poses_contacts_fetch(hd, 0, p(off), None, None, None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_OK and np.array_equal(off, t['pose_off'])                  # no record asked for: cap is not looked at
    s = ctx.poses_summary(x[:6], h[:6], 5.0, 0.1, False)
    assert s.dtype == np.uint32 and np.array_equal(s, t['summary'])
    # A first buffer that is too small: 24 poses of a movable set of 256 heavy atoms in the middle of the protein at the widest
    # cutoff, 36.9 records per posed atom (tests/test_ligand_library.py counts them), more than the 32 the first buffer holds.
    # The launch is repeated with room for all; four poses at a time fit the first buffer, and joined they are the same records.
    lig = synth.ligand('chain', 6, size=256)
    both = ligand_library.complex_of(pc, lig)
    sel = np.arange(pc.n_atoms, both.n_atoms)
    bx, bh = synth.library_poses_of(pc, lig, pc.xyz.astype(np.float64).mean(axis=0), 24, seed=4, shift=1.0)
    ctx.set_complex(both)
    big = device_table(ctx, both, sel, bx, bh, (6.0, 0.3, False))
    assert len(big['i']) > max(1 << 16, 24 * 256 * 32)                                  # the first buffer was too small
    assert most_records_of_a_wave(big) > 192                                            # a wave flushed its queue inside a pose
    assert int(big['j'].max()).bit_length() == index_bits(both.n_atoms)                # the lower id column fills its width
    parts = [ctx.poses_contacts(bx[a:a + 4], bh[a:a + 4], 6.0, 0.3, False) for a in range(0, 24, 4)]
    assert all(len(q['i']) <= 1 << 16 for q in parts)                                   # ... and theirs was not
    assert differences(poses.concat(parts), big) == []
    check_consistent(big, None)
    ctx.close()


@pytest.mark.gpu
def test_a_caller_owned_stream_and_chunks_joined():
    from test_gpu_paths import _hip_runtime
    pc, idx, x, h = case_main()
    params = (5.0, 0.1, False)
    ctx = _ctx(pc)
    whole = device_table(ctx, pc, idx, x, h, params)
    parts = [ctx.poses_contacts(x[a:b], h[a:b], *params) for a, b in ((0, 1), (1, 64), (64, 70))]
    assert differences(poses.concat(parts), whole) == []
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    assert differences(ctx.poses_contacts(x, h, *params), whole) == []
    assert np.array_equal(ctx.poses_summary(x[:7], h[:7], *params), whole['summary'][:7])
    ctx.use_stream(0)                                               # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0
    # InteractionComplex.run_poses chunks the same way
    ic = InteractionComplex(copy.copy(pc))
    t = ic.run_poses(['RESNAME:HEM'], x, h, *params, chunk=32)
    assert differences(t, whole) == [] and differences(ic.run_poses(np.asarray(idx), x, h, *params), whole) == []
