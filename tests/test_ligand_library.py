"""A ligand library on a resident receptor (arp_set_ligand_library, arp_library_contacts_launch / _fetch / _info,
arp_library_best_launch / _fetch; Context.set_ligand_library / library_contacts / library_summary / library_best / library_info;
InteractionComplex.run_ligand_library; arpeggio_amd.ligand_library; synth.ligands / library_poses_of).

Two yardsticks, neither touched by the library's code:

  (A) the pose route: a ``Context`` on ``complex_of(receptor, ligand_l)`` — the receptor with the ligand appended as one more
      residue, uploaded as ONE structure —, ``set_selection`` of the ligand's atoms, ``poses_contacts`` on the same poses; j -> a =
      j - n (pinned to the ensemble route and the oracle by tests/test_poses.py)
  (B) ``oracle.OracleComplex`` on the pose's pack, for the main case with one parameter set

Every comparison is exact: ids, SIFt and contact type as integers, distances as bytes.  No tolerance anywhere, no time asserted."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, synth
from arpeggio_amd import ligand_library as ll
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
T = config.ATOM_TYPE_BIT
# every SIFt bit from clash to weak_polar but `covalent`: a ligand has no bond to the receptor (the contract), so no yardstick can
# give that bit for a receptor - ligand row; the coverage test asserts that the oracle indeed never does
NEEDED = tuple(n for n in config.SIFT_NAMES if n != 'covalent')
PARAMS = ((5.0, 0.1, False), (4.0, 0.0, True), (6.0, 0.3, False))
MAIN_P = (70, 1, 3, 0, 5, 2, 1)


# ------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def receptor():
    return synth.proteinlike(n_res=40, seed=21, n_waters=20)


def _atom(pc, res_name, atom_name, pick=0):
    hits = [a for a in range(pc.n_atoms) if pc.atom_name[a] == atom_name and pc.res_name[pc.res_id[a]] == res_name]
    return hits[pick]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _rotation(frm, to):
    """A rotation matrix that turns unit vector ``frm`` into unit vector ``to`` (Rodrigues)."""
    frm, to = _unit(frm), _unit(to)
    v, c = np.cross(frm, to), float(np.dot(frm, to))
    if np.linalg.norm(v) < 1e-9:
        if c > 0:
            return np.eye(3)
        p = _unit(np.cross(frm, [1.0, 0.0, 0.0] if abs(frm[0]) < 0.9 else [0.0, 1.0, 0.0]))
        return 2.0 * np.outer(p, p) - np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K / (1.0 + c)


def dock(lig, a, toward, anchor, u, dist):
    """One pose of ``lig``: atom ``a`` at ``anchor + dist u``, the ligand turned so that its own direction ``toward`` points
    back at the anchor (-u).  Returns ``(xyz float32 [1, S, 3], h_xyz float64 [1, SH, 3])``."""
    u = _unit(u)
    R = _rotation(toward, -u)
    x0 = lig.xyz.astype(np.float64)
    at = np.asarray(anchor, np.float64) + dist * u
    x = (x0 - x0[a]) @ R.T + at
    h = (lig.h_xyz.reshape(-1, 3) - x0[a]) @ R.T + at
    return x.astype(np.float32)[None], h[None]


def _stack(*poses):
    return np.concatenate([p[0] for p in poses]), np.concatenate([p[1] for p in poses])


@functools.lru_cache(maxsize=None)
def main_ligands():
    rec = receptor()
    hem = ll.from_residue(rec, int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]))
    return (synth.ligand('water', 1), synth.ligand('ion', 2), hem, synth.ligand('amine', 3), synth.ligand('halo', 4),
            synth.ligand('chain', 5, size=65), synth.ligand('chain', 6, size=256))


@functools.lru_cache(maxsize=None)
def case_main():
    """L = 7 (S = 1, 1, 23, 16, 12, 65, 256), P = 70, 1, 3, 0, 5, 2, 1: the ligand without poses sits in the middle."""
    rec, ligs = receptor(), main_ligands()
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    fe = rec.xyz[_atom(rec, 'HEM', 'FE')].astype(np.float64)
    acc = rec.xyz[_atom(rec, 'ASP', 'OD1')].astype(np.float64)
    poses = [synth.library_poses_of(rec, ligs[0], centre, 70, seed=3, shift=6.0),
             dock(ligs[1], 0, [1.0, 0.0, 0.0], acc, acc - centre, 2.3),                  # the ion 2.3 A from an acceptor
             synth.library_poses_of(rec, ligs[2], fe + [0.0, 0.0, 3.6], 3, seed=11, shift=1.5, jitter=0.2),
             None,
             synth.library_poses_of(rec, ligs[4], fe + [0.0, 0.0, 3.8], 5, seed=7, shift=2.0),
             synth.library_poses_of(rec, ligs[5], centre, 2, seed=5, shift=3.0, stretch=0.3),
             synth.library_poses_of(rec, ligs[6], centre, 1, seed=9)]
    assert tuple(0 if p is None else len(p[0]) for p in poses) == MAIN_P
    return rec, ligs, poses


@functools.lru_cache(maxsize=None)
def case_docked():
    """Hand-placed poses that reach what random placements do not: halogen bonds in both directions, hydrogen bonds decided by
    hydrogen rows on either side, a halogen weak hydrogen bond, metal complexes on either side, an ionic pair."""
    rec = receptor()
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    amine, halo, ion, chain = synth.ligand('amine', 3), synth.ligand('halo', 4), synth.ligand('ion', 2), synth.ligand('chain', 5, size=65)
    x = lambda a: rec.xyz[a].astype(np.float64)
    out_of = lambda a: x(a) - centre
    o_bb, o_asp = _atom(rec, 'ALA', 'O', 3), _atom(rec, 'ASP', 'OD1')
    nz = amine.atom_name.index('NZ')
    hz1 = amine.h_xyz[amine.h_off[nz]]
    amine_poses = _stack(dock(amine, nz, hz1 - amine.xyz[nz], x(o_bb), out_of(o_bb), 2.9),       # N-H ... O: the ligand donor's rows
                         dock(amine, nz, hz1 - amine.xyz[nz], x(o_asp), out_of(o_asp), 2.9))     # ... and an ionic pair
    cl, c1 = halo.atom_name.index('CL1'), halo.atom_name.index('C1')
    axis = halo.xyz[cl].astype(np.float64) - halo.xyz[c1]
    ca = _atom(rec, 'ALA', 'CA', 5)
    ha = rec.h_xyz[rec.h_off[ca]]
    halo_poses = _stack(dock(halo, cl, axis, x(o_bb), out_of(o_bb), 3.0),                         # C-Cl ... O: the ligand is the donor
                        dock(halo, cl, np.cross(axis, [0.0, 0.0, 1.0]), ha, ha - x(ca), 2.6))     # C-H ... Cl from the side
    ion_poses = dock(ion, 0, [1.0, 0.0, 0.0], x(o_bb), out_of(o_bb), 2.3)
    o_lig = next(a for a in range(chain.n_atoms) if chain.type_mask[a] & T['xbond acceptor'])
    back = chain.xyz.astype(np.float64).mean(axis=0) - chain.xyz[o_lig]
    fe, rcl, rcbb = _atom(rec, 'HEM', 'FE'), _atom(rec, 'HEM', 'CL1'), _atom(rec, 'HEM', 'CBB')
    n_bb = _atom(rec, 'ALA', 'N', 7)
    hn = rec.h_xyz[rec.h_off[n_bb]]
    chain_poses = _stack(dock(chain, o_lig, -back, x(rcl), x(rcl) - x(rcbb), 3.0),               # C-Cl ... O: the receptor is the donor
                         dock(chain, o_lig, -back, x(fe), [0.0, 0.0, 1.0], 2.3),                  # an acceptor on the receptor's metal
                         dock(chain, o_lig, -back, x(n_bb), hn - x(n_bb), 2.9))                   # N-H ... O: the receptor donor's rows
    return rec, (amine, halo, ion, chain), [amine_poses, halo_poses, ion_poses, chain_poses]


def halo_pair():
    """Two ligands that differ only in one atom's type mask and in sb_nbr, on identical poses next to each other."""
    halo = synth.ligand('halo', 4)
    other = copy.copy(halo)
    cl, c2 = halo.atom_name.index('CL1'), halo.atom_name.index('C2')
    other.type_mask = halo.type_mask.copy()
    other.type_mask[c2] |= T['hbond acceptor'] | T['xbond acceptor']
    other.sb_nbr = halo.sb_nbr.copy()
    other.sb_nbr[cl] = halo.atom_name.index('C4')          # (the halogen's angle is measured at another atom)
    return halo, other


# ------------------------------------------------------------------------------------------------------------- yardsticks
def _lig_mask(rec, lig):
    m = np.zeros(rec.n_atoms + lig.n_atoms, np.uint8)
    m[rec.n_atoms:] = 1
    return m


def oracle_rows(rec, ligs, poses, params):
    """(B) per ligand, per pose: the oracle's pass over the complex with the pose in, its receptor - ligand rows."""
    out = []
    for lig, item in zip(ligs, poses):
        rows = []
        for p in range(0 if item is None else len(item[0])):
            oc = oracle.OracleComplex(ll.complex_of(rec, lig, item[0][p], item[1][p]))
            oc.make_selection(_lig_mask(rec, lig))
            bag = oc.atom_contacts(*params)
            assert bag['err'] == 0
            rows.append(ll.reference_rows(bag, rec.n_atoms))
        out.append(rows)
    return out


def pose_route_rows(ctx, rec, ligs, poses, params):
    """(A) per ligand, per pose: ``poses_contacts`` on the complex with the ligand selected, j -> a = j - n."""
    out = []
    for lig, item in zip(ligs, poses):
        if item is None or len(item[0]) == 0:
            out.append([])
            continue
        ctx.set_complex(ll.complex_of(rec, lig))
        ctx.set_selection(_lig_mask(rec, lig))
        t = ctx.poses_contacts(item[0], item[1], *params)
        assert (t['i'] < rec.n_atoms).all() and (t['j'] >= rec.n_atoms).all()
        off = t['pose_off'].astype(np.int64)
        out.append([dict(i=t['i'][off[p]:off[p + 1]], a=(t['j'][off[p]:off[p + 1]] - rec.n_atoms).astype(np.int32), dist=t['dist'][off[p]:off[p + 1]],
                         sift=t['sift'][off[p]:off[p + 1]], ctype=t['ctype'][off[p]:off[p + 1]]) for p in range(len(off) - 1)])
    return out


@functools.lru_cache(maxsize=None)
def main_pose_route(params):
    rec, ligs, poses = case_main()
    ctx = _capi.Context(0)
    rows = pose_route_rows(ctx, rec, ligs, poses, params)
    ctx.close()
    return rows


def differences(got, want):
    """The names of what differs: columns as integers, distances as bytes, offsets, summary."""
    bad = [k for k in ('i', 'a', 'sift', 'ctype') if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    if got['dist'].dtype != np.float32 or got['dist'].tobytes() != want['dist'].tobytes():
        bad.append('dist')
    bad += [k for k in ('pose_off', 'summary', 'ligand_pose_off') if not np.array_equal(got[k], want[k])]
    return bad


def check_consistent(t, lib):
    """pose_off and summary against the records themselves, the canonical order, the id ranges."""
    off = t['pose_off'].astype(np.int64)
    Tn = len(off) - 1
    assert off[0] == 0 and off[-1] == len(t['i']) and (np.diff(off) >= 0).all()
    assert t['summary'].shape == (Tn, 16) and np.array_equal(t['summary'][:, 15].astype(np.int64), np.diff(off))
    S, _ = ll.sizes(lib)
    for l, per_pose in enumerate(ll.split(t)):
        for r in per_pose:
            key = r['i'].astype(np.int64) << 32 | r['a'].astype(np.int64)
            assert (np.diff(key) > 0).all() and (r['a'] >= 0).all() and (r['a'] < S[l]).all()
    for tt in range(Tn):
        assert np.array_equal(t['summary'][tt], ll.summarise(t['sift'][off[tt]:off[tt + 1]])), tt


def _ctx(pc):
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    return ctx


def index_bits(count):
    """The bits of the ids 0 ... count - 1 in a sort key (index_bits of csrc/arp_api.hip)."""
    return max(int(count - 1).bit_length(), 1)


def most_records_of_a_wave(t):
    """The most records one wave of k_library_contacts queues within one pose: wave w takes the ligand's atoms a = w (mod 4).  More
    than LIB_QCAP - 64 = 192 of them: the wave flushed its queue inside the pose."""
    return int(np.bincount(ll.pose_of(t) * 4 + t['a'] % 4).max()) if len(t['a']) else 0


def launch(ctx, lib, poses, params=PARAMS[0]):
    off, x, h = ll.flatten_poses(lib, poses)
    return ctx.library_contacts(off, x, h, *params)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_pack_from_residue_and_complex_of_round_trip():
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    S, SH = ll.sizes(lib)
    assert S.tolist() == [1, 1, 23, 16, 12, 65, 256] and SH.tolist()[:5] == [2, 0, 0, 11, 4] and ll.n_ligands(lib) == 7
    assert lib['atom_off'].dtype == np.int32 and lib['h_off'].dtype == np.int32 and lib['h_off'][-1] == SH.sum()
    for l, pc in enumerate(ligs):
        a0, a1 = lib['atom_off'][l], lib['atom_off'][l + 1]
        assert np.array_equal(lib['type_mask'][a0:a1], pc.type_mask) and np.array_equal(lib['flags'][a0:a1], pc.flags)
        assert np.array_equal(lib['vdw'][a0:a1], pc.vdw) and np.array_equal(lib['cov'][a0:a1], pc.cov)
        assert np.array_equal(lib['sb_nbr'][a0:a1], pc.sb_nbr)                    # (within the ligand: not shifted)
        assert np.array_equal(np.diff(lib['h_off'][a0:a1 + 1]), np.diff(pc.h_off))
    # HEM cut from the stand-in: the atoms of the residue in packed order, bonds and neighbours re-indexed
    hem, r = ligs[2], int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0])
    idx = np.nonzero(rec.res_id == r)[0]
    assert hem.n_atoms == 23 and hem.n_residues == 1 and hem.n_rings == 0 and np.array_equal(hem.xyz, rec.xyz[idx])
    assert hem.atom_name == [rec.atom_name[a] for a in idx] and hem.res_name == ['HEM'] and hem.res_flags[0] == 0
    assert np.array_equal(np.where(hem.sb_nbr >= 0, idx[np.maximum(hem.sb_nbr, 0)], -1), rec.sb_nbr[idx])
    assert len(hem.bond_idx) == sum(rec.bond_off[a + 1] - rec.bond_off[a] for a in idx)
    with pytest.raises(ValueError, match='bonded to another residue'):
        ll.from_residue(rec, 3)
    # the complex: the receptor unchanged, then the ligand as one more residue with the pose in
    x, h = poses[5]
    both = ll.complex_of(rec, ligs[5], x[1], h[1])
    n = rec.n_atoms
    assert both.n_atoms == n + 65 and both.n_residues == rec.n_residues + 1 and np.array_equal(both.xyz[:n], rec.xyz)
    assert np.array_equal(both.xyz[n:], x[1]) and np.array_equal(both.h_xyz[len(rec.h_xyz):], h[1]) and (both.res_id[n:] == rec.n_residues).all()
    assert np.array_equal(both.sb_nbr[n:], np.where(ligs[5].sb_nbr >= 0, ligs[5].sb_nbr + n, -1)) and both.res_flags[-1] == 0
    assert np.array_equal(ll.complex_of(rec, ligs[5]).xyz[n:], ligs[5].xyz)
    with pytest.raises(ValueError):
        ll.complex_of(rec, ligs[5], x[1][:-1])
    # flatten_poses: ligand-major, then pose-major
    off, fx, fh = ll.flatten_poses(lib, poses)
    assert off.tolist() == [0, 70, 71, 74, 74, 79, 81, 82] and len(fx) == 3 * int((np.array(MAIN_P) * S).sum()) and len(fh) == 3 * int((np.array(MAIN_P) * SH).sum())
    assert np.array_equal(fx[3 * 70:3 * 71], poses[1][0].reshape(-1)) and fx.dtype == np.float32 and fh.dtype == np.float64
    with pytest.raises(ValueError):
        ll.flatten_poses(lib, poses[:-1])


def test_every_refusal_of_pack_by_name():
    rec, ligs, _ = case_main()
    with pytest.raises(ValueError, match='MAX_LIGANDS'):
        ll.pack([])
    with pytest.raises(ValueError, match='not one residue'):
        ll.pack([ligs[0], rec])
    lys = copy.copy(ligs[3])
    lys.res_flags = np.array([config.R_POLYPEPTIDE | config.R_HAS_SEQ], np.uint8)
    with pytest.raises(ValueError, match='polypeptide'):
        ll.pack([lys])
    seq = copy.copy(ligs[3])
    seq.res_flags = np.array([config.R_HAS_SEQ], np.uint8)
    with pytest.raises(ValueError, match='sequence neighbours'):
        ll.pack([seq])
    with pytest.raises(ValueError, match='MAX_ATOMS'):
        ll.pack([synth.ligand('chain', 1, size=257)])
    good = ll.pack(ligs[:5])

    def broken(**kw):
        lib = {k: np.array(good[k]) for k in ll.ARRAYS}
        for k, (at, v) in kw.items():
            lib[k][at] = v
        return lib
    for cause, lib in (('atom_off must start at 0', broken(atom_off=(0, 1))), ('MAX_ATOMS', broken(atom_off=(1, 0))),
                       ('MAX_ATOMS', broken(atom_off=(3, 500))), ('h_off must start at 0', broken(h_off=(0, 1))),
                       ('h_off must not decrease', broken(h_off=(3, 0))), ('radii', broken(vdw=(4, np.nan))), ('radii', broken(cov=(4, -0.1))),
                       ('radii', broken(vdw=(2, np.inf))), ('sb_nbr', broken(sb_nbr=(2, 23))), ('sb_nbr', broken(sb_nbr=(2, -2))),
                       ('sb_nbr', broken(sb_nbr=(5, 3)))):          # (library atom 5 is atom 3 of the haem: its own index)
        with pytest.raises(ValueError, match=cause):
            ll.validate(lib)
    bad = copy.copy(ligs[4])
    bad.sb_nbr = bad.sb_nbr.copy()
    bad.sb_nbr[6] = 6
    with pytest.raises(ValueError, match='sb_nbr'):
        ll.pack([bad])
    assert ll.validate(good) is good


def hand_table():
    """Three ligands with 2, 0 and 3 poses; records written by hand."""
    def rows(i, a, d, s):
        return dict(i=np.array(i, np.int32), a=np.array(a, np.int32), dist=np.array(d, np.float32), sift=np.array(s, np.uint16),
                    ctype=np.full(len(i), CT['INTER'], np.uint8))
    r = [[rows([4, 9], [0, 0], [3.0, 4.004], [BIT['vdw'] | BIT['hbond'], BIT['proximal']]), rows([], [], [], [])],
         [],
         [rows([4], [1], [2.5], [BIT['clash']]), rows([7, 7, 8], [0, 2, 2], [3.5, 3.25, 3.0], [BIT['proximal'] | BIT['hydrophobic'], BIT['vdw_clash'] | BIT['polar'], BIT['vdw']]),
          rows([4], [0], [3.9], [BIT['proximal']])]]
    return r, ll.from_rows(r)


def test_split_concat_best_records_and_csv_on_a_hand_made_table(tmp_path):
    r, t = hand_table()
    assert t['pose_off'].tolist() == [0, 2, 2, 3, 6, 7] and t['ligand_pose_off'].tolist() == [0, 2, 2, 5] and ll.n_poses(t) == 5
    assert ll.pose_of(t).tolist() == [0, 0, 2, 3, 3, 3, 4] and ll.ligand_of(t).tolist() == [0, 0, 2, 2, 2]
    assert t['summary'][0].tolist() == [0, 0, 0, 1, 1, 1] + [0] * 9 + [2] and not t['summary'][1].any()
    parts = ll.split(t)
    assert [len(p) for p in parts] == [2, 0, 3]
    assert all(np.array_equal(parts[l][p][k], r[l][p][k]) for l in range(3) for p in range(len(r[l])) for k in ll.COLUMNS)
    # launches over consecutive ranges of the global poses, a ligand cut between two of them
    plan = ll.chunk_plan(t['ligand_pose_off'], 3)
    assert [(a, b) for _, a, b in plan] == [(0, 3), (3, 5)] and [o.tolist() for o, _, _ in plan] == [[0, 2, 2, 3], [0, 0, 0, 2]]
    first = ll.from_rows([r[0], [], r[2][:1]])
    second = ll.from_rows([[], [], r[2][1:]])
    assert differences(ll.concat([first, second]), t) == [] and differences(ll.concat([t]), t) == []
    with pytest.raises(ValueError):
        ll.concat([second, first])
    with pytest.raises(ValueError):
        ll.concat([])
    # best: scores 2*vdw + total = [4, 0 | 1, 5, 1]; a tie goes to the lower pose; the ligand without poses
    w = np.zeros(16, np.int64)
    w[3], w[15] = 2, 1
    b = ll.best(t, w)
    assert b['n_poses'].tolist() == [2, 0, 3] and b['best_pose'].tolist() == [0, -1, 3] and b['score'].tolist() == [4, ll.INT64_MIN, 5]
    w[:] = 0
    w[4] = -1                                           # minus the proximal records: [-1, 0 | 0, -1, -1]
    b = ll.best(t, w)
    assert b['best_pose'].tolist() == [1, -1, 2] and b['score'].tolist() == [0, ll.INT64_MIN, 0]
    assert ll.best(t, np.zeros(16))['best_pose'].tolist() == [0, -1, 2]      # all equal: the first pose of each ligand
    with pytest.raises(ValueError):
        ll.best(t, np.full(16, (1 << 24) + 1))
    # records and CSV: the receptor atom from the receptor's pack, the ligand atom from the ligand's own
    rec = receptor()
    ligs = [synth.ligand('halo', 4), synth.ligand('ion', 2), synth.ligand('amine', 3)]
    recs = ll.to_records(t, rec, ligs)
    assert [(x['ligand'], x['pose']) for x in recs] == [(0, 0), (0, 0), (2, 0), (2, 1), (2, 1), (2, 1), (2, 2)]
    assert recs[0]['contact'] == ['vdw', 'hbond'] and recs[0]['type'] == 'atom-atom' and recs[1]['distance'] == 4.0
    assert recs[0]['end']['label_comp_id'] == 'HAL' and recs[0]['end']['auth_atom_id'] == 'C1' and recs[0]['end']['auth_asym_id'] == 'L'
    assert recs[4]['end']['label_comp_id'] == 'LYF' and recs[4]['end']['auth_atom_id'] == 'CD' and recs[0]['bgn']['auth_atom_id'] == rec.atom_name[4]
    assert recs[0]['interacting_entities'] == 'INTER' and sorted(recs[0]) == ['bgn', 'contact', 'distance', 'end', 'interacting_entities', 'ligand', 'pose', 'type']
    ic = InteractionComplex(rec)
    ic.ligand_library = t
    ic.ligand_library_ligands = ligs
    path = ic.write_ligand_library(str(tmp_path))
    lines = open(path).read().splitlines()
    assert path.endswith('proteinlike.library') and lines[0] == ','.join(ll.CSV_HEADER) and len(lines) == 8
    assert lines[1].split(',') == ['0', '0', 'A/1/' + rec.atom_name[4], 'L/1/C1', '3.0', 'vdw|hbond', 'INTER']


def test_synthetic_ligands_are_what_they_say():
    ligs = synth.ligands(10, seed=3, sizes=(20, 60))
    assert [pc.res_name[0] for pc in ligs] == ['HOH', 'ZN', 'LYF', 'HAL', 'LIG'] * 2 and all(pc.n_residues == 1 and pc.res_flags[0] == 0 for pc in ligs)
    water, ion, amine, halo, chain = ligs[:5]
    assert water.n_atoms == 1 and len(water.h_xyz) == 2 and water.flags[0] & config.F_WATER and ion.flags[0] & config.F_METAL
    h_atoms = np.nonzero(amine.flags & config.F_HYDROGEN)[0]
    assert len(h_atoms) == 11 and len(amine.h_xyz) == 11 and np.array_equal(np.sort(amine.h_xyz, axis=0), np.sort(amine.xyz[h_atoms].astype(np.float64), axis=0))
    cl = halo.atom_name.index('CL1')
    assert halo.flags[cl] & config.F_HALOGEN and halo.element[halo.sb_nbr[cl]] == 'C' and halo.type_mask[cl] & T['xbond donor']
    assert 20 <= chain.n_atoms <= 60 and ligs[9].n_atoms != chain.n_atoms and not (chain.flags & config.F_HYDROGEN).any() and len(chain.h_xyz) > 0
    hal = np.nonzero(chain.flags & config.F_HALOGEN)[0]
    assert len(hal) > 0 and all(chain.element[chain.sb_nbr[a]] == 'C' for a in hal)
    assert all(abs(pc.xyz[(pc.flags & config.F_HYDROGEN) == 0].astype(np.float64).mean(axis=0)).max() < 1e-5 for pc in ligs)
    assert synth.ligands(3, seed=1, sizes=(30, 31, 32), kinds=('chain',))[2].n_atoms == 32
    # poses: pose 0 at the centre, the others rigid; stretch scales parent - hydrogen vectors
    rec = receptor()
    c = np.array([1.0, 2.0, 3.0])
    x, h = synth.library_poses_of(rec, chain, c, 4, seed=2, shift=3.0)
    assert x.shape == (4, chain.n_atoms, 3) and h.shape == (4, len(chain.h_xyz), 3) and x.dtype == np.float32 and h.dtype == np.float64
    assert np.abs(x[0].astype(np.float64).mean(axis=0) - c).max() < 1e-5 and np.abs(x[1:] - x[0]).max() > 0.5
    d = np.linalg.norm(x[:, 1:].astype(np.float64) - x[:, :-1], axis=2)
    assert np.abs(d - d[0]).max() < 1e-4
    x2, h2 = synth.library_poses_of(rec, chain, c, 2, seed=2, stretch=0.5)
    par = np.repeat(np.arange(chain.n_atoms), np.diff(chain.h_off))
    assert np.allclose(np.linalg.norm(h2 - x2[:, par].astype(np.float64), axis=2), 1.5, atol=1e-4)


def test_the_oracle_alone_meets_the_coverage_condition():
    """Asserted of the oracle's receptor - ligand rows over the main case and the docked case (placements were chosen for it)."""
    seen, ctypes, missing = 0, set(), []
    found = dict.fromkeys(('xbond ligand donor', 'xbond receptor donor', 'hbond ligand rows', 'hbond receptor rows', 'weak hbond halogen branch',
                           'metal ligand ion', 'metal receptor ion', 'water rule'), False)
    for rec, ligs, poses in (case_main(), case_docked()):
        for lig, rows in zip(ligs, oracle_rows(rec, ligs, poses, PARAMS[0])):
            for r in rows:
                seen |= int(np.bitwise_or.reduce(r['sift'])) if len(r['sift']) else 0
                ctypes |= set(r['ctype'].tolist())
                for i, a, s in zip(r['i'].tolist(), r['a'].tolist(), r['sift'].tolist()):
                    ti, ta, fi, fa = int(rec.type_mask[i]), int(lig.type_mask[a]), int(rec.flags[i]), int(lig.flags[a])
                    hi, ha = rec.h_off[i + 1] > rec.h_off[i], lig.h_off[a + 1] > lig.h_off[a]
                    water = (fi | fa) & config.F_WATER
                    if s & BIT['xbond']:
                        found['xbond ligand donor'] |= bool(ta & T['xbond donor'] and ti & T['xbond acceptor'])
                        found['xbond receptor donor'] |= bool(ti & T['xbond donor'] and ta & T['xbond acceptor'])
                    if s & BIT['hbond'] and not water:
                        # decided by the hydrogens of the only side that can donate
                        lig_donates, rec_donates = bool(ta & T['hbond donor'] and ti & T['hbond acceptor']), bool(ti & T['hbond donor'] and ta & T['hbond acceptor'])
                        found['hbond ligand rows'] |= lig_donates and not rec_donates and ha
                        found['hbond receptor rows'] |= rec_donates and not lig_donates and hi
                    if s & BIT['weak_hbond']:
                        # the halogen branches come last (I:873-886): one of them applies, so it decided
                        found['weak hbond halogen branch'] |= bool(fa & config.F_HALOGEN and ta & T['weak hbond acceptor'] and ti & (T['hbond donor'] | T['weak hbond donor']) and hi)
                    if s & BIT['metal_complex']:
                        found['metal ligand ion'] |= bool(fa & config.F_METAL)
                        found['metal receptor ion'] |= bool(fi & config.F_METAL)
                    if s & BIT['hbond'] and fa & config.F_WATER:          # I:791-802: a water beside a donor or an acceptor, no geometry
                        found['water rule'] |= bool(ti & (T['hbond acceptor'] | T['hbond donor']))
    missing += [n for n in NEEDED if not seen & BIT[n]] + [k for k, v in found.items() if not v]
    assert missing == []
    assert not seen & BIT['covalent']                     # no bond to the receptor: never covalent
    assert {CT['INTER'], CT['NON_SELECTION_WATER']} <= ctypes


# ------------------------------------------------------------------------------------------------------------- GPU: parity
@pytest.mark.gpu
@pytest.mark.parametrize('params', PARAMS, ids=[f'{c}-{v}-{int(s)}' for c, v, s in PARAMS])
def test_main_case_equals_the_pose_route_per_ligand(params):
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    want = ll.from_rows(main_pose_route(params))
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    got = launch(ctx, lib, poses, params)
    # the two id columns have widths of their own (k_pose_columns with hi_bits != lo_bits): a receptor id that the ligand atoms'
    # bits could not hold comes back whole
    assert index_bits(rec.n_atoms) != index_bits(256) and int(got['i'].max()).bit_length() > index_bits(256)
    # ligands of one atom: three waves of their blocks have no atom, and their empty queues go through the drain at the end
    assert ll.sizes(lib)[0][0] == 1 and int(got['pose_off'][70]) > 0
    assert differences(got, want) == []
    check_consistent(got, lib)
    info = ctx.library_info()
    assert info == dict(ligands=7, poses=82, records=len(got['i']), atoms=374, hydrogens=int(lib['h_off'][-1]), blocks=82, max_atoms=256, best=False)
    per_lig = [sum(len(r['i']) for r in rows) for rows in ll.split(got)]
    assert per_lig[3] == 0 and all(per_lig[l] > 0 for l in (0, 1, 2, 4, 5, 6)) and len(got['i']) > 5000
    if params == PARAMS[0]:      # ... and against the oracle itself
        assert differences(got, ll.from_rows(oracle_rows(rec, ligs, poses, params))) == []
    ctx.close()


@pytest.mark.gpu
def test_docked_poses_equal_the_pose_route():
    rec, ligs, poses = case_docked()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    got = launch(ctx, lib, poses)
    check_consistent(got, lib)
    other = _capi.Context(0)
    assert differences(got, ll.from_rows(pose_route_rows(other, rec, ligs, poses, PARAMS[0]))) == []
    other.close()
    assert (got['sift'] & BIT['xbond']).any() and (got['sift'] & BIT['metal_complex']).any() and (got['sift'] & BIT['ionic']).any()
    ctx.close()


@pytest.mark.gpu
def test_neighbouring_ligands_get_their_own_staged_rows():
    """Two ligands that differ only in one atom's type mask and in sb_nbr, on identical poses next to each other in pose_off:
    a block that kept the rows staged for the pose before would give both the same records."""
    rec, _, docked = case_docked()
    halo, other = halo_pair()
    x, h = docked[1]
    fe = rec.xyz[_atom(rec, 'HEM', 'FE')].astype(np.float64)
    more = synth.library_poses_of(rec, halo, fe + [0.0, 0.0, 3.8], 3, seed=7, shift=2.0)
    x, h = np.concatenate([x, more[0]]), np.concatenate([h, more[1]])
    ligs, poses = (halo, other, halo, other), [(x, h)] * 4
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    got = launch(ctx, lib, poses)
    ref = _capi.Context(0)
    assert differences(got, ll.from_rows(pose_route_rows(ref, rec, ligs, poses, PARAMS[0]))) == []
    ref.close()
    parts = ll.split(got)
    same = lambda u, v: all(np.array_equal(p[k], q[k]) for p, q in zip(u, v) for k in ll.COLUMNS)
    assert same(parts[0], parts[2]) and same(parts[1], parts[3]) and not same(parts[0], parts[1])
    ctx.close()


@pytest.mark.gpu
def test_seams_far_away_half_outside_one_pose_and_more_poses_than_blocks():
    rec, ligs, _ = case_main()
    hem, water = ligs[2], ligs[0]
    lib = ll.pack([hem, water])
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    # the haem 100 A away, half outside each face of the receptor's box, and at home
    x0 = hem.xyz.astype(np.float64)
    c = x0.mean(axis=0)
    lo, hi = rec.xyz.min(axis=0).astype(np.float64), rec.xyz.max(axis=0).astype(np.float64)
    moves = [np.array([100.0, 0.0, 0.0]), np.array([-100.0, -100.0, -100.0])]
    for ax in range(3):
        for face in (lo, hi):
            d = np.zeros(3)
            d[ax] = face[ax] - c[ax]
            moves.append(d)
    moves.append(np.zeros(3))
    x = np.stack([(x0 + d).astype(np.float32) for d in moves])
    poses = [(x, None), None]
    got = launch(ctx, lib, poses)
    ref = _capi.Context(0)
    rows = pose_route_rows(ref, rec, (hem, water), poses, PARAMS[0])
    assert differences(got, ll.from_rows(rows)) == []
    off = got['pose_off'].astype(np.int64)
    assert off[0] == off[1] == off[2] == 0 and not got['summary'][:2].any()              # 100 A away: nothing, equal offsets
    per = np.diff(off)
    assert (per[2:8] > 0).sum() >= 4 and per[8] == per.max() > 300
    for p in (8, 0, 4):                                                                  # T = 1
        one = launch(ctx, lib, [(x[p:p + 1], None), None])
        assert (len(one['i']) == 0) == (p == 0)                                          # pose 0 alone: a result of no record at all
        assert differences(one, ll.from_rows([rows[0][p:p + 1], []])) == [] and ctx.library_info()['poses'] == 1
    # 1030 poses of the water: more than one round of the offsets scan, and more poses than blocks (a second grid stride)
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    wx, wh = synth.library_poses_of(rec, water, centre, 1030, seed=13, shift=9.0)
    poses = [None, (wx, wh)]
    got = launch(ctx, lib, poses)
    info = ctx.library_info()
    assert info['poses'] == 1030 and 0 < info['blocks'] < 1030
    assert differences(got, ll.from_rows(pose_route_rows(ref, rec, (hem, water), poses, PARAMS[0]))) == []
    assert (np.diff(got['pose_off'].astype(np.int64))[1024:] > 0).any() and len(got['i']) > 10000
    ref.close()
    ctx.close()


@pytest.mark.gpu
def test_capacity_null_pointers_and_the_summary_alone():
    rec, ligs, _ = case_main()
    big = ligs[6]
    lib = ll.pack([big])
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    # 24 poses of the S = 256 ligand in the middle of the protein at the widest cutoff: 36.9 records per posed atom (counted on
    # the host: 226 793), more than the 32 the first buffer holds
    x, h = synth.library_poses_of(rec, big, centre, 24, seed=4, shift=1.0)
    poses = [(x, h)]
    params = PARAMS[2]
    t = launch(ctx, lib, poses, params)
    k = len(t['i'])
    assert k > max(1 << 16, 24 * 256 * 32)                                            # the first buffer was too small
    assert most_records_of_a_wave(t) > 192                                            # a wave flushed its queue inside a pose
    ref = _capi.Context(0)
    assert differences(t, ll.from_rows(pose_route_rows(ref, rec, (big,), poses, params))) == []
    ref.close()
    L, hd = ctx._L, ctx._h
    n = C.c_int64(0)
    i = np.full(k, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.arp_library_contacts_fetch(hd, k - 1, None, p(i), None, None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_E_CAPACITY and n.value == k and (i == -7).all()          # the needed count, nothing written
    rc = L.arp_library_contacts_fetch(hd, k, None, None, p(i), None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_OK and n.value == k and np.array_equal(i, t['a'])          # one column alone
    off = np.zeros(25, np.uint64)
    rc = L.arp_library_contacts_fetch(hd, 0, p(off), None, None, None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_OK and np.array_equal(off, t['pose_off'])                  # no record asked for: cap is not looked at
    fo, fx, fh = ll.flatten_poses(lib, poses)
    s = ctx.library_summary(fo, fx, fh, *params)
    assert s.dtype == np.uint32 and np.array_equal(s, t['summary'])
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: errors
def _fetch_fails(ctx):
    n = C.c_int64(0)
    s = np.zeros((2048, 16), np.uint32)
    rc = ctx._L.arp_library_contacts_fetch(ctx._h, 0, None, None, None, None, None, None, s.ctypes.data_as(C.c_void_p), C.byref(n))
    return rc == _capi.ARP_E_ARG


@pytest.mark.gpu
def test_non_finite_coordinates_are_found_on_the_device_and_leave_no_result():
    rec, ligs, docked = case_docked()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    good = launch(ctx, lib, docked)
    for which, at, value in (('x', (0, 1, 3, 1), np.nan), ('x', (3, 2, 64, 0), np.inf), ('h', (0, 0, 10, 2), np.nan), ('h', (1, 1, 0, 0), -np.inf)):
        poses = [(x.copy(), h.copy()) for x, h in docked]
        poses[at[0]][0 if which == 'x' else 1][at[1:]] = value
        with pytest.raises(ValueError, match='non-finite'):
            launch(ctx, lib, poses)
        assert _fetch_fails(ctx) and ctx.library_info()['poses'] == 0       # a launch past its argument checks voids the result before it
        assert differences(launch(ctx, lib, docked), good) == []
    with pytest.raises(ValueError, match='cutoff'):                          # a refusal on the arguments leaves the resident result alone
        launch(ctx, lib, docked, (7.0, 0.1, False))
    assert not _fetch_fails(ctx) and ctx.library_info()['poses'] == 8
    # a halogen-bond donor without a single-bond neighbour, on the pose where it is the donor of an accepted pair
    halo = copy.copy(ligs[1])
    halo.sb_nbr = halo.sb_nbr.copy()
    halo.sb_nbr[halo.atom_name.index('CL1')] = -1
    lib2 = ll.pack([halo])
    ctx.set_ligand_library(lib2)
    with pytest.raises(AttributeError):
        launch(ctx, lib2, [docked[1]])
    assert _fetch_fails(ctx)
    ctx.close()


@pytest.mark.gpu
def test_every_host_refusal_names_its_cause_in_order():
    rec, ligs, poses = case_main()
    good = ll.pack(ligs[:5])
    ctx = _capi.Context(0)
    L, hd = ctx._L, ctx._h
    n = C.c_int64(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def set_library(nlig=5, **kw):
        lib = {k: np.array(good[k]) for k in ll.ARRAYS}
        for k, v in kw.items():
            if v is None:
                lib[k] = None
            else:
                lib[k][v[0]] = v[1]
        rc = L.arp_set_ligand_library(hd, nlig, *[p(lib[k]) for k in ll.ARRAYS])
        return rc, L.arp_last_error(hd).decode()

    def lib_refused(word, **kw):
        rc, msg = set_library(**kw)
        assert rc == _capi.ARP_E_ARG and word in msg, (word, rc, msg)
    # the library: in the order of the header, an earlier cause wins over a later one
    lib_refused('ARP_LIBRARY_MAX_LIGANDS', nlig=0, vdw=None)
    lib_refused('ARP_LIBRARY_MAX_LIGANDS', nlig=(1 << 16) + 1)
    lib_refused('an array is missing', vdw=None, atom_off=(0, 1))
    lib_refused('atom_off must start at 0', atom_off=(0, 1), h_off=(0, 1))
    lib_refused('ARP_LIBRARY_MAX_ATOMS', atom_off=(1, 0), h_off=(0, 1))
    lib_refused('ARP_LIBRARY_MAX_ATOMS', atom_off=(3, 500))
    lib_refused('h_off must start at 0', h_off=(0, 1), vdw=(0, np.nan))
    lib_refused('h_off must not decrease', h_off=(3, 0), vdw=(0, np.nan))
    lib_refused('radii', vdw=(4, np.nan), sb_nbr=(2, 23))
    lib_refused('radii', cov=(4, -0.5))
    lib_refused('radii', cov=(4, np.inf))
    lib_refused('sb_nbr', sb_nbr=(2, 23))
    lib_refused('sb_nbr', sb_nbr=(2, -2))
    lib_refused('sb_nbr', sb_nbr=(5, 3))
    assert ctx.library_info()['ligands'] == 0
    # the launch
    off5, x5, h5 = ll.flatten_poses(good, poses[:5])

    def launch_raw(off=off5, cutoff=5.0, comp=0.1, xs=x5, hs=h5):
        off = None if off is None else np.ascontiguousarray(off, np.int64)
        rc = L.arp_library_contacts_launch(hd, p(off), p(xs), p(hs), cutoff, comp, 0, C.byref(n))
        return rc, L.arp_last_error(hd).decode()

    def refused(word, **kw):
        rc, msg = launch_raw(**kw)
        assert rc == _capi.ARP_E_ARG and word in msg, (word, rc, msg)
    refused('no structure resident')
    ctx.set_complex(rec)
    refused('no ligand library')
    assert set_library()[0] == _capi.ARP_OK and ctx.library_info()['ligands'] == 5
    refused('pose_off missing', off=None)
    refused('pose_off must start at 0', off=off5 + 1)
    refused('pose_off must not decrease', off=[0, 70, 69, 74, 74, 79], cutoff=9.0)
    refused('ARP_POSES_MAX_POSES', off=[0] * 6, cutoff=9.0)
    refused('ARP_POSES_MAX_POSES', off=[0, 0, 0, 0, 0, (1 << 20) + 1])
    refused('cutoff', cutoff=6.0000001, comp=np.nan)
    refused('cutoff', cutoff=0.0)
    refused('cutoff', cutoff=float('nan'))
    refused('vdw_comp', comp=np.inf, xs=None)
    refused('xyz missing', xs=None, hs=None)
    refused('h_xyz missing', hs=None)
    assert launch_raw()[0] == _capi.ARP_OK and n.value > 0
    # best: before a result, bad weights
    w = np.zeros(16, np.int32)
    w[0] = (1 << 24) + 1
    assert L.arp_library_best_launch(hd, p(w)) == _capi.ARP_E_ARG and 'ARP_SHORTLIST_MAX_WEIGHT' in L.arp_last_error(hd).decode()
    assert L.arp_library_best_launch(hd, None) == _capi.ARP_E_ARG and 'weights missing' in L.arp_last_error(hd).decode()
    nl = C.c_int64(0)
    assert L.arp_library_best_fetch(hd, 0, None, None, None, C.byref(nl)) == _capi.ARP_E_ARG            # no best-pose table yet
    w[0] = 1
    assert L.arp_library_best_launch(hd, p(w)) == _capi.ARP_OK
    best = np.zeros(5, np.int32)
    assert L.arp_library_best_fetch(hd, 4, None, p(best), None, C.byref(nl)) == _capi.ARP_E_CAPACITY and nl.value == 5
    assert L.arp_library_best_fetch(hd, 0, None, None, None, C.byref(nl)) == _capi.ARP_OK and nl.value == 5
    # a batch, models, shard ownership as the receptor: refused as the pose launches refuse them
    m = np.zeros(rec.n_atoms, np.uint8)
    m[:10] = 1
    ctx.set_batch([rec, rec], [m, m])
    refused('batch')
    ctx.set_topology(rec)
    X = np.stack([rec.xyz, rec.xyz])
    ctx.set_models(X, np.stack([rec.h_xyz, rec.h_xyz]))
    refused('models')
    ctx.set_complex(rec)
    ctx._check(L.arp_set_ownership(hd, p(np.ones(rec.n_atoms, np.uint8)), p(np.arange(rec.n_atoms, dtype=np.int32))), 'arp_set_ownership')
    refused('shard')
    ctx.close()
    # the Python layer checks the lengths the library cannot see
    ctx = _ctx(rec)
    with pytest.raises(ValueError, match='no ligand library'):
        ctx.library_contacts(off5, x5, h5)
    ctx.set_ligand_library(good)
    with pytest.raises(ValueError, match='pose_off'):
        ctx.library_contacts(off5[:-1], x5, h5)
    with pytest.raises(ValueError, match='xyz'):
        ctx.library_contacts(off5, x5[:-3], h5)
    with pytest.raises(ValueError, match='h_xyz'):
        ctx.library_contacts(off5, x5, h5[:-3])
    with pytest.raises(ValueError, match='h_off'):
        ctx.set_ligand_library(dict(good, h_off=good['h_off'][:-1]))
    with pytest.raises(ValueError, match='weights'):
        ctx.library_best(np.zeros(15))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
def _fetch_everything(ctx):
    packed, _ = ctx.fetch_packed()
    bags = {name: {k: np.array(v) for k, v in bag.items()} for name, bag in packed.items()}      # (copies: the buffer is the context's)
    return bags, ctx.residue_pairs(), ctx.networks()


def _same_bytes(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bytes(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _poses_fetch(ctx, P):
    t = dict(i=np.empty(1 << 16, np.int32), summary=np.empty((P, 16), np.uint32), pose_off=np.empty(P + 1, np.uint64))
    n = C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx._check(ctx._L.arp_poses_contacts_fetch(ctx._h, 1 << 16, p(t['pose_off']), p(t['i']), None, None, None, None, p(t['summary']), C.byref(n)), 'fetch')
    t['i'] = t['i'][:n.value]
    return t


@pytest.mark.gpu
def test_a_launch_voids_nothing_and_the_result_goes_with_its_inputs_only():
    rec, ligs, docked = case_docked()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    hem = np.nonzero(rec.res_id == int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]))[0]
    m = np.zeros(rec.n_atoms, np.uint8)
    m[hem] = 1
    ctx.set_selection(m)
    counts = ctx.run_launch(5.0, 0.1, False)
    px, ph = synth.poses_of(rec, hem, 4, seed=11, shift=2.0)
    ctx.poses_contacts(px, ph, 5.0, 0.1, False)
    before = _fetch_everything(ctx), _poses_fetch(ctx, 4)
    assert counts['atom_atom'] > 0 and len(before[1]['i']) > 0 and _fetch_fails(ctx)
    ctx.set_ligand_library(lib)
    t = launch(ctx, lib, docked, (4.0, 0.0, True))         # (another cutoff: the static columns change their cell order)
    assert len(t['i']) > 0 and _same_bytes((_fetch_everything(ctx), _poses_fetch(ctx, 4)), before)
    best = ctx.library_best(np.ones(16, np.int32))
    assert _same_bytes((_fetch_everything(ctx), _poses_fetch(ctx, 4)), before) and ctx.library_info()['best']
    # it reads no selection: it survives set_selection (which voids the poses result)
    ctx.set_selection(m)
    assert not _fetch_fails(ctx) and ctx.poses_info()['poses'] == 0 and _same_bytes(ctx.library_best(np.ones(16, np.int32)), best)
    # a new library launch replaces it and takes the best-pose table with it
    launch(ctx, lib, docked)
    nl = C.c_int64(0)
    assert not ctx.library_info()['best'] and ctx._L.arp_library_best_fetch(ctx._h, 0, None, None, None, C.byref(nl)) == _capi.ARP_E_ARG
    # refused after a new structure, models, a batch, a new library; the library itself stays through all but the last
    ctx.set_complex(rec)
    assert _fetch_fails(ctx) and ctx.library_info() == dict(ligands=4, poses=0, records=0, atoms=94, hydrogens=int(lib['h_off'][-1]), blocks=0, max_atoms=65, best=False)
    launch(ctx, lib, docked)
    ctx.set_topology(rec)
    assert not _fetch_fails(ctx)                            # (the kept topology is not the resident structure)
    ctx.set_models(np.stack([rec.xyz, rec.xyz]), np.stack([rec.h_xyz, rec.h_xyz]))
    assert _fetch_fails(ctx)
    ctx.set_complex(rec)
    launch(ctx, lib, docked)
    ctx.set_batch([rec, rec], [m, m])
    assert _fetch_fails(ctx)
    ctx.set_complex(rec)
    launch(ctx, lib, docked)
    ctx.set_ligand_library(lib)
    assert _fetch_fails(ctx) and ctx.library_info()['ligands'] == 4
    # the same library against a second receptor, without another set_ligand_library
    rec2 = synth.proteinlike(n_res=30, seed=5, n_waters=10)
    shift = rec.xyz.astype(np.float64).mean(axis=0) - rec2.xyz.astype(np.float64).mean(axis=0)
    rec2 = copy.copy(rec2)
    rec2.xyz = (rec2.xyz.astype(np.float64) + shift).astype(np.float32)
    rec2.h_xyz = rec2.h_xyz + shift
    ctx.set_complex(rec2)
    got = launch(ctx, lib, docked)
    ref = _capi.Context(0)
    assert differences(got, ll.from_rows(pose_route_rows(ref, rec2, ligs, docked, PARAMS[0]))) == [] and len(got['i']) > 100
    ref.close()
    ctx.close()


@pytest.mark.gpu
def test_best_pose_per_ligand_equals_the_host_mirror():
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    t = launch(ctx, lib, poses)
    w1 = np.array([-8, 0, -2, 1, 0, 5, 2, 6, 6, 6, 2, 1, 2, 1, 1, 0], np.int64)
    w2 = np.zeros(16, np.int64)
    w2[0], w2[2] = -(1 << 24), -1                        # negative weights; most poses of the water tie at 0
    for w in (w1, w2):
        got, want = ctx.library_best(w), ll.best(t, w)
        assert all(got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in ('n_poses', 'best_pose', 'score')), w
        assert got['best_pose'][3] == -1 and got['score'][3] == ll.INT64_MIN and got['n_poses'].tolist() == list(MAIN_P)
    score = (t['summary'][:70].astype(np.int64) * w2).sum(axis=1)
    assert (score == score.max()).sum() > 1                # the tie is real, and the lower id wins it
    assert ctx.library_best(w2)['best_pose'][0] == int(np.argmax(score))
    ctx.close()


@pytest.mark.gpu
def test_a_caller_owned_stream_and_run_ligand_library_chunked():
    from test_gpu_paths import _hip_runtime
    rec, ligs, poses = case_main()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    whole = launch(ctx, lib, poses)
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    assert differences(launch(ctx, lib, poses), whole) == []
    w = np.arange(16, dtype=np.int64) - 4
    assert _same_bytes(ctx.library_best(w), ll.best(whole, w))
    ctx.use_stream(0)                                               # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0
    ic = InteractionComplex(copy.copy(rec))
    t = ic.run_ligand_library(ligs, poses, *PARAMS[0])
    assert differences(t, whole) == [] and ic.ligand_library is t
    for chunk in (32, 71, 1):
        if chunk == 1:          # every pose a launch of its own: the first three ligands only
            few = ic.run_ligand_library(ligs[:3], poses[:3], *PARAMS[0], chunk=1)
            want = ll.from_rows(ll.split(whole)[:3])
            assert differences(few, want) == []
        else:
            assert differences(ic.run_ligand_library(ligs, poses, *PARAMS[0], chunk=chunk), whole) == []
    t = ic.run_ligand_library(ligs, poses, *PARAMS[0], chunk=40, weights=w)
    assert _same_bytes(ic.ligand_library_best, ll.best(whole, w))
