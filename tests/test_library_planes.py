"""A ligand library on a resident receptor, ring and amide contacts (arp_set_ligand_library_planes, arp_library_planes_launch /
_fetch / _info; Context.set_ligand_library_planes / library_planes / library_planes_summary / library_planes_info;
InteractionComplex.run_ligand_library(planes=True); arpeggio_amd.ligand_library; synth.PLANE_LIGAND_KINDS).

Two yardsticks, neither touched by the new code:

  (B) the definition: a ``Context`` on ``complex_of(receptor, ligand_l, xyz_pose)`` — the receptor with the ligand appended as one
      more residue, uploaded as ONE structure — with the ligand selected, ring and amide geometry and ring residues made by the
      device for the complex (as initialize() makes them: amide normals carry no SVD sign) and a pass over the whole structure;
      its four bags are cut by ``ligand_library.plane_reference_rows``
  (A) the pose route: ``set_plane_atoms`` and ``poses_planes`` on the same complex, the ligand's home coordinates 1 000 A away
      along x so that the home clause of arp_poses_planes_launch adds no ring

Every comparison is exact: ids, masks, classes and contact types as integers, every float column as bytes.  No tolerance anywhere,
no time asserted.  On the CPU the oracle stands in, fed ``ref_py`` geometry per pose; it is used for counts and classes only."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from oracle import ref_py
from arpeggio_amd import _capi, poses, synth
from arpeggio_amd import ligand_library as ll
from arpeggio_amd import library_fingerprints as lfp
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex
from helpers import tiny_complex
import test_ligand_library as tl

CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
AP = {n: 1 << k for k, n in enumerate(config.ATOM_PLANE_NAMES)}
T = config.ATOM_TYPE_BIT
TABLES = poses.PLANE_TABLES
_p = lambda a: a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------------------- cases
receptor = tl.receptor


def _ring(rec, res_name, pick=0):
    """Ring id, centre and unit normal (float64 of the float32 atoms) of the pick-th ring of a residue of that name."""
    r = [k for k in range(rec.n_rings) if rec.res_name[int(rec.res_id[rec.ring_atoms[k][0]])] == res_name][pick]
    c, n = ref_py.ring_geometry(rec.xyz, [rec.ring_atoms[r]])
    return r, c[0], n[0]


def _backbone_amide(rec, pick=3):
    """Amide id, centre and unit normal of a backbone amide between two ALA."""
    am = [a for a in range(rec.n_amides) if all(rec.res_name[int(rec.res_id[i])] == 'ALA' for i in rec.amide_atoms[a][:3])][pick]
    x = rec.xyz.astype(np.float64)
    N, Cc, O = (x[int(i)] for i in rec.amide_atoms[am][:3])
    nv = np.cross(Cc - (Cc + O + N) / 3.0, O - (Cc + O + N) / 3.0)
    return am, (Cc + N) / 2.0, nv / np.linalg.norm(nv)


def place(lig, point, direction, at, to):
    """One pose of ``lig``: its own point ``point`` at ``at``, turned so that its own ``direction`` becomes ``to``.  Returns
    ``(xyz float32 [1, S, 3], h_xyz float64 [1, SH, 3])``."""
    R = tl._rotation(direction, to)
    x0, p0 = lig.xyz.astype(np.float64), np.asarray(point, np.float64)
    x = (x0 - p0) @ R.T + np.asarray(at, np.float64)
    h = (lig.h_xyz.reshape(-1, 3) - p0) @ R.T + np.asarray(at, np.float64)
    return x.astype(np.float32)[None], h[None]


def _ring_centre(lig, q=0):
    return lig.xyz[np.asarray(lig.ring_atoms[q], np.int64)].astype(np.float64).mean(axis=0)


def _ring_normal(lig, q=0):
    return ref_py.ring_geometry(lig.xyz, [lig.ring_atoms[q]])[1][0]


def _amide_centre(lig, g=0):
    a = lig.amide_atoms[g]
    return (lig.xyz[a[0]].astype(np.float64) + lig.xyz[a[1]]) / 2.0


@functools.lru_cache(maxsize=None)
def main_ligands():
    rec = receptor()
    hem = ll.from_residue(rec, int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]), planes=True)
    return (synth.ligand('water', 1), synth.ligand('ion', 2), hem, synth.ligand('amine', 3), synth.ligand('arylamide', 4),
            synth.ligand('biaryl', 5), synth.ligand('halo', 6, planes=True))


MAIN_P = (3, 1, 3, 2, 5, 0, 2)


@functools.lru_cache(maxsize=None)
def case_main():
    """L = 7: water 3 poses, ion 1, the haem cut out with its rings 3, amine (no ring, no amide) 2, arylamide 5, biaryl 0 (the
    ligand without poses sits inside the list), halo with its ring 2."""
    rec, ligs = receptor(), main_ligands()
    fe = rec.xyz[tl._atom(rec, 'HEM', 'FE')].astype(np.float64)
    _, c0, n0 = _ring(rec, 'PHE', 0)
    _, c1, n1 = _ring(rec, 'PHE', 1)
    _, c2, n2 = _ring(rec, 'PHE', 2)
    ps = [synth.library_poses_of(rec, ligs[0], c0 + 0.8 * n0, 3, seed=3, shift=2.5),          # pose 0 takes the ring over
          tl.dock(ligs[1], 0, [1.0, 0.0, 0.0], c1, n1, 2.5),
          synth.library_poses_of(rec, ligs[2], fe + [0.0, 0.0, 3.6], 3, seed=11, shift=1.5, jitter=0.2),
          synth.library_poses_of(rec, ligs[3], c2 + 3.5 * n2, 2, seed=5, shift=1.5),
          synth.library_poses_of(rec, ligs[4], c1 + 3.8 * n1, 5, seed=7, shift=2.0),
          None,
          synth.library_poses_of(rec, ligs[6], c0 + 4.0 * n0, 2, seed=9, shift=1.0)]
    assert tuple(0 if p is None else len(p[0]) for p in ps) == MAIN_P
    return rec, ligs, ps


@functools.lru_cache(maxsize=None)
def case_docked():
    """Hand-placed poses: every kind of ring / amide contact between a ligand and the receptor, in both directions."""
    rec = receptor()
    amine, aryl, biaryl, halo = synth.ligand('amine', 3), synth.ligand('arylamide', 4), synth.ligand('biaryl', 5), synth.ligand('halo', 6, planes=True)
    z = np.array([0.0, 0.0, 1.0])
    _, c0, n0 = _ring(rec, 'PHE', 0)
    _, c3, n3 = _ring(rec, 'PHE', 3)
    _, c4, n4 = _ring(rec, 'PHE', 4)
    _, ac, an = _backbone_amide(rec)
    side = tl._unit(np.cross(n0, [1.0, 0.3, 0.2]))
    nz_l, ce_l = amine.atom_name.index('NZ'), amine.atom_name.index('CE')
    nz_r, ce_r = tl._atom(rec, 'LYS', 'NZ', 1), tl._atom(rec, 'LYS', 'CB', 1)          # (the stand-in's lysine is short: CB - NZ)
    out = tl._unit(rec.xyz[nz_r].astype(np.float64) - rec.xyz[ce_r])
    cl, c1 = halo.atom_name.index('CL1'), halo.atom_name.index('C1')
    aryl_poses = tl._stack(place(aryl, _ring_centre(aryl), z, c0 + 3.6 * n0, n0),                      # face to face, 3.6 A
                           place(aryl, _ring_centre(aryl), z, c0 + 5.0 * n0, side),                    # edge to face
                           place(aryl, _ring_centre(aryl), z, rec.xyz[nz_r] + 3.5 * out, out),         # a receptor LYS NZ above the ligand's ring
                           place(aryl, _amide_centre(aryl), z, ac + 3.8 * an, an),                     # the ligand's amide on a backbone amide
                           place(aryl, _amide_centre(aryl), z, c3 + 3.8 * n3, n3))                     # the ligand's amide over a receptor ring
    amine_poses = tl.dock(amine, nz_l, amine.xyz[nz_l].astype(np.float64) - amine.xyz[ce_l], c4, n4, 3.5)      # NZ 3.5 A above a ring centre
    halo_poses = tl.dock(halo, cl, halo.xyz[cl].astype(np.float64) - halo.xyz[c1], c3, -n3, 3.5)       # the halogen points at a ring
    biaryl_poses = tl._stack(place(biaryl, _ring_centre(biaryl, 0), _ring_normal(biaryl, 0), ac + 3.8 * an, an),     # a backbone amide over a ligand ring
                             place(biaryl, _ring_centre(biaryl, 1), _ring_normal(biaryl, 1), c4 - 3.7 * n4, n4))
    return rec, (aryl, amine, halo, biaryl), [aryl_poses, amine_poses, halo_poses, biaryl_poses]


def _lig_mask(rec, lig):
    m = np.zeros(rec.n_atoms + lig.n_atoms, np.uint8)
    m[rec.n_atoms:] = 1
    return m


def second_receptor():
    return synth.proteinlike(n_res=36, seed=22, n_waters=5, id='second')


# ------------------------------------------------------------------------------------------------------------- CPU
def planes_cpu(pc):
    """``pc`` with the planes initialize() makes for its coordinates (ref_py: device-independent)."""
    q = copy.copy(pc)
    q.ring_center, q.ring_normal = ref_py.ring_geometry(pc.xyz, pc.ring_atoms)
    q.ring_res = ref_py.ring_residues(pc.xyz, pc.res_id, q.ring_center)[0]
    q.amide_center, q.amide_normal = ref_py.amide_geometry(pc.xyz, pc.amide_atoms)
    return q


def test_pack_and_validate_planes_refuse_by_name():
    ligs = main_ligands()
    lib = ll.pack(ligs)
    assert [lib[k].dtype for k in ll.PLANE_ARRAYS] == [np.int32] * 5
    assert lib['ring_off'].tolist() == [0, 0, 0, 4, 4, 5, 7, 8] and lib['amide_off'].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    assert np.diff(lib['ring_atom_off']).tolist() == [5, 5, 5, 5, 6, 6, 6, 6] and lib['amide_atoms'].tolist() == [[6, 7, 8, 0]]
    # a pack without rings or amides gives empty ranges, and the keys of before are as they were
    plain = ll.pack([synth.ligand('halo', 6), synth.ligand('water', 1)])
    assert plain['ring_off'].tolist() == [0, 0, 0] and plain['ring_atom_off'].tolist() == [0] and plain['amide_atoms'].shape == (0, 4)
    assert all(np.array_equal(plain[k], ll.pack([synth.ligand('halo', 6, planes=True), synth.ligand('water', 1)])[k]) for k in ll.ARRAYS)

    def refused(word, **change):
        bad = dict(lib)
        bad.update(change)
        with pytest.raises(ValueError, match=word):
            ll.validate_planes(bad)
    refused('an array is missing', ring_atom_idx=None)
    refused('ring_off must start at 0', ring_off=lib['ring_off'] + 1)
    refused('ring_off must start at 0 and never decrease', ring_off=np.array([0, 0, 0, 4, 3, 5, 7, 8], np.int32))
    refused('ring_atom_off must start at 0 and never decrease', ring_atom_off=lib['ring_atom_off'][::-1].copy())
    refused('amide_off must start at 0 and never decrease', amide_off=np.array([0, 0, 1, 0, 0, 1, 1, 1], np.int32))
    many = np.repeat(np.arange(3, dtype=np.int32)[None], 33, axis=0)
    refused('more than PLANES_MAX_RINGS', ring_off=np.array([0, 0, 0, 33, 33, 33, 33, 33], np.int32), ring_atom_off=np.arange(0, 100, 3, dtype=np.int32),
            ring_atom_idx=many.reshape(-1))
    refused('more than PLANES_MAX_AMIDES', amide_off=np.array([0, 0, 0, 33, 33, 33, 33, 33], np.int32), amide_atoms=np.tile(np.array([0, 1, 2, -1], np.int32), (33, 1)))
    short = lib['ring_atom_off'].copy()
    short[1:] -= 3                                                   # the first ring keeps two atoms
    refused('at least three atoms', ring_atom_off=short, ring_atom_idx=lib['ring_atom_idx'][3:])
    idx = lib['ring_atom_idx'].copy()
    idx[-1] = ligs[6].n_atoms                                        # one past the halide's last atom
    refused('ring atom index outside its own ligand', ring_atom_idx=idx)
    idx[-1] = -1
    refused('ring atom index outside its own ligand', ring_atom_idx=idx)
    refused('amide atom index outside its own ligand', amide_atoms=np.array([[6, 7, 16, 0]], np.int32))
    ll.validate_planes(dict(lib, amide_atoms=np.array([[6, 7, 8, -1]], np.int32)))      # the fourth atom is not read
    over = copy.copy(ligs[6])
    over.ring_atoms = [np.array([0, 1, 12], np.int32)]
    with pytest.raises(ValueError, match='outside its own ligand'):
        ll.pack([over])


def test_from_residue_with_planes_round_trip_and_complex_of_carries_them():
    rec = receptor()
    r = int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0])
    idx = np.nonzero(rec.res_id == r)[0]
    hem = ll.from_residue(rec, r, planes=True)
    mine = [k for k in range(rec.n_rings) if rec.res_id[rec.ring_atoms[k][0]] == r]
    assert hem.n_rings == len(mine) == 4 and hem.n_amides == 0 and ll.from_residue(rec, r).n_rings == 0
    for q, k in enumerate(mine):
        assert np.array_equal(idx[hem.ring_atoms[q]], rec.ring_atoms[k]) and np.array_equal(hem.ring_center[q], rec.ring_center[k])
    assert hem.rings_not_in_path_order() == []
    # a PHE's ring lies in the residue, its amides are shared with the neighbours: refused by name
    phe = int(np.nonzero(np.array(rec.res_name) == 'PHE')[0][0])
    with pytest.raises(ValueError, match='bonded to another residue'):
        ll.from_residue(rec, phe, planes=True)
    # a ring or an amide that names atoms of two residues WITHOUT a bond between them (an inconsistent pack): refused by its own name
    loose = tiny_complex([[0.0, 0.0, 0.0], [1.4, 0.0, 0.0], [0.7, 1.2, 0.0], [0.7, -1.2, 0.0]], res_id=[0, 0, 0, 1])
    loose.ring_atoms = [np.array([0, 1, 3], np.int32)]
    loose.ring_center, loose.ring_normal, loose.ring_res = np.zeros((1, 3)), np.zeros((1, 3)), np.zeros(1, np.int32)
    with pytest.raises(ValueError, match='a ring of residue 0 shares atoms with another residue'):
        ll.from_residue(loose, 0, planes=True)
    loose.ring_atoms = [np.array([0, 1, 2], np.int32)]
    loose.amide_center, loose.amide_normal, loose.amide_res = np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.zeros(1, np.int32)
    loose.amide_atoms = np.array([[0, 1, 3, 2]], np.int32)
    with pytest.raises(ValueError, match='an amide of residue 0 shares atoms with another residue'):
        ll.from_residue(loose, 0, planes=True)
    loose.amide_atoms = np.array([[0, 1, 2, 3]], np.int32)           # only the fourth atom lies outside: it is not read, and becomes -1
    cut = ll.from_residue(loose, 0, planes=True)
    assert cut.n_rings == 1 and cut.amide_atoms.tolist() == [[0, 1, 2, -1]] and ll.from_residue(loose, 0).n_amides == 0
    both = ll.complex_of(rec, hem)
    n = rec.n_atoms
    assert both.n_rings == rec.n_rings + 4 and len(both.ring_atoms) == both.n_rings and both.n_amides == rec.n_amides
    assert all(np.array_equal(both.ring_atoms[rec.n_rings + q], hem.ring_atoms[q] + n) for q in range(4))
    assert all(np.array_equal(both.ring_atoms[k], rec.ring_atoms[k]) for k in range(rec.n_rings))
    aryl = synth.ligand('arylamide', 4)
    both = ll.complex_of(rec, aryl, aryl.xyz + 5.0)
    assert both.n_amides == rec.n_amides + 1 and both.amide_atoms[-1].tolist() == [n + 6, n + 7, n + 8, n] and both.amide_res[-1] == rec.n_residues
    assert np.array_equal(both.amide_atoms[:-1], rec.amide_atoms) and both.ring_res[-1] == rec.n_residues
    assert both.atom_name[n:] == aryl.atom_name and both.res_name[-1] == 'ARA' and both.rings_not_in_path_order() == []
    plain = ll.complex_of(rec, synth.ligand('amine', 3))
    assert plain.n_rings == rec.n_rings and np.array_equal(plain.amide_atoms, rec.amide_atoms)


def test_affected_rings_just_inside_and_just_outside_three_angstrom():
    rec = planes_cpu(receptor())
    r, c, n = _ring(rec, 'PHE', 2)
    c = rec.ring_center[r]
    far = np.array([[500.0, 0.0, 0.0]], np.float32)
    inside = (c + [0.0, 0.0, 3.0]).astype(np.float32)
    while poses._kd2(c[None], inside[None].astype(np.float64))[0, 0] > 9.0:
        inside[2] = np.nextafter(inside[2], np.float32(c[2]))
    outside = inside.copy()
    outside[2] = np.nextafter(inside[2], np.float32(1e9))
    assert poses._kd2(c[None], outside[None].astype(np.float64))[0, 0] > 9.0
    assert ll.affected_rings(rec, np.concatenate([far, inside[None]])).tolist() == [r]
    assert ll.affected_rings(rec, np.concatenate([far, outside[None]])).tolist() == []
    empty = copy.copy(rec)
    empty.ring_center, empty.ring_normal, empty.ring_res, empty.ring_atoms = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), []
    assert ll.affected_rings(empty, inside[None]).tolist() == []


def hand_planes():
    """Two ligands, poses 2 and 1, written by hand: global pose 0 has one record in every table, pose 2 two atom-plane records."""
    e = lambda n: {c: [] for c, _ in poses.plane_columns(n)}
    rows = [[dict(atom_plane=dict(atom=[540], ring=[2], dist=[3.5], theta=[12.0], mask=[1 | 4], ctype=[CT['INTER']]),
                  plane_plane=dict(bgn=[1], end=[9], dist=[4.0], dihedral=[5.0], theta_bgn=[10.0], theta_end=[np.nan], type1=[0], type2=[255], ctype=[CT['INTER']]),
                  group_group=dict(bgn=[39], end=[1], dist=[3.75], dihedral=[8.0], theta=[20.0], ctype=[CT['INTER']]),
                  group_plane=dict(amide=[39], ring=[2], dist=[4.25], dihedral=[9.0], theta=[21.0], ctype=[CT['INTER']])),
             dict(atom_plane=e('atom_plane'), plane_plane=e('plane_plane'), group_group=e('group_group'), group_plane=e('group_plane'))],
            [dict(atom_plane=dict(atom=[5, 533], ring=[9, 0], dist=[3.0, 5.5], theta=[1.0, 40.0], mask=[2, 16], ctype=[CT['INTER'], CT['INTER']]),
                  plane_plane=e('plane_plane'), group_group=e('group_group'), group_plane=e('group_plane'))]]
    rows = [[{n: {c: np.asarray(r[n][c], dt) for c, dt in poses.plane_columns(n)} for n in TABLES} for r in lig] for lig in rows]
    return rows, ll.planes_from_rows(rows)


def test_the_host_table_functions_on_a_hand_made_table(tmp_path):
    rows, t = hand_planes()
    assert t['ligand_pose_off'].tolist() == [0, 2, 3] and 'movable' not in t
    assert t['summary'][:, :4].tolist() == [[1, 1, 1, 1], [0, 0, 0, 0], [2, 0, 0, 0]] and t['summary'][:, 15].tolist() == [4, 0, 2]
    assert t['atom_plane']['pose_off'].tolist() == [0, 1, 1, 3] and t['group_group']['dist'].dtype == np.float32
    per = ll.split_planes(t)
    assert [len(p) for p in per] == [2, 1] and per[1][0]['atom_plane']['atom'].tolist() == [5, 533] and len(per[0][1]['plane_plane']['bgn']) == 0
    again = ll.concat_planes([ll.planes_from_rows([rows[0][:1], []]), ll.planes_from_rows([rows[0][1:], rows[1]])])
    assert differences(again, t) == []
    with pytest.raises(ValueError, match='not consecutive'):
        ll.concat_planes([ll.planes_from_rows([[], rows[1]]), ll.planes_from_rows([rows[0], []])])
    with pytest.raises(ValueError, match='different sizes'):
        ll.concat_planes([t, ll.planes_from_rows([rows[0]])])
    e = ll.empty_planes(2, [0, 2, 3])
    assert e['summary'].shape == (3, 16) and differences(ll.concat_planes([e]), e) == []
    rec = receptor()
    ligs = (synth.ligand('arylamide', 4), synth.ligand('halo', 6, planes=True))      # complex ids: atoms 532 + a, rings 9 + q, amide 39
    recs = ll.planes_to_records(t, rec, ligs)
    assert [(r['ligand'], r['pose']) for r in recs] == [(0, 0)] * 4 + [(1, 0)] * 2
    ap = next(r for r in recs if r['type'] == 'atom-plane')
    assert ap['contact'] == ['CARBONPI', 'DONORPI'] and ap['interacting_entities'] == 'INTER' and ap['distance'] == 3.5
    path = ll.write_library_planes(str(tmp_path), rec.id, t, rec, ligs)
    lines = open(path).read().splitlines()
    assert path.endswith('.libraryplanes') and lines[0] == ','.join(ll.PLANES_CSV_HEADER) and len(lines) == 7
    assert lines[1].split(',')[:5] == ['0', '0', 'atom-plane', 'L/1/O9', 'ring/2']          # atom 540 = the arylamide's atom 8
    assert lines[-1].split(',')[:5] == ['1', '0', 'atom-plane', 'L/1/C2', 'ring/0'] and lines[-1].split(',')[6:] == ['METSULPHURPI', 'INTER']


def test_the_new_synthetic_kinds_have_rings_along_their_bond_graph():
    assert synth.LIGAND_KINDS == ('water', 'ion', 'amine', 'halo', 'chain') and synth.PLANE_LIGAND_KINDS == ('arylamide', 'biaryl')
    assert [pc.id for pc in synth.ligands(5, seed=3)] == [synth.ligand(k, 3 + i, size=pc.n_atoms).id for i, (k, pc) in enumerate(zip(synth.LIGAND_KINDS, synth.ligands(5, seed=3)))]
    assert synth.ligand('halo', 4).n_rings == 0 and synth.ligand('halo', 4, planes=True).n_rings == 1
    for kind, rings, amides, S in (('arylamide', 1, 1, 16), ('biaryl', 2, 0, 22)):
        pc = synth.ligand(kind, 1)
        assert (pc.n_rings, pc.n_amides, pc.n_atoms) == (rings, amides, S) and pc.n_residues == 1
        for a in pc.ring_atoms:                                      # a cycle of the bond graph, listed along it
            a = [int(v) for v in a]
            assert len(a) == 6 and len(set(a)) == 6
            for k in range(6):
                assert a[(k + 1) % 6] in pc.bond_idx[pc.bond_off[a[k]]:pc.bond_off[a[k] + 1]].tolist()
            assert all(pc.type_mask[v] & T['aromatic'] for v in a)
        assert pc.rings_not_in_path_order() == []
        heavy = np.nonzero((pc.flags & config.F_HYDROGEN) == 0)[0]
        d = np.linalg.norm(pc.xyz[heavy][:, None].astype(np.float64) - pc.xyz[heavy][None], axis=2) + 9.0 * np.eye(len(heavy))
        assert d.min() > 1.2
        ll.pack([pc])
    ar = synth.ligand('arylamide', 1)
    n, c, o, ca = ar.amide_atoms[0]
    assert [ar.element[i] for i in (n, c, o, ca)] == ['N', 'C', 'O', 'C'] and ca in ar.ring_atoms[0].tolist()
    assert c in ar.bond_idx[ar.bond_off[n]:ar.bond_off[n + 1]] and o in ar.bond_idx[ar.bond_off[c]:ar.bond_off[c + 1]]
    nz = ar.atom_name.index('NZ')
    assert ar.type_mask[nz] & T['pos ionisable'] and ar.h_off[nz + 1] - ar.h_off[nz] == 3
    bi = synth.ligand('biaryl', 1)
    cl = bi.atom_name.index('CL1')
    assert bi.type_mask[cl] & T['xbond donor'] and bi.sb_nbr[cl] in bi.ring_atoms[1].tolist()
    assert abs(float(np.dot(_ring_normal(bi, 0), _ring_normal(bi, 1)))) < 0.9           # the second ring is twisted


def oracle_rows(rec, ligs, ps):
    """Per ligand, per pose: (the oracle's rows of the complex cut to the affected entities, the receptor rings taken over)."""
    home = planes_cpu(rec)
    out = []
    for lig, item in zip(ligs, ps):
        rows = []
        for p in range(0 if item is None else len(item[0])):
            q = planes_cpu(ll.complex_of(rec, lig, item[0][p], item[1][p]))
            oc = oracle.OracleComplex(q)
            oc.make_selection(_lig_mask(rec, lig))
            bags = dict(atom_plane=oc.atom_plane(), plane_plane=oc.plane_plane(), group_group=oc.group_group(), group_plane=oc.group_plane())
            rows.append((ll.plane_reference_rows(bags, home, lig, item[0][p]), int((q.ring_res[:rec.n_rings] != home.ring_res).sum())))
        out.append(rows)
    return out


def test_the_oracle_alone_meets_the_coverage_condition():
    s = dict(ap_lig_ring=0, ap_rec_ring=0, pp_lig_rec=0, pp_lig_lig=0, gg_lig_first=0, gg_rec_first=0, gp_lig_amide=0, gp_rec_amide=0, takeover=0)
    bits, cts = dict.fromkeys(('CARBONPI', 'CATIONPI', 'DONORPI', 'HALOGENPI'), 0), set()
    for rec, ligs, ps in (case_main(), case_docked()):
        nr, na = rec.n_rings, rec.n_amides
        for lig_rows in oracle_rows(rec, ligs, ps):
            for rows, taken in lig_rows:
                b = rows['atom_plane']
                s['ap_lig_ring'] += int((b['ring'] >= nr).sum())
                s['ap_rec_ring'] += int((b['ring'] < nr).sum())
                for name in bits:
                    bits[name] += int(((b['mask'] & AP[name]) != 0).sum())
                b = rows['plane_plane']
                s['pp_lig_rec'] += int(((b['bgn'] >= nr) != (b['end'] >= nr)).sum())
                s['pp_lig_lig'] += int(((b['bgn'] >= nr) & (b['end'] >= nr)).sum())
                b = rows['group_group']
                s['gg_lig_first'] += int(((b['bgn'] >= na) & (b['end'] < na)).sum())
                s['gg_rec_first'] += int(((b['bgn'] < na) & (b['end'] >= na)).sum())
                b = rows['group_plane']
                s['gp_lig_amide'] += int((b['amide'] >= na).sum())
                s['gp_rec_amide'] += int(((b['amide'] < na) & (b['ring'] >= nr)).sum())
                s['takeover'] += taken
                for name in TABLES:
                    cts |= set(rows[name]['ctype'].tolist())
    print(s, bits, cts)
    assert all(v > 0 for v in s.values()), s
    assert all(v > 0 for v in bits.values()), bits
    assert len(cts) >= 2


# ------------------------------------------------------------------------------------------------------------- yardsticks
def device_planes(pc):
    """``pc`` with the planes the device makes for its coordinates, as initialize() would leave them (one model of the topology)."""
    if pc.n_rings == 0 and pc.n_amides == 0:
        return pc
    ctx = _capi.Context(0)
    ctx.set_topology(pc)
    ctx.set_models(pc.xyz[None], pc.h_xyz[None])
    pl = ctx.models_planes()
    ctx.close()
    q = copy.copy(pc)
    q.ring_center, q.ring_normal, q.ring_res = pl['ring_center'][0], pl['ring_normal'][0], pl['ring_res'][0].astype(np.int32)
    q.amide_center, q.amide_normal = pl['amide_center'][0], pl['amide_normal'][0]
    return q


@functools.lru_cache(maxsize=None)
def receptor_gpu():
    return device_planes(receptor())


def definition_rows(rec_gpu, lig, x, h=None):
    """(B) for one pose: (rows, summary slots 12, 13, 14)."""
    both = device_planes(ll.complex_of(rec_gpu, lig, x, h))
    ctx = _capi.Context(0)
    ctx.set_complex(both)
    ctx.set_selection(_lig_mask(rec_gpu, lig))
    ctx.run_launch(5.0, 0.1, False)
    bags = {name: ctx.fetch_bag(name) for name in TABLES}
    ctx.close()
    nr = rec_gpu.n_rings
    near = ll.affected_rings(rec_gpu, x)
    aff = np.concatenate([near, np.arange(nr, both.n_rings)]).astype(np.int64)
    slots = (len(aff), int((both.ring_res[:nr] != rec_gpu.ring_res).sum()), int((both.ring_res[aff] < 0).sum()))
    # a receptor ring that is not affected keeps its residue
    keeps = np.ones(nr, bool)
    keeps[near] = False
    assert (both.ring_res[:nr][keeps] == rec_gpu.ring_res[keeps]).all()
    return ll.plane_reference_rows(bags, rec_gpu, lig, x), slots


def definition_table(rec_gpu, ligs, ps):
    rows, slots = [], []
    for lig, item in zip(ligs, ps):
        per = [definition_rows(rec_gpu, lig, item[0][p], item[1][p]) for p in range(0 if item is None else len(item[0]))]
        rows.append([r for r, _ in per])
        slots += [s for _, s in per]
    want = ll.planes_from_rows(rows)
    want['summary'][:, 12:15] = np.asarray(slots, np.uint32).reshape(-1, 3)
    return want


def differences(got, want, slots=tuple(range(16))):
    """The names of what differs: id, mask, class and type columns as integers, float columns as bytes, offsets, the summary."""
    bad = []
    for name in TABLES:
        for c, dt in poses.plane_columns(name):
            a, b = got[name][c], want[name][c]
            if a.dtype != dt or a.shape != b.shape or a.tobytes() != b.astype(dt).tobytes():
                bad.append(f'{name}.{c}')
        if not np.array_equal(got[name]['pose_off'], want[name]['pose_off']):
            bad.append(f'{name}.pose_off')
    s = list(slots)
    if got['summary'].shape != want['summary'].shape or not np.array_equal(got['summary'][:, s], want['summary'][:, s]):
        bad.append('summary')
    if not np.array_equal(got['ligand_pose_off'], want['ligand_pose_off']):
        bad.append('ligand_pose_off')
    return bad


def library_ctx(rec_gpu, ligs):
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)
    ctx.set_complex(rec_gpu)
    ctx.set_ligand_library(lib)
    ctx.set_ligand_library_planes(lib)
    return ctx, lib


def launch(ctx, lib, ps):
    off, x, _ = ll.flatten_poses(lib, ps)
    return ctx.library_planes(off, x)


def check_against_the_definition(rec, ligs, ps):
    """Launch, compare with (B) column by column, and check the canonical order; returns (ctx, got, want)."""
    rec_gpu = device_planes(rec)
    ctx, lib = library_ctx(rec_gpu, ligs)
    got = launch(ctx, lib, ps)
    want = definition_table(rec_gpu, ligs, ps)
    assert differences(got, want) == []
    for per in ll.split_planes(got):
        for bags in per:
            for name in TABLES:
                a, b = (bags[name][c].astype(np.int64) for c in poses.PLANE_ORDER[name])
                assert (np.diff(a << 32 | b) > 0).all()
    return ctx, got, want


@functools.lru_cache(maxsize=None)
def main_definition():
    rec, ligs, ps = case_main()
    return definition_table(receptor_gpu(), ligs, ps)


# ------------------------------------------------------------------------------------------------------------- GPU: parity
@pytest.mark.gpu
def test_main_case_equals_the_definition_and_the_pose_route():
    rec, ligs, ps = case_main()
    rec_gpu = receptor_gpu()
    ctx, lib = library_ctx(rec_gpu, ligs)
    got = launch(ctx, lib, ps)
    want = main_definition()
    assert differences(got, want) == []
    assert got['ligand_pose_off'].tolist() == [0, 3, 4, 7, 9, 14, 14, 16]
    info = ctx.library_planes_info()
    assert (info['ligands'], info['rings'], info['amides'], info['poses'], info['blocks']) == (7, 8, 1, 16, 16) and info['plane_table'] and info['setup']
    assert [info[n] for n in TABLES] == [len(got[n]['ctype']) for n in TABLES] and info['launches'] == 1
    assert all(len(got[n]['ctype']) > 0 for n in ('atom_plane', 'plane_plane', 'group_plane'))
    assert got['summary'][0, 13] == 1                                 # the water's first pose takes a ring over
    assert (got['summary'][:, 12] >= np.repeat([0, 0, 4, 0, 1, 2, 1], np.diff(got['ligand_pose_off']))).all()
    ctx.close()
    # (A) the pose route, ligand by ligand: the complex with the ligand's home 1 000 A away along x
    ref = _capi.Context(0)
    per = ll.split_planes(got)
    lo = got['ligand_pose_off']
    for l, (lig, item) in enumerate(zip(ligs, ps)):
        if item is None:
            continue
        home = device_planes(ll.complex_of(rec_gpu, lig, lig.xyz + np.array([1000.0, 0.0, 0.0], np.float32), lig.h_xyz + np.array([1000.0, 0.0, 0.0])))
        ref.set_complex(home)
        ref.set_selection(_lig_mask(rec_gpu, lig))
        ref.set_plane_atoms(home)
        t = ref.poses_planes(item[0])
        for p, bags in enumerate(poses.split_planes(t)):
            for name in TABLES:
                for c, dt in poses.plane_columns(name):
                    assert bags[name][c].tobytes() == per[l][p][name][c].tobytes(), (l, p, name, c)
        slots = list(range(13)) + [14, 15]                           # (slot 13 of the pose route also counts the ligand's own rings)
        assert np.array_equal(t['summary'][:, slots], got['summary'][lo[l]:lo[l + 1]][:, slots])
    ref.close()


@pytest.mark.gpu
def test_hand_docked_poses_equal_the_definition():
    rec, ligs, ps = case_docked()
    ctx, got, want = check_against_the_definition(rec, ligs, ps)
    nr, na = rec.n_rings, rec.n_amides
    ap, pp, gg, gp = (got[n] for n in TABLES)
    assert ((ap['ring'] >= nr) & (ap['atom'] < rec.n_atoms)).any() and ((ap['ring'] < nr) & (ap['atom'] >= rec.n_atoms)).any()
    assert all(((ap['mask'] & AP[n]) != 0).any() for n in ('CARBONPI', 'CATIONPI', 'DONORPI', 'HALOGENPI'))
    assert ((pp['bgn'] < nr) & (pp['end'] >= nr)).any() and ((pp['bgn'] >= nr) & (pp['end'] >= nr)).any()
    assert ((gg['bgn'] >= na) & (gg['end'] < na)).any() and ((gg['bgn'] < na) & (gg['end'] >= na)).any()
    assert (gp['amide'] >= na).any() and ((gp['amide'] < na) & (gp['ring'] >= nr)).any()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: seams
def benzene_receptor(extra=()):
    """Six carbons of one residue on a circle of 1.5 A in the plane z = 0 as a ring, and ``extra`` atoms of residues of their own."""
    ang = np.arange(6) * np.pi / 3.0
    ring = np.stack([1.5 * np.cos(ang), 1.5 * np.sin(ang), np.zeros(6)], axis=1)
    xyz = np.concatenate([ring, np.asarray(extra, np.float64).reshape(-1, 3)])
    pc = tiny_complex(list(xyz), res_id=[0] * 6 + list(range(1, 1 + len(extra))), bonds=[(k, (k + 1) % 6) for k in range(6)])
    pc.ring_atoms = [np.arange(6, dtype=np.int32)]
    pc.ring_center, pc.ring_normal = ref_py.ring_geometry(pc.xyz, pc.ring_atoms)
    pc.ring_res = np.array([0], np.int32)
    return pc


def _water_at(points):
    return [(np.asarray(points, np.float32).reshape(-1, 1, 3), np.zeros((len(points), 2, 3)))]


@pytest.mark.gpu
def test_three_angstrom_seam_take_over_and_release():
    rec = benzene_receptor(extra=[[30.0, 0.0, 0.0]])
    rec_gpu = device_planes(rec)
    c = rec_gpu.ring_center[0]
    kd2 = lambda p: float(poses._kd2(c[None], np.asarray(p, np.float32)[None].astype(np.float64))[0, 0])
    inside = (c + [0.0, 0.0, 3.0]).astype(np.float32)
    while kd2(inside) > 9.0:
        inside[2] = np.nextafter(inside[2], np.float32(0.0))
    outside = inside.copy()
    outside[2] = np.nextafter(inside[2], np.float32(9.0))
    assert kd2(inside) <= 9.0 < kd2(outside)
    # the nearest receptor atom of the centre by the residue search's distance; a ligand atom wins only when strictly nearer
    dist = lambda p: float(np.linalg.norm(np.asarray(p, np.float32).astype(np.float64) - c))
    nearest = min(dist(rec.xyz[k]) for k in range(6))
    takes = (c + [0.0, 0.0, nearest]).astype(np.float32)
    while dist(takes) >= nearest:
        takes[2] = np.nextafter(takes[2], np.float32(0.0))
    gives = takes.copy()
    gives[2] = np.nextafter(takes[2], np.float32(9.0))
    assert dist(takes) < nearest <= dist(gives)
    water = synth.ligand('water', 1)
    ctx, got, want = check_against_the_definition(rec, (water,), _water_at([inside, outside, takes, gives]))
    assert got['summary'][:, 12].tolist() == [1, 0, 1, 1] and got['summary'][:, 13].tolist() == [0, 0, 1, 0] and got['summary'][:, 14].tolist() == [0, 0, 0, 0]
    # taken over, the ring is the ligand's residue's: selected, so its records with the receptor's atoms are INTER
    ap = ll.split_planes(got)[0][2]['atom_plane']
    assert len(ap['atom']) > 0 and set(ap['ctype'][ap['atom'] < rec.n_atoms].tolist()) <= {CT['INTER']}
    ctx.close()


@pytest.mark.gpu
def test_a_spread_ligand_ring_has_no_residue_and_the_selection_plus_seam():
    # three carbons 3.5 A from their centre as a ligand 'ring': no atom within 3 A of the centre, 50 A from the receptor
    ang = np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
    tri = tiny_complex(list(3.5 * np.stack([np.cos(ang), np.sin(ang), np.zeros(3)], axis=1)), res_id=[0, 0, 0], bonds=[(0, 1), (1, 2), (2, 0)],
                       flags=config.F_ELEM_C)
    tri.ring_atoms = [np.arange(3, dtype=np.int32)]
    tri.ring_center, tri.ring_normal = ref_py.ring_geometry(tri.xyz, tri.ring_atoms)
    tri.ring_res = np.zeros(1, np.int32)
    rec = benzene_receptor(extra=[[30.0, 0.0, 0.0]])
    x = (tri.xyz.astype(np.float64) + [0.0, 0.0, 50.0]).astype(np.float32)
    near = (tri.xyz.astype(np.float64) + [0.0, 0.0, 1.0]).astype(np.float32)          # ... and 1 A above the receptor's ring: a receptor residue
    ctx, got, want = check_against_the_definition(rec, (tri,), [(np.stack([x, near]), np.zeros((2, 0, 3)))])
    # (its atoms stay sqrt(3.5^2 + 1) = 3.64 A from the receptor ring's centre: that ring is not affected)
    assert got['summary'][:, 12].tolist() == [1, 1] and got['summary'][:, 14].tolist() == [1, 0] and got['summary'][0, 15] == 0
    ctx.close()
    # a MET SD on the normal of a six-atom ligand ring: at 5.8 A the ring's atoms lie within 6 A of it (sqrt(5.8^2 + 1.39^2) < 6), at
    # 5.95 A only the centre does: the sulphur is not in selection_plus and there is no record
    met = tiny_complex([[0.0, 0.0, 0.0]], vdw=1.8, cov=1.05, type_mask=int(T['hbond acceptor']), flags=config.F_ELEM_S | config.F_RES_MET)
    halo = synth.ligand('halo', 6, planes=True)
    z = np.array([0.0, 0.0, 1.0])
    ps = tl._stack(place(halo, _ring_centre(halo), z, 5.8 * z, z), place(halo, _ring_centre(halo), z, 5.95 * z, z))
    for p in (0, 1):
        ringd = np.linalg.norm(ps[0][p][:6].astype(np.float64), axis=1)
        assert (ringd.min() < 6.0) == (p == 0) and np.linalg.norm(ps[0][p][:6].astype(np.float64).mean(axis=0)) < 6.0
    ctx, got, want = check_against_the_definition(met, (halo,), [ps])
    assert got['summary'][:, 0].tolist() == [1, 0] and got['atom_plane']['mask'].tolist() == [AP['METSULPHURPI']] and got['summary'][:, 12].tolist() == [1, 1]
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: shapes
@pytest.mark.gpu
def test_far_away_half_outside_the_box_and_one_pose():
    rec = receptor()
    aryl, biaryl = synth.ligand('arylamide', 4), synth.ligand('biaryl', 5)
    lo, hi = rec.xyz.min(axis=0).astype(np.float64), rec.xyz.max(axis=0).astype(np.float64)
    mid = (lo + hi) / 2.0
    faces = []
    for axis in range(3):
        for end in (lo, hi):
            at = mid.copy()
            at[axis] = end[axis]
            faces.append(place(biaryl, _ring_centre(biaryl, 0), [0.0, 0.0, 1.0], at, np.eye(3)[axis]))
    far = place(aryl, _ring_centre(aryl), [0.0, 0.0, 1.0], hi + 100.0, [0.0, 0.0, 1.0])
    ctx, got, want = check_against_the_definition(rec, (aryl, biaryl), [far, tl._stack(*faces)])
    assert got['summary'][0].tolist() == [0] * 12 + [1, 0, 0, 0] and (got['summary'][1:, 12] >= 2).all() and got['summary'][1:, 15].sum() > 0
    # T = 1: each pose alone is its rows of the joint launch
    lib = ll.pack((aryl, biaryl))
    one = ctx.library_planes(np.array([0, 0, 1]), faces[3][0])
    w = ll.planes_from_rows([[], [ll.split_planes(want)[1][3]]])
    w['summary'][:, 12:15] = want['summary'][4, 12:15]
    assert differences(one, w) == [] and ctx.library_planes_info()['poses'] == 1 and ctx.library_planes_info()['blocks'] == 1
    ctx.close()


@pytest.mark.gpu
def test_more_poses_than_blocks_mixing_one_atom_and_many():
    """1 029 poses of the one-atom water beside one arylamide pose: beyond the grid of blocks, S = 1 and S = 16 in one grid stride."""
    rec, rec_gpu = receptor(), receptor_gpu()
    water, aryl = synth.ligand('water', 1), synth.ligand('arylamide', 4)
    _, c0, n0 = _ring(rec, 'PHE', 0)
    _, c1, n1 = _ring(rec, 'PHE', 1)
    spots = np.stack([c0 + d * n0 for d in (0.5, 2.0, 2.9, 3.4, 4.4)] + [c1 - d * n1 for d in (1.0, 3.6)] + [c0 + 80.0]).astype(np.float32)
    rows_w = [definition_rows(rec_gpu, water, s[None]) for s in spots]
    xa, ha = place(aryl, _ring_centre(aryl), [0.0, 0.0, 1.0], c1 + 3.7 * n1, n1)
    row_a = definition_rows(rec_gpu, aryl, xa[0], ha[0])
    pick = np.arange(1029) % len(spots)
    ctx, lib = library_ctx(rec_gpu, (water, aryl))
    got = launch(ctx, lib, [(spots[pick][:, None, :], np.zeros((1029, 2, 3))), (xa, ha)])
    want = ll.planes_from_rows([[rows_w[k][0] for k in pick], [row_a[0]]])
    want['summary'][:, 12:15] = np.asarray([rows_w[k][1] for k in pick] + [row_a[1]], np.uint32)
    assert differences(got, want) == []
    info = ctx.library_planes_info()
    assert info['poses'] == 1030 and 0 < info['blocks'] < 1030 and got['summary'][-1, 15] > 0 and got['summary'][:-1, 15].sum() > 0
    ctx.close()


def crowd_receptor(n_rings, radius, seed=1):
    """``n_rings`` three-atom rings (every atom a residue of its own) whose centres lie within ``radius`` of the origin."""
    rs = np.random.RandomState(seed)
    ctr = rs.normal(size=(n_rings, 3))
    ctr *= (radius * rs.uniform(0.2, 1.0, n_rings) / np.linalg.norm(ctr, axis=1))[:, None]
    ang = np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
    xyz = []
    for k in range(n_rings):
        u = tl._unit(rs.normal(size=3))
        v = tl._unit(np.cross(u, rs.normal(size=3)))
        xyz += [ctr[k] + 0.8 * (np.cos(a) * u + np.sin(a) * v) for a in ang]
    pc = tiny_complex(xyz, flags=config.F_ELEM_C)
    pc.ring_atoms = [np.arange(3 * k, 3 * k + 3, dtype=np.int32) for k in range(n_rings)]
    pc.ring_center, pc.ring_normal = ref_py.ring_geometry(pc.xyz, pc.ring_atoms)
    pc.ring_res = ref_py.ring_residues(pc.xyz, pc.res_id, pc.ring_center)[0].astype(np.int32)
    return pc


@pytest.mark.gpu
def test_a_first_record_buffer_that_is_too_small_is_grown_and_the_launch_repeated():
    """150 receptor rings crowded around the ligand: every pose affects them all, and the pairs among them alone are 11 175
    plane-plane records a pose.  Eight poses outgrow the first buffer (65 536 records); one pose at a time does not."""
    rec_gpu = device_planes(crowd_receptor(150, 2.5))
    halo = synth.ligand('halo', 6, planes=True)
    x, h = synth.library_poses_of(rec_gpu, halo, np.zeros(3), 8, seed=2, shift=0.3)
    ctx, lib = library_ctx(rec_gpu, (halo,))
    before = ctx.library_planes_info()['launches']
    big = launch(ctx, lib, [(x, h)])
    k = int(big['summary'][:, 15].sum())
    assert k > max(1 << 16, 8 * 64) and ctx.library_planes_info()['launches'] == before + 2            # launched, grown, launched again
    assert (big['summary'][:, 12] == 151).all() and big['summary'][:, 15].max() <= 1 << 16
    parts = [launch(ctx, lib, [(x[p:p + 1], h[p:p + 1])]) for p in range(8)]
    assert ctx.library_planes_info()['launches'] == before + 10
    assert differences(ll.concat_planes(parts), big) == []
    first = definition_table(rec_gpu, (halo,), [(x[:1], h[:1])])                                       # ... and one of them against (B)
    assert differences(parts[0], first) == []
    ctx.close()


@pytest.mark.gpu
def test_null_columns_capacity_and_the_summary_alone():
    rec, ligs, ps = case_main()
    ctx, lib = library_ctx(receptor_gpu(), ligs)
    off, x, _ = ll.flatten_poses(lib, ps)
    t = ctx.library_planes(off, x)
    k = len(t['plane_plane']['bgn'])
    assert k > 1
    L, hd = ctx._L, ctx._h
    n = C.c_int64(0)
    e = np.full(k, -7, np.int32)
    rc = L.arp_library_planes_fetch(hd, 1, k - 1, None, None, _p(e), *([None] * 8), C.byref(n))
    assert rc == _capi.ARP_E_CAPACITY and n.value == k and (e == -7).all()            # the needed count, nothing written
    rc = L.arp_library_planes_fetch(hd, 1, k, None, None, _p(e), *([None] * 8), C.byref(n))
    assert rc == _capi.ARP_OK and n.value == k and np.array_equal(e, t['plane_plane']['end'])     # one column alone
    po = np.zeros(17, np.uint64)
    rc = L.arp_library_planes_fetch(hd, 3, 0, _p(po), *([None] * 10), C.byref(n))
    assert rc == _capi.ARP_OK and np.array_equal(po, t['group_plane']['pose_off'])    # no record asked for: cap is not looked at
    rc = L.arp_library_planes_fetch(hd, 2, 0, *([None] * 11), C.byref(n))
    assert rc == _capi.ARP_OK and n.value == len(t['group_group']['bgn'])             # every pointer NULL: the count
    buf = np.zeros(4096, np.float64)
    rc = L.arp_library_planes_fetch(hd, 0, 4096, None, None, None, None, None, _p(buf), None, None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_E_ARG and 'no such value column' in L.arp_last_error(hd).decode()
    rc = L.arp_library_planes_fetch(hd, 4, 0, *([None] * 11), C.byref(n))
    assert rc == _capi.ARP_E_ARG and 'table must be' in L.arp_last_error(hd).decode()
    s = ctx.library_planes_summary(off, x)
    assert s.dtype == np.uint32 and np.array_equal(s, t['summary']) and np.array_equal(s, main_definition()['summary'])
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: errors
def _fetch_fails(ctx):
    n = C.c_int64(0)
    s = np.zeros((2048, 16), np.uint32)
    rc = ctx._L.arp_library_planes_fetch(ctx._h, 0, 0, *([None] * 10), _p(s), C.byref(n))
    return rc == _capi.ARP_E_ARG


@pytest.mark.gpu
def test_non_finite_coordinates_are_found_on_the_device_and_leave_no_result():
    rec, ligs, ps = case_docked()
    ctx, lib = library_ctx(receptor_gpu(), ligs)
    off, x, _ = ll.flatten_poses(lib, ps)
    good = ctx.library_planes(off, x)
    for at, value in ((5, np.nan), (16 * 3 * 5 + 7, np.inf), (len(x) - 1, -np.inf)):
        bx = x.copy()
        bx[at] = value
        with pytest.raises(ValueError, match='non-finite'):
            ctx.library_planes(off, bx)
        assert _fetch_fails(ctx) and ctx.library_planes_info()['poses'] == 0
        assert differences(ctx.library_planes(off, x), good) == []
    with pytest.raises(ValueError):
        ctx.library_planes(off, x[:-3])                              # a refusal on the arguments leaves the resident result alone
    assert not _fetch_fails(ctx) and ctx.library_planes_info()['poses'] == 9
    ctx.close()


@pytest.mark.gpu
def test_more_near_rings_than_the_list_holds_fails_by_name():
    rec_gpu = device_planes(crowd_receptor(300, 1.5, seed=3))
    water = synth.ligand('water', 1)
    assert len(ll.affected_rings(rec_gpu, np.zeros((1, 3), np.float32))) == 300           # more than ARP_POSES_PLANES_MAX_NEAR = 256
    ctx, lib = library_ctx(rec_gpu, (water,))
    with pytest.raises(ValueError, match='ARP_POSES_PLANES_MAX_NEAR'):
        launch(ctx, lib, _water_at([[0.0, 0.0, 0.0]]))
    assert _fetch_fails(ctx)
    t = launch(ctx, lib, _water_at([[0.0, 0.0, 40.0]]))               # the same receptor from a distance is fine
    assert t['summary'][0].tolist() == [0] * 16
    ctx.close()


@pytest.mark.gpu
def test_every_host_refusal_names_its_cause_in_order():
    rec, ligs, ps = case_main()
    rec_gpu = receptor_gpu()
    lib = ll.pack(ligs)
    off, x, _ = ll.flatten_poses(lib, ps)
    ctx = _capi.Context(0)
    L, hd = ctx._L, ctx._h
    counts = np.zeros(4, np.int64)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    arrs = {k: i32(lib[k]) for k in ll.PLANE_ARRAYS}

    def set_planes(**change):
        a = dict(arrs)
        a.update(change)
        rc = L.arp_set_ligand_library_planes(hd, *[None if a[k] is None else _p(a[k]) for k in ll.PLANE_ARRAYS])
        return rc, L.arp_last_error(hd).decode()

    def launch_rc(pose_off=off, xs=x):
        rc = L.arp_library_planes_launch(hd, None if pose_off is None else _p(np.ascontiguousarray(pose_off, np.int64)), None if xs is None else _p(xs), _p(counts))
        return rc, L.arp_last_error(hd).decode()

    def refused(call, word, **kw):
        rc, msg = call(**kw)
        assert rc == _capi.ARP_E_ARG and word in msg, (word, rc, msg)
    # ---- the launch: the receptor's refusals first, then the library, the plane table, pose_off, xyz
    refused(launch_rc, 'no structure resident')
    refused(set_planes, 'no ligand library')
    ctx.set_complex(rec_gpu)
    refused(launch_rc, 'no ligand library')
    # a pass that has not been waited for comes first at both entry points: before 'no ligand library' ...
    m = np.zeros(rec.n_atoms, np.uint8)
    m[:10] = 1
    ctx.set_selection(m)
    ctx.run_enqueue(5.0, 0.1, False)
    refused(set_planes, 'not been waited for')
    refused(launch_rc, 'not been waited for')
    ctx.run_wait()
    refused(set_planes, 'no ligand library')
    ctx.set_ligand_library(lib)
    refused(launch_rc, 'no library plane table')
    # ---- the plane table, in its order
    refused(set_planes, 'an array is missing', ring_off=None)
    refused(set_planes, 'an array is missing', ring_atom_idx=None)
    refused(set_planes, 'an array is missing', amide_atoms=None)
    refused(set_planes, 'ring_off must start at 0', ring_off=arrs['ring_off'] + 1)
    refused(set_planes, 'ring_off must start at 0 and never decrease', ring_off=i32([0, 0, 0, 4, 3, 5, 7, 8]))
    refused(set_planes, 'ring_atom_off must start at 0 and never decrease', ring_atom_off=arrs['ring_atom_off'][::-1].copy())
    refused(set_planes, 'amide_off must start at 0 and never decrease', amide_off=i32([0, 0, 1, 0, 0, 1, 1, 1]))
    refused(set_planes, 'ARP_LIBRARY_PLANES_MAX_RINGS', ring_off=i32([0, 0, 0, 33, 33, 33, 33, 33]), ring_atom_off=np.arange(0, 100, 3, dtype=np.int32),
            ring_atom_idx=np.tile(i32([0, 1, 2]), 33))
    refused(set_planes, 'ARP_LIBRARY_PLANES_MAX_AMIDES', amide_off=i32([0, 0, 0, 33, 33, 33, 33, 33]), amide_atoms=np.tile(i32([0, 1, 2, -1]), (33, 1)))
    short = arrs['ring_atom_off'].copy()
    short[1:] -= 3
    refused(set_planes, 'at least three atoms', ring_atom_off=short, ring_atom_idx=arrs['ring_atom_idx'][3:].copy())
    idx = arrs['ring_atom_idx'].copy()
    idx[-1] = ligs[6].n_atoms
    refused(set_planes, 'ring atom index outside its own ligand', ring_atom_idx=idx)
    refused(set_planes, 'amide atom index outside its own ligand', amide_atoms=i32([[6, 7, -1, 0]]))
    refused(launch_rc, 'no library plane table')                     # none of them left a table behind
    # the Python layer checks the lengths the library cannot see
    with pytest.raises(ValueError, match='ring_off must be'):
        ctx.set_ligand_library_planes(dict(lib, ring_off=lib['ring_off'][:-1]))
    with pytest.raises(ValueError, match='ring_atom_idx must hold'):
        ctx.set_ligand_library_planes(dict(lib, ring_atom_idx=lib['ring_atom_idx'][:-1]))
    with pytest.raises(ValueError, match='amide_atoms must be'):
        ctx.set_ligand_library_planes(dict(lib, amide_atoms=np.zeros((2, 4), np.int32)))
    ctx.set_ligand_library_planes(lib)
    good = ctx.library_planes(off, x)
    contacts = ctx.library_contacts(*ll.flatten_poses(lib, ps))
    refused(set_planes, 'at least three atoms', ring_atom_off=short, ring_atom_idx=arrs['ring_atom_idx'][3:].copy())

    def resident_as_before():
        t = dict(good)
        n = C.c_int64(0)
        for q, name in enumerate(TABLES):
            tab, args = ctx._plane_table_buffers(name, len(good[name]['ctype']), 17)
            assert L.arp_library_planes_fetch(hd, q, len(good[name]['ctype']), _p(tab['pose_off']), *args, None, C.byref(n)) == _capi.ARP_OK
            t[name] = tab
        again = ctx._pose_records_fetch('arp_library_contacts_fetch', 'a', 16, len(contacts['i']))
        return differences(t, good) == [] and all(again[k].tobytes() == contacts[k].tobytes() for k in again)
    assert resident_as_before()                                      # a refused table leaves the resident one and the results alone
    # ... and, with everything resident, before every other cause; the resident results are as they were
    ctx.run_enqueue(5.0, 0.1, False)
    refused(set_planes, 'not been waited for', ring_off=None)
    refused(launch_rc, 'not been waited for', pose_off=None)
    ctx.run_wait()
    assert resident_as_before()
    # ---- the launch's own arguments
    refused(launch_rc, 'pose_off missing', pose_off=None)
    refused(launch_rc, 'pose_off must start at 0', pose_off=off + 1)
    down = off.copy()
    down[3] = down[2] - 1
    refused(launch_rc, 'pose_off must not decrease', pose_off=down)
    refused(launch_rc, 'ARP_POSES_MAX_POSES', pose_off=np.zeros(8, np.int64))
    refused(launch_rc, 'ARP_POSES_MAX_POSES', pose_off=np.concatenate([[0], np.full(7, (1 << 20) + 1)]))
    refused(launch_rc, 'xyz missing', xs=None)
    assert L.arp_library_planes_launch(hd, _p(off), _p(x), None) == _capi.ARP_E_ARG
    assert resident_as_before()
    with pytest.raises(ValueError, match='pose_off must be'):
        ctx.library_planes(off[:-1], x)
    with pytest.raises(ValueError, match='xyz must hold'):
        ctx.library_planes(off, x[:-3])
    assert resident_as_before()
    # ---- a batch, models, shard ownership: the receptor's refusals come before the library's
    ctx.set_batch([rec_gpu, rec_gpu], [m, m])
    refused(launch_rc, 'batch')
    ctx.set_topology(rec)
    ctx.set_models(np.stack([rec.xyz, rec.xyz]), np.stack([rec.h_xyz, rec.h_xyz]))
    refused(launch_rc, 'models')
    ctx.set_complex(rec_gpu)
    ctx._check(L.arp_set_ownership(hd, _p(np.ones(rec.n_atoms, np.uint8)), _p(np.arange(rec.n_atoms, dtype=np.int32))), 'arp_set_ownership')
    refused(launch_rc, 'shard')
    ctx.close()
    # a receptor uploaded without arp_set_residues: the ligand's residue, the receptor's residue count, would be residue 0 of its atoms
    bare = _capi.Context(0)
    bare._check(L.arp_set_atoms(bare._h, rec.n_atoms, _p(rec.xyz), _p(rec.vdw), _p(rec.cov), _p(rec.type_mask), _p(rec.flags), _p(np.zeros(rec.n_atoms, np.int32))),
                'arp_set_atoms')
    bare.set_ligand_library(lib)
    bare.set_ligand_library_planes(lib)
    rc = L.arp_library_planes_launch(bare._h, _p(off), _p(x), _p(counts))
    assert rc == _capi.ARP_E_ARG and 'no residue table resident' in L.arp_last_error(bare._h).decode()
    bare.close()


def bare_atoms(n):
    """``n`` atoms of one residue scattered over a 300 A box: no bonds, hydrogens, rings or amides."""
    from arpeggio_amd.core.packed import PackedComplex
    rs = np.random.RandomState(7)
    return PackedComplex(xyz=(300.0 * rs.random_sample((n, 3))).astype(np.float32), vdw=np.full(n, 1.7), cov=np.full(n, 0.76), type_mask=np.zeros(n, np.uint16),
                         flags=np.zeros(n, np.uint16), res_id=np.zeros(n, np.int32), res_flags=[0], res_prev=[-1], res_next=[-1], bond_off=np.zeros(n + 1, np.int32),
                         bond_idx=np.zeros(0, np.int32), h_off=np.zeros(n + 1, np.int32), h_xyz=np.zeros((0, 3)), sb_nbr=np.full(n, -1, np.int32),
                         ring_center=np.zeros((0, 3)), ring_normal=np.zeros((0, 3)), ring_res=np.zeros(0, np.int32), id='bare')


@pytest.mark.gpu
def test_a_receptor_whose_complex_outgrows_the_sort_key_is_refused_before_the_library_is_looked_at():
    """The second launch refusal: n + ARP_LIBRARY_MAX_ATOMS = 256 not below 2^21.  It is host arithmetic in front of any kernel: a
    receptor of 2^21 - 256 bare atoms meets it, one atom fewer passes it and meets the next cause (no library is resident)."""
    ctx = _capi.Context(0)
    L, hd = ctx._L, ctx._h
    counts = np.zeros(4, np.int64)
    off, x = np.array([0, 1], np.int64), np.zeros(3, np.float32)
    for n, word in (((1 << 21) - 256, '2^21 atoms, rings or amides of the complex'), ((1 << 21) - 257, 'no ligand library')):
        ctx.set_complex(bare_atoms(n))
        rc = L.arp_library_planes_launch(hd, _p(off), _p(x), _p(counts))
        assert rc == _capi.ARP_E_ARG and word in L.arp_last_error(hd).decode(), (n, L.arp_last_error(hd).decode())
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
@pytest.mark.gpu
def test_making_the_result_voids_nothing_and_it_goes_with_what_it_reads():
    rec, ligs, ps = case_main()
    rec_gpu = receptor_gpu()
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    want = main_definition()
    ctx = _capi.Context(0)
    ctx.set_complex(rec_gpu)
    hem = np.nonzero(rec.res_id == int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]))[0]
    m = np.zeros(rec.n_atoms, np.uint8)
    m[hem] = 1
    ctx.set_selection(m)
    ctx.set_plane_atoms(rec_gpu)
    counts = ctx.run_launch(5.0, 0.1, False)
    px, ph = synth.poses_of(rec, hem, 6, seed=11, shift=2.0)
    pc_t = ctx.poses_contacts(px, ph, 5.0, 0.1, False)
    pp_t = ctx.poses_planes(px)
    ctx.set_ligand_library(lib)
    lc_t = ctx.library_contacts(off, x, h, 5.0, 0.1, False)
    ctx.library_best(np.arange(16, dtype=np.int64) - 4)
    refs = lfp.references([lfp.reference_from_pose(lc_t, 0, rec.res_id, level='residue')])
    ctx.library_fingerprints(refs, 0x7FFF, bits=True)
    L, hd = ctx._L, ctx._h

    def everything():
        n = C.c_int64(0)
        best = dict(n_poses=np.empty(7, np.int64), best_pose=np.empty(7, np.int32), score=np.empty(7, np.int64))
        ctx._check(L.arp_library_best_fetch(hd, 7, _p(best['n_poses']), _p(best['best_pose']), _p(best['score']), C.byref(n)), 'best')
        planes = []
        for q, name in enumerate(TABLES):
            tab, args = ctx._plane_table_buffers(name, len(pp_t[name]['ctype']), 7)
            ctx._check(L.arp_poses_planes_fetch(hd, q, len(pp_t[name]['ctype']), _p(tab['pose_off']), *args, None, C.byref(n)), 'planes')
            planes.append(tab)
        info = ctx.library_fingerprints_info()
        fpc, fpx = np.empty(info['rows'], np.uint32), np.empty((info['rows'], info['n_refs']), np.uint32)
        ctx._check(L.arp_library_fingerprints_fetch(hd, 0, None, _p(fpc), _p(fpx), None, None, C.byref(n)), 'fp')
        return (tl._fetch_everything(ctx), ctx._pose_records_fetch('arp_poses_contacts_fetch', 'j', 6, len(pc_t['i'])), planes,
                ctx._pose_records_fetch('arp_library_contacts_fetch', 'a', 16, len(lc_t['i'])), best, fpc, fpx)
    before = everything()
    ctx.set_ligand_library_planes(lib)
    assert tl._same_bytes(everything(), before)
    got = ctx.library_planes(off, x)
    assert differences(got, want) == [] and tl._same_bytes(everything(), before)
    # alternating with the contacts at another cutoff stays exact on both sides
    c4 = ctx.library_contacts(off, x, h, 4.0, 0.1, False)
    for _ in range(2):
        assert differences(ctx.library_planes(off, x), want) == []
        assert tl.differences(ctx.library_contacts(off, x, h, 4.0, 0.1, False), c4) == []
    assert ctx.run_launch(5.0, 0.1, False) == counts and differences(ctx.library_planes(off, x), want) == []
    # the result survives a new selection; it goes with the plane table, the library, models and a new structure
    ctx.set_selection(m)
    assert not _fetch_fails(ctx)
    ctx.set_ligand_library_planes(lib)
    assert _fetch_fails(ctx) and ctx.library_planes_info()['poses'] == 0 and ctx.library_planes_info()['plane_table']
    assert differences(ctx.library_planes(off, x), want) == []
    ctx.set_ligand_library(lib)
    assert _fetch_fails(ctx) and not ctx.library_planes_info()['plane_table']
    with pytest.raises(ValueError, match='no library plane table'):
        ctx.library_planes(off, x)
    ctx.set_ligand_library_planes(lib)
    assert differences(ctx.library_planes(off, x), want) == []
    ctx.set_topology(rec)
    assert not _fetch_fails(ctx)                                     # (the kept topology is not the resident structure)
    ctx.set_models(np.stack([rec.xyz, rec.xyz]), np.stack([rec.h_xyz, rec.h_xyz]))
    assert _fetch_fails(ctx)
    ctx.set_complex(rec_gpu)
    assert _fetch_fails(ctx) and ctx.library_planes_info()['plane_table'] and not ctx.library_planes_info()['setup']
    assert differences(ctx.library_planes(off, x), want) == []       # the library and its plane table stayed resident
    ctx.set_complex(rec_gpu)
    assert _fetch_fails(ctx)
    ctx.close()


@pytest.mark.gpu
def test_the_same_library_against_a_second_receptor_and_a_caller_owned_stream():
    from test_gpu_paths import _hip_runtime
    rec, ligs, ps = case_main()
    lib = ll.pack(ligs)
    off, x, _ = ll.flatten_poses(lib, ps)
    ctx, _ = library_ctx(receptor_gpu(), ligs)
    assert differences(ctx.library_planes(off, x), main_definition()) == []
    other_gpu = device_planes(second_receptor())                    # another protein in the same place: the library and its table stay
    ctx.set_complex(other_gpu)
    got = ctx.library_planes(off, x)
    assert differences(got, definition_table(other_gpu, ligs, ps)) == [] and got['summary'][:, 15].sum() > 0
    # a caller-owned stream
    ctx.set_complex(receptor_gpu())
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    assert differences(ctx.library_planes(off, x), main_definition()) == []
    assert np.array_equal(ctx.library_planes_summary(off, x), main_definition()['summary'])
    ctx.use_stream(0)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------------------------------------------------- GPU: host-level routes
@pytest.mark.gpu
def test_run_ligand_library_with_planes_chunked_and_the_csv(tmp_path):
    rec, ligs, ps = case_main()
    ic = InteractionComplex(copy.copy(receptor_gpu()))
    plain = ic.run_ligand_library(ligs, ps, 5.0, 0.1, False)
    assert getattr(ic, 'library_planes', None) is None
    with pytest.raises(AttributeError):
        ic.write_library_planes(str(tmp_path))
    whole = ic.run_ligand_library(ligs, ps, 5.0, 0.1, False, planes=True)
    assert tl.differences(whole, plain) == [] and differences(ic.library_planes, main_definition()) == []
    chunked = ic.run_ligand_library(ligs, ps, 5.0, 0.1, False, chunk=4, planes=True)
    assert tl.differences(chunked, plain) == [] and differences(ic.library_planes, main_definition()) == []
    path = ic.write_library_planes(str(tmp_path))
    lines = open(path).read().splitlines()
    t = ic.library_planes
    assert path.endswith('.libraryplanes') and lines[0] == ','.join(ll.PLANES_CSV_HEADER) and len(lines) == 1 + int(t['summary'][:, 15].sum())
    assert [ln.split(',')[2] for ln in lines[1:]].count('plane-plane') == len(t['plane_plane']['bgn'])
    recs = ll.planes_to_records(t, ic.pc, ligs)
    assert len(recs) == len(lines) - 1 and {r['ligand'] for r in recs} <= {0, 1, 2, 3, 4, 6}
    # without planes: the contacts are unchanged, and the planes of the run before do not stay behind for the next writer
    again = ic.run_ligand_library(ligs[:5], ps[:5], 5.0, 0.1, False, chunk=4)
    assert tl.differences(again, ic.run_ligand_library(ligs[:5], ps[:5], 5.0, 0.1, False)) == [] and ic.library_planes is None
    with pytest.raises(AttributeError):
        ic.write_library_planes(str(tmp_path))
