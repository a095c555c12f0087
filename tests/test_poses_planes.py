"""Ligand poses on a resident receptor, ring and amide contacts (arp_set_plane_atoms, arp_poses_planes_launch / _fetch / _info,
Context.poses_planes / poses_planes_summary, InteractionComplex.run_poses(planes=True), arpeggio_amd.poses).

The yardstick is the ensemble route, which the new code does not touch: ``EnsembleComplex`` on ``poses.as_models(...)`` evaluates
every pose as a whole model — ring and amide geometry and ring residues made on the device per model, each model's four bags
pinned to its single run and to the oracle by tests/test_models.py —; of each model's bags the rows that involve an affected
entity (``poses.plane_reference_rows``) are what the pose must give.  The resident structure is the HOME pack: the same pack with
the planes the device makes for the resident coordinates, as initialize() would leave them.  Every comparison is exact: ids,
masks, classes and contact types as integers, every float column as bytes.  No tolerance anywhere, no time asserted.

On the CPU the oracle stands in, fed ``ref_py.ring_geometry``, ``ref_py.ring_residues`` and ``ref_py.amide_geometry`` per pose;
it is used for counts and classes only.  The counts it gives (records with an affected entity, over all poses):
HEM 290 atom_plane (INTER, INTRA_SELECTION, INTRA_BINDING_SITE), 146 plane_plane (47 affected x unaffected, 99 both affected), 29
group_plane (all unmoved amide x moved ring); LYS 14 group_group, 2 atom_plane of a movable atom with an unaffected ring, 2
take-overs; water 3 such atom_plane records, 2 take-overs; PHE 19 INTER group_group and 4 group_plane with a moved amide."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from oracle import ref_py
from arpeggio_amd import _capi, poses, synth
from arpeggio_amd.core import config, utils
from arpeggio_amd.core.interactions import EnsembleComplex, InteractionComplex
from helpers import concat_packs, tiny_complex
import test_poses as tp

CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
PARAMS = (5.0, 0.1, False)


# ------------------------------------------------------------------------------------------------------------- cases
def case_phe():
    """The mid-chain PHE, residue 10: a moved ring and two amides shared with the neighbours."""
    pc = tp.protein()
    assert pc.res_name[10] == 'PHE' and pc.res_prev[10] == 9 and pc.res_next[10] == 11
    idx = utils.selection_parser([tp._residue_selector(pc, 10)], pc)
    x, h = synth.poses_of(pc, idx, 48, seed=3, shift=4.0, jitter=0.1)
    return pc, idx, x, h


def _water_atoms(pc):
    idx = np.nonzero(pc.res_id == tp.water_residue(pc))[0]
    o = next(int(a) for a in idx if not pc.flags[a] & config.F_HYDROGEN)
    return idx, o


def _phe_ring(pc, skip_res=()):
    """A six-ring of a receptor PHE and its centre and unit normal (float64 of the float32 atoms)."""
    r = next(k for k in range(pc.n_rings) if pc.res_name[int(pc.res_id[pc.ring_atoms[k][0]])] == 'PHE' and int(pc.res_id[pc.ring_atoms[k][0]]) not in skip_res)
    c, n = ref_py.ring_geometry(pc.xyz, [pc.ring_atoms[r]])
    return r, c[0], n[0]


def case_takeover():
    """The water, by hand: pose 0 puts its O 0.5 A above the centre of a receptor PHE ring (it becomes the ring's residue),
    pose 1 leaves it at home."""
    pc = tp.protein()
    idx, o = _water_atoms(pc)
    r, c, n = _phe_ring(pc)
    x0 = pc.xyz[idx].astype(np.float64)
    d = c + 0.5 * n - pc.xyz[o].astype(np.float64)
    h0 = pc.h_xyz[poses.movable(pc, idx)[1]]
    return pc, idx, np.stack([(x0 + d).astype(np.float32), x0.astype(np.float32)]), np.stack([h0 + d, h0]), r


@functools.lru_cache(maxsize=None)
def release_pack():
    """A copy of the pack in which that water sits above the ring AT HOME."""
    pc, idx, x, h, r = case_takeover()
    q = copy.copy(pc)
    q.xyz = pc.xyz.copy()
    q.xyz[idx] = x[0]
    q.h_xyz = pc.h_xyz.copy()
    q.h_xyz[poses.movable(pc, idx)[1]] = h[0]
    return q, r


def case_release():
    pc, r = release_pack()
    idx, _ = _water_atoms(tp.protein())
    x, h = synth.poses_of(pc, idx, 6, seed=4, shift=6.0, jitter=0.0)
    return pc, idx, x, h


@functools.lru_cache(maxsize=None)
def triangle_pack():
    """The small protein with three hand-made carbon atoms, one residue, that form a 'ring' spread beyond 3 A: every atom of
    the triangle is 3.5 A from its centre."""
    pc = tp.protein()
    ang = np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
    far = pc.xyz.max(axis=0).astype(np.float64) + 30.0
    tri = far + 3.5 * np.stack([np.cos(ang), np.sin(ang), np.zeros(3)], axis=1)
    q = tiny_complex(list(tri), vdw=1.7, cov=0.76, type_mask=0)
    both = concat_packs(pc, q)
    n = pc.n_atoms
    both.ring_atoms = list(pc.ring_atoms) + [np.array([n, n + 1, n + 2], np.int32)]
    both.amide_atoms = pc.amide_atoms
    c, nv = ref_py.ring_geometry(both.xyz, [both.ring_atoms[-1]])
    both.ring_center = np.concatenate([pc.ring_center, c])
    both.ring_normal = np.concatenate([pc.ring_normal, nv])
    both.ring_res = np.concatenate([pc.ring_res, [-1]]).astype(np.int32)
    return both


def case_triangle():
    """Pose 0: the triangle's centre 1 A from a receptor carbon (the ring's residue is the receptor's, not the ligand's);
    pose 1: 100 A away (no atom within 3 A: residue -1); pose 2: home (likewise -1)."""
    pc = triangle_pack()
    n = tp.protein().n_atoms
    idx = np.arange(n, n + 3)
    x0 = pc.xyz[idx].astype(np.float64)
    c = x0.mean(axis=0)
    r, rc, rn = _phe_ring(tp.protein())
    target = pc.xyz[int(pc.ring_atoms[r][0])].astype(np.float64) + np.array([0.0, 0.0, 1.0])
    x = np.stack([(x0 + (target - c)).astype(np.float32), (x0 + 100.0).astype(np.float32), x0.astype(np.float32)])
    return pc, idx, x, np.zeros((3, 0, 3))


CASES = dict(main=tp.case_main, lys=tp.case_lys, phe=case_phe, water=tp.case_water, two=tp.case_two_residues, spread=tp.case_spread,
             seams=tp.case_seams, takeover=lambda: case_takeover()[:4], release=case_release, triangle=case_triangle)


# ------------------------------------------------------------------------------------------------------------- yardsticks
def home_pack_cpu(pc):
    """``pc`` with the planes initialize() makes for its coordinates (ref_py)."""
    q = copy.copy(pc)
    q.ring_center, q.ring_normal = ref_py.ring_geometry(pc.xyz, pc.ring_atoms)
    q.ring_res = ref_py.ring_residues(pc.xyz, pc.res_id, q.ring_center)[0]
    q.amide_center, q.amide_normal = ref_py.amide_geometry(pc.xyz, pc.amide_atoms)
    return q


def oracle_bags(pc, m):
    oc = oracle.OracleComplex(pc)
    oc.make_selection(m)
    return dict(atom_plane=oc.atom_plane(), plane_plane=oc.plane_plane(), group_group=oc.group_group(), group_plane=oc.group_plane())


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """Per pose of a case: (reference rows, moved amides, affected rings, posed ring residues), and the home pack."""
    pc, idx, x, h = CASES[name]()
    home = home_pack_cpu(pc)
    X, H = poses.as_models(pc, idx, x, h)
    m = tp._mask(pc, idx)
    out = []
    for p in range(len(X)):
        q = home_pack_cpu(tp.pose_pack(pc, X, H, p))
        moved, rings = poses.affected(home, idx, x[p])
        out.append((poses.plane_reference_rows(oracle_bags(q, m), home, idx, x[p]), moved, rings, q.ring_res))
    return out, home


@functools.lru_cache(maxsize=None)
def home_pack_gpu(name):
    """The case's pack with the planes the device makes for its resident coordinates (one model of the topology)."""
    pc = CASES[name]()[0]
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
def ensemble_table(name):
    """The table the device must return for a case: the ensemble route's bags of every pose, cut to the affected rows."""
    pc, idx, x, h = CASES[name]()
    home = home_pack_gpu(name)
    X, H = poses.as_models(pc, idx, x, h)
    ens = EnsembleComplex((copy.copy(pc), X, H))
    ens.run_arpeggio(np.asarray(idx), *PARAMS)
    rows = [poses.plane_reference_rows(ens._results[f]['bags'], home, idx, x[f]) for f in range(len(X))]
    ens._ctx.close()
    want = poses.planes_from_rows(rows, idx)
    want['summary'][:, 12] = [len(poses.affected(home, idx, x[f])[1]) for f in range(len(X))]
    return want


def differences(got, want, rings=True):
    """The names of what differs: id, mask, class and type columns as integers, float columns as bytes, offsets, and the summary
    (slots 13 and 14 are checked where a test knows them)."""
    bad = []
    for name in poses.PLANE_TABLES:
        for c, dt in poses.plane_columns(name):
            a, b = got[name][c], want[name][c]
            if a.dtype != dt or a.shape != b.shape or a.tobytes() != b.astype(dt).tobytes():
                bad.append(f'{name}.{c}')
        if not np.array_equal(got[name]['pose_off'], want[name]['pose_off']):
            bad.append(f'{name}.pose_off')
    slots = list(range(12)) + ([12] if rings else []) + [15]
    if got['summary'].shape != want['summary'].shape or not np.array_equal(got['summary'][:, slots], want['summary'][:, slots]):
        bad.append('summary')
    if not np.array_equal(got['movable'], want['movable']):
        bad.append('movable')
    return bad


def _ctx(pc, idx):
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(tp._mask(pc, idx))
    ctx.set_plane_atoms(pc)
    return ctx


def device_case(name):
    pc, idx, x, h = CASES[name]()
    ctx = _ctx(home_pack_gpu(name), idx)
    got = ctx.poses_planes(x)
    return ctx, got, ensemble_table(name)


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_planes():
    """Two poses written by hand: pose 0 has one record in every table, pose 1 two atom-plane records."""
    rows = [dict(atom_plane=dict(atom=[7], ring=[2], dist=[3.5], theta=[12.0], mask=[1 | 4], ctype=[CT['INTER']]),
                 plane_plane=dict(bgn=[1], end=[2], dist=[4.0], dihedral=[5.0], theta_bgn=[10.0], theta_end=[np.nan], type1=[0], type2=[255], ctype=[CT['INTER']]),
                 group_group=dict(bgn=[3], end=[1], dist=[3.75], dihedral=[8.0], theta=[20.0], ctype=[CT['INTRA_SELECTION']]),
                 group_plane=dict(amide=[3], ring=[2], dist=[4.25], dihedral=[9.0], theta=[21.0], ctype=[CT['INTER']])),
            dict(atom_plane=dict(atom=[5, 9], ring=[0, 0], dist=[3.0, 5.5], theta=[1.0, 40.0], mask=[2, 16], ctype=[CT['INTER'], CT['INTRA_BINDING_SITE']]),
                 plane_plane={c: [] for c, _ in poses.plane_columns('plane_plane')}, group_group={c: [] for c, _ in poses.plane_columns('group_group')},
                 group_plane={c: [] for c, _ in poses.plane_columns('group_plane')})]
    rows = [{n: {c: np.asarray(r[n][c], dt) for c, dt in poses.plane_columns(n)} for n in poses.PLANE_TABLES} for r in rows]
    return rows, poses.planes_from_rows(rows, [5, 7])


def test_the_host_functions_on_a_hand_made_table(tmp_path):
    rows, t = hand_planes()
    assert t['summary'].tolist() == [[1, 1, 1, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 4], [2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2]]
    assert t['atom_plane']['pose_off'].tolist() == [0, 1, 3] and t['group_plane']['pose_off'].tolist() == [0, 1, 1]
    assert t['group_group']['dist'].dtype == np.float32 and t['plane_plane']['theta_end'].dtype == np.float64
    per = poses.split_planes(t)
    assert len(per) == 2 and per[1]['atom_plane']['atom'].tolist() == [5, 9] and len(per[1]['plane_plane']['bgn']) == 0
    again = poses.concat_planes([poses.planes_from_rows(rows[:1], [5, 7]), poses.planes_from_rows(rows[1:], [5, 7])])
    assert differences(again, t) == []
    with pytest.raises(ValueError):
        poses.concat_planes([poses.planes_from_rows(rows[:1], [5, 7]), poses.planes_from_rows(rows[1:], [5, 8])])
    e = poses.empty_planes(3, [1])
    assert differences(poses.concat_planes([e]), e) == [] and e['summary'].shape == (3, 16)
    pc = tp.protein()
    recs = poses.planes_to_records(t, pc)
    assert [r['pose'] for r in recs] == [0, 0, 0, 0, 1, 1] and sorted(r['type'] for r in recs[:4]) == ['atom-plane', 'group-group', 'group-plane', 'plane-plane']
    ap = next(r for r in recs if r['type'] == 'atom-plane')
    assert ap['contact'] == ['CARBONPI', 'DONORPI'] and ap['interacting_entities'] == 'INTER' and ap['distance'] == 3.5
    path = poses.write_pose_planes(str(tmp_path), pc.id, t, pc)
    lines = open(path).read().splitlines()
    assert path.endswith('proteinlike.poseplanes') and lines[0] == ','.join(poses.PLANES_CSV_HEADER) and len(lines) == 7
    assert lines[1].split(',')[:4] == ['0', 'atom-plane', 'A/%d/%s' % (pc.res_seq[pc.res_id[7]], pc.atom_name[7]), 'ring/2']
    assert lines[-1].split(',')[5:] == ['METSULPHURPI', 'INTRA_BINDING_SITE']


def test_affected_just_inside_and_just_outside_three_angstrom():
    """One benzene-like ring of six atoms and two free atoms; the distances are exact in float32 and float64."""
    ang = np.arange(6) * np.pi / 3.0
    ring = np.stack([1.5 * np.cos(ang), 1.5 * np.sin(ang), np.zeros(6)], axis=1).astype(np.float32)
    free = np.array([[0.0, 0.0, 8.0], [20.0, 0.0, 0.0]], np.float32)
    pc = tiny_complex(list(np.concatenate([ring, free]).astype(np.float64)), res_id=[0] * 6 + [1, 2])
    pc.ring_atoms = [np.arange(6, dtype=np.int32)]
    pc.ring_center, pc.ring_normal = ref_py.ring_geometry(pc.xyz, pc.ring_atoms)
    pc.ring_res = np.array([0], np.int32)
    c = pc.ring_center[0]
    sel = np.array([6])
    at = lambda z: (c + np.array([0.0, 0.0, z])).astype(np.float32)[None]
    inside, outside = np.float32(3.0), np.nextafter(np.float32(3.0), np.float32(4.0))
    assert (np.float64(at(inside)[0, 2]) - c[2]) ** 2 <= 9.0 < (np.float64(at(outside)[0, 2]) - c[2]) ** 2
    assert poses.affected(pc, sel, at(inside))[1].tolist() == [0]             # 3.0 A in the pose: inclusive
    assert poses.affected(pc, sel, at(outside))[1].tolist() == []             # one float32 step further: not
    # ... at home: the same atom resident at 3.0 A is affected wherever the pose puts it
    q = copy.copy(pc)
    q.xyz = pc.xyz.copy()
    q.xyz[6] = at(inside)[0]
    assert poses.affected(q, sel, at(50.0))[1].tolist() == [0]
    q.xyz[6] = at(outside)[0]
    assert poses.affected(q, sel, at(50.0))[1].tolist() == []
    # an atom of the path moves: affected at any distance; no amides here
    moved, rings = poses.affected(pc, np.array([2]), (pc.xyz[2] + 30.0)[None])
    assert rings.tolist() == [0] and moved.tolist() == []
    with pytest.raises(ValueError):
        poses.affected(pc, sel, np.zeros((2, 3)))
    # amides: moved by N, C or O, not by the C-alpha
    prot = tp.protein()
    a = prot.amide_atoms[3]
    for k in range(3):
        assert 3 in poses.affected(prot, np.array([a[k]]), prot.xyz[a[k]][None])[0].tolist()
    others = set(prot.amide_atoms[:, :3].ravel().tolist())
    if int(a[3]) not in others:
        assert poses.affected(prot, np.array([a[3]]), prot.xyz[a[3]][None])[0].tolist() == []


def test_the_oracle_alone_meets_the_coverage_condition():
    """Every kind of record the feature must get right occurs in the cases, asserted of the oracle's rows: each table, each
    orientation of each loop, several contact types per ring table, and ring residues taken over by a pose."""
    seen = {}
    for name in ('main', 'lys', 'water', 'phe'):
        per, home = oracle_case(name)
        pc, idx, x, h = CASES[name]()
        m = tp._mask(pc, idx).astype(bool)
        has = np.array([bool(m[a].any()) for a in pc.ring_atoms])
        s = dict(ap=0, ap_movable_unaffected=0, pp_mixed=0, pp_both=0, gg=0, gg_inter=0, gp=0, gp_unmoved=0, gp_moved=0, takeover=0, ap_ct=set(), pp_ct=set())
        for rows, moved, rings, posed_res in per:
            rg = np.zeros(pc.n_rings, bool)
            rg[rings] = True
            am = np.zeros(pc.n_amides, bool)
            am[moved] = True
            b = rows['atom_plane']
            s['ap'] += len(b['atom'])
            s['ap_movable_unaffected'] += int((m[b['atom']] & ~rg[b['ring']]).sum())
            s['ap_ct'] |= set(b['ctype'].tolist())
            b = rows['plane_plane']
            both = rg[b['bgn']] & rg[b['end']]
            s['pp_both'] += int(both.sum())
            s['pp_mixed'] += int((~both).sum())
            s['pp_ct'] |= set(b['ctype'].tolist())
            b = rows['group_group']
            s['gg'] += len(b['bgn'])
            s['gg_inter'] += int((b['ctype'] == CT['INTER']).sum())
            b = rows['group_plane']
            s['gp'] += len(b['amide'])
            s['gp_unmoved'] += int((~am[b['amide']]).sum())
            s['gp_moved'] += int(am[b['amide']].sum())
            s['takeover'] += int(((posed_res != home.ring_res) & ~has).sum())
            # a ring that is not affected keeps its residue
            assert ((posed_res == home.ring_res) | rg).all()
        seen[name] = s
        print(name, s)
    hem, lys, water, phe = (seen[k] for k in ('main', 'lys', 'water', 'phe'))
    assert hem['ap'] > 0 and {CT['INTER'], CT['INTRA_SELECTION'], CT['INTRA_BINDING_SITE']} <= hem['ap_ct']
    assert hem['pp_mixed'] > 0 and hem['pp_both'] > 0 and len(hem['pp_ct']) >= 2
    assert hem['gp'] > 0 and hem['gp_unmoved'] == hem['gp']
    assert lys['ap_movable_unaffected'] > 0 and lys['gg'] > 0 and lys['takeover'] > 0
    assert water['ap'] > 0 and water['ap_movable_unaffected'] > 0 and water['takeover'] > 0
    assert phe['gg_inter'] > 0 and phe['gp_moved'] > 0


# ------------------------------------------------------------------------------------------------------------- GPU: parity
@pytest.mark.gpu
def test_main_parity_with_the_ensemble_route():
    ctx, got, want = device_case('main')
    assert differences(got, want) == []
    info = ctx.poses_planes_info()
    assert info['poses'] == 70 and info['atoms'] == len(got['movable']) and info['moved_rings'] >= 4 and info['plane_atoms']
    assert [info[n] for n in poses.PLANE_TABLES] == [len(got[n]['ctype']) for n in poses.PLANE_TABLES]
    assert len(got['atom_plane']['atom']) > 100 and len(got['plane_plane']['bgn']) > 50 and len(got['group_plane']['amide']) > 10
    assert {CT['INTER'], CT['INTRA_SELECTION'], CT['INTRA_BINDING_SITE']} <= set(got['atom_plane']['ctype'].tolist())
    # the canonical order inside every pose
    for bags in poses.split_planes(got):
        for name in poses.PLANE_TABLES:
            a, b = (bags[name][c].astype(np.int64) for c in poses.PLANE_ORDER[name])
            assert (np.diff(a << 32 | b) > 0).all()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ('lys', 'phe', 'water', 'two', 'spread'))
def test_other_movable_sets_equal_the_ensemble_route(name):
    ctx, got, want = device_case(name)
    assert differences(got, want) == []
    if name == 'lys':        # partly selected amides: both peptide links are moved, the ring tables see the lysine's atoms only
        assert ctx.poses_planes_info()['moved_amides'] == 2 and len(got['group_group']['bgn']) > 0
    if name == 'phe':
        info = ctx.poses_planes_info()
        assert info['moved_rings'] == 1 and info['moved_amides'] == 2
        assert (got['group_group']['ctype'] == CT['INTER']).any() and len(got['group_plane']['amide']) > 0
    if name == 'water':
        assert got['summary'][:, 13].sum() > 0 and len(got['atom_plane']['atom']) > 0
    if name == 'spread':     # 30 moved rings over the whole box, pairs of two affected rings among the records
        assert ctx.poses_planes_info()['moved_rings'] == 30 and len(got['plane_plane']['bgn']) > 0
    ctx.close()


@pytest.mark.gpu
def test_box_seams_far_away_half_outside_and_one_pose():
    ctx, got, want = device_case('seams')
    assert differences(got, want) == []
    assert got['summary'][:2, 15].tolist() == [0, 0] and got['summary'][8, 15] == got['summary'][:, 15].max() > 0
    pc, idx, x, h = CASES['seams']()
    for p in (8, 0, 4):
        one = ctx.poses_planes(x[p:p + 1])
        per = poses.split_planes(want)[p]
        w = poses.planes_from_rows([per], idx)
        w['summary'][:, 12] = want['summary'][p, 12]
        assert differences(one, w) == [] and ctx.poses_planes_info()['poses'] == 1
    ctx.close()


@pytest.mark.gpu
def test_a_hand_made_take_over_and_a_release():
    pc, idx, x, h, r = case_takeover()
    ctx, got, want = device_case('takeover')
    assert differences(got, want) == []
    assert got['summary'][:, 13].tolist() == [1, 0]            # pose 0: one ring's residue is the water's now
    per = poses.split_planes(got)[0]
    mine = per['atom_plane']['ring'] == r
    # under the water's residue the ring is selected: with the water's own oxygen INTRA_SELECTION, with receptor rings INTER
    assert mine.any() and set(per['atom_plane']['ctype'][mine & np.isin(per['atom_plane']['atom'], idx)].tolist()) == {CT['INTRA_SELECTION']}
    assert set(per['atom_plane']['ctype'][mine & ~np.isin(per['atom_plane']['atom'], idx)].tolist()) <= {CT['INTER']}
    pp = (per['plane_plane']['bgn'] == r) | (per['plane_plane']['end'] == r)
    assert pp.any() and set(per['plane_plane']['ctype'][pp].tolist()) == {CT['INTER']}
    ctx.close()
    # the release: the water sits there at home, the poses take it away
    home = home_pack_gpu('release')
    pcr, rr = release_pack()
    wres = int(pcr.res_id[idx[0]])
    assert home.ring_res[rr] == wres == ref_py.ring_residues(pcr.xyz, pcr.res_id, home.ring_center)[0][rr]
    ctx, got, want = device_case('release')
    assert differences(got, want) == []
    assert got['summary'][0, 13] == 0 and (got['summary'][1:, 13] >= 1).all()      # pose 0 is home; every other gives the ring back to its own residue
    ctx.close()


@pytest.mark.gpu
def test_a_moved_ring_with_a_receptor_residue_and_one_with_none():
    ctx, got, want = device_case('triangle')
    assert differences(got, want) == []
    assert got['summary'][:, 12].min() >= 1 and got['summary'][:, 14].tolist() == [0, 1, 1]
    assert got['summary'][0, 13] == 1 and got['summary'][1:, 15].tolist() == [0, 0]     # residue -1 qualifies for nothing
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
def _fetch_fails(ctx):
    n = C.c_int64(0)
    s = np.zeros((4096, 16), np.uint32)
    rc = ctx._L.arp_poses_planes_fetch(ctx._h, 0, 0, *([None] * 10), s.ctypes.data_as(C.c_void_p), C.byref(n))
    return rc == _capi.ARP_E_ARG


@pytest.mark.gpu
def test_a_launch_voids_nothing_and_alternating_with_the_contacts_stays_exact():
    pc, idx, x, h = CASES['main']()
    home = home_pack_gpu('main')
    want = ensemble_table('main')
    ctx = _ctx(home, idx)
    counts = ctx.run_launch(*PARAMS)
    before = tp._fetch_everything(ctx)
    contacts = ctx.poses_contacts(x[:9], h[:9], 4.0, 0.25, True)
    got = ctx.poses_planes(x)
    assert differences(got, want) == []
    assert tp._same_bytes(tp._fetch_everything(ctx), before)
    n = C.c_int64(0)
    assert tp.differences(ctx.poses_contacts(x[:9], h[:9], 4.0, 0.25, True), contacts) == []      # the other result is as it was ...
    for _ in range(2):                                                                            # ... and the two alternate exactly
        assert differences(ctx.poses_planes(x), want) == []
        assert tp.differences(ctx.poses_contacts(x[:9], h[:9], 4.0, 0.25, True), contacts) == []
    assert ctx.run_launch(*PARAMS) == counts and tp._same_bytes(tp._fetch_everything(ctx), before)
    assert differences(ctx.poses_planes(x), want) == []
    ctx.close()


@pytest.mark.gpu
def test_the_result_goes_with_the_inputs_the_selection_and_the_plane_atoms():
    pc, idx, x, h = CASES['main']()
    home = home_pack_gpu('main')
    m = tp._mask(pc, idx)
    ctx = _capi.Context(0)
    ctx.set_complex(home)
    assert _fetch_fails(ctx) and ctx.poses_planes_info()['poses'] == 0
    ctx.set_selection(m)
    ctx.set_plane_atoms(home)
    t = ctx.poses_planes(x[:5])
    assert not _fetch_fails(ctx) and ctx.poses_planes_info()['atom_plane'] == len(t['atom_plane']['atom'])
    ctx.set_selection(m)                                             # the same selection, uploaded again
    assert _fetch_fails(ctx) and ctx.poses_planes_info()['poses'] == 0
    assert differences(ctx.poses_planes(x[:5]), t) == []            # (the plane atoms stay with the structure)
    ctx.set_plane_atoms(home)
    assert _fetch_fails(ctx)
    ctx.poses_planes(x[:5])
    ctx.set_complex(home)                                            # a new structure: the plane atoms go with the old one
    assert _fetch_fails(ctx) and not ctx.poses_planes_info()['plane_atoms']
    ctx.set_selection(m)
    with pytest.raises(ValueError, match='no plane atoms'):
        ctx.poses_planes(x[:5])
    ctx.set_plane_atoms(home)
    ctx.poses_planes(x[:5])
    ctx.set_topology(pc)
    assert not _fetch_fails(ctx)                                     # (the kept topology is not the resident structure)
    X, H = poses.as_models(pc, idx, x[:2], h[:2])
    ctx.set_models(X, H)
    assert _fetch_fails(ctx)
    ctx.close()


@pytest.mark.gpu
def test_every_refusal_names_its_cause():
    pc, idx, x, h = CASES['main']()
    home = home_pack_gpu('main')
    m = tp._mask(pc, idx)
    x = x[:3]
    ctx = _capi.Context(0)
    L, hd = ctx._L, ctx._h
    counts = np.zeros(4, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def launch(P=3, xs=x):
        xs = np.ascontiguousarray(xs, np.float32)
        rc = L.arp_poses_planes_launch(hd, P, p(xs), p(counts))
        return rc, L.arp_last_error(hd).decode()

    def refused(word, **kw):
        rc, msg = launch(**kw)
        assert rc == _capi.ARP_E_ARG and word in msg, (word, rc, msg)
    refused('no structure resident')
    ctx.set_complex(home)
    refused('no uploaded selection')
    ctx.set_selection(np.ones(pc.n_atoms, np.uint8))
    refused('whole structure')
    ctx.set_selection(np.zeros(pc.n_atoms, np.uint8))
    refused('ARP_POSES_MAX_ATOMS')
    ctx.set_selection(m)
    refused('ARP_POSES_MAX_POSES', P=0)
    refused('ARP_POSES_MAX_POSES', P=(1 << 20) + 1)
    refused('no plane atoms')
    # counts differ: the Python layer sees another pack's counts, the library missing arrays
    with pytest.raises(ValueError, match='counts differ'):
        ctx.set_plane_atoms(tp.soup())
    rc = L.arp_set_plane_atoms(hd, None, None, None)
    assert rc == _capi.ARP_E_ARG and 'counts differ' in L.arp_last_error(hd).decode()
    off = np.zeros(pc.n_rings + 1, np.int32)
    rc = L.arp_set_plane_atoms(hd, p(off), p(off), p(np.ascontiguousarray(pc.amide_atoms)))
    assert rc == _capi.ARP_E_ARG and 'at least three atoms' in L.arp_last_error(hd).decode()
    ctx.set_plane_atoms(home)
    assert launch()[0] == _capi.ARP_OK and counts.sum() > 0
    # a batch, models, shard ownership
    ctx.set_batch([home, home], [m, m])
    refused('batch')
    ctx.set_topology(pc)
    X, H = poses.as_models(pc, idx, x[:2], h[:2])
    ctx.set_models(X, H)
    ctx.set_selection(np.tile(m, 2))
    refused('models')
    ctx.set_complex(home)
    ctx.set_selection(m)
    ctx.set_plane_atoms(home)
    ctx._check(L.arp_set_ownership(hd, p(np.ones(pc.n_atoms, np.uint8)), p(np.arange(pc.n_atoms, dtype=np.int32))), 'arp_set_ownership')
    refused('shard')
    ctx.close()
    # the Python layer checks the shapes the library cannot see
    ctx = _capi.Context(0)
    ctx.set_complex(home)
    with pytest.raises(ValueError):
        ctx.poses_planes(x)                                          # no selection yet
    ctx.set_selection(m)
    ctx.set_plane_atoms(home)
    with pytest.raises(ValueError):
        ctx.poses_planes(x[:, :-1])
    # a column the table does not have
    ctx.poses_planes(x)
    n = C.c_int64(0)
    buf = np.zeros(4096, np.float64)
    rc = L.arp_poses_planes_fetch(ctx._h, 0, 4096, None, None, None, None, None, p(buf), None, None, None, None, None, C.byref(n))
    assert rc == _capi.ARP_E_ARG and 'no such value column' in L.arp_last_error(ctx._h).decode()
    rc = L.arp_poses_planes_fetch(ctx._h, 4, 0, *([None] * 11), C.byref(n))
    assert rc == _capi.ARP_E_ARG and 'table must be' in L.arp_last_error(ctx._h).decode()
    ctx.close()


@pytest.mark.gpu
def test_nan_and_inf_are_found_on_the_device_and_leave_no_result():
    pc, idx, x, h = CASES['lys']()
    ctx = _ctx(home_pack_gpu('lys'), idx)
    good = ctx.poses_planes(x[:4])
    for bad_value, where in ((np.nan, (2, 3, 1)), (np.inf, (3, 0, 0)), (-np.inf, (0, 5, 2))):
        bx = x[:4].copy()
        bx[where] = bad_value
        with pytest.raises(ValueError, match='non-finite'):
            ctx.poses_planes(bx)
        assert _fetch_fails(ctx) and ctx.poses_planes_info()['poses'] == 0
        assert differences(ctx.poses_planes(x[:4]), good) == []
    with pytest.raises(ValueError):
        ctx.poses_planes(x[:4, :-1])                                 # a refusal on the arguments leaves the resident result alone
    assert not _fetch_fails(ctx) and ctx.poses_planes_info()['poses'] == 4
    ctx.close()


@pytest.mark.gpu
def test_capacity_null_pointers_and_the_summary_alone():
    pc, idx, x, h = CASES['main']()
    ctx = _ctx(home_pack_gpu('main'), idx)
    t = ctx.poses_planes(x[:6])
    k = len(t['plane_plane']['bgn'])
    assert k > 1
    L, hd = ctx._L, ctx._h
    n = C.c_int64(0)
    e = np.full(k, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.arp_poses_planes_fetch(hd, 1, k - 1, None, None, p(e), *([None] * 8), C.byref(n))
    assert rc == _capi.ARP_E_CAPACITY and n.value == k and (e == -7).all()            # the needed count, nothing written
    rc = L.arp_poses_planes_fetch(hd, 1, k, None, None, p(e), *([None] * 8), C.byref(n))
    assert rc == _capi.ARP_OK and n.value == k and np.array_equal(e, t['plane_plane']['end'])     # one column alone
    off = np.zeros(7, np.uint64)
    rc = L.arp_poses_planes_fetch(hd, 3, 0, p(off), *([None] * 10), C.byref(n))
    assert rc == _capi.ARP_OK and np.array_equal(off, t['group_plane']['pose_off'])   # no record asked for: cap is not looked at
    s = ctx.poses_planes_summary(x[:6])
    assert s.dtype == np.uint32 and np.array_equal(s, t['summary'])
    ctx.close()


@pytest.mark.gpu
def test_a_caller_owned_stream_chunks_joined_and_run_poses():
    from test_gpu_paths import _hip_runtime
    pc, idx, x, h = CASES['main']()
    home = home_pack_gpu('main')
    want = ensemble_table('main')
    ctx = _ctx(home, idx)
    whole = ctx.poses_planes(x)
    assert differences(whole, want) == []
    parts = [ctx.poses_planes(x[a:b]) for a, b in ((0, 1), (1, 64), (64, 70))]
    assert differences(poses.concat_planes(parts), whole) == []
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    assert differences(ctx.poses_planes(x), whole) == []
    assert np.array_equal(ctx.poses_planes_summary(x[:7]), whole['summary'][:7])
    ctx.use_stream(0)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0
    # InteractionComplex.run_poses: without planes what it returned before, with planes the tables as well
    ic = InteractionComplex(copy.copy(home))
    plain = ic.run_poses(['RESNAME:HEM'], x, h, *PARAMS, chunk=32)
    assert getattr(ic, 'pose_planes', None) is None
    t = ic.run_poses(['RESNAME:HEM'], x, h, *PARAMS, chunk=32, planes=True)
    assert tp.differences(t, plain) == [] and differences(ic.pose_planes, whole) == []
    ic.run_poses(np.asarray(idx), x, h, *PARAMS, planes=True)
    assert differences(ic.pose_planes, whole) == []
