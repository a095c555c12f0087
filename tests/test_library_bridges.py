"""Library water bridges (arp_library_water_bridges_launch / _fetch / _info; Context.library_water_bridges /
library_water_bridges_info; InteractionComplex.run_library_water_bridges / write_library_water_bridges;
arpeggio_amd.library_bridges).

The yardstick, touched by none of the code under test: for pose t of ligand l, ``oracle.OracleComplex`` on
``complex_of(receptor, ligand_l, pose)`` with EVERYTHING selected, ``water_bridges.join`` over its bag, cut by
``library_bridges.reference_rows``.  The mirror ``library_bridges.join`` is checked against it on oracle-made inputs (which checks
the two independence claims of the definition), the device against the mirror on its own fetched tables and against the yardstick.
Every comparison is exact: ids and SIFt as integers, distances as bytes.  No tolerance anywhere, no time asserted."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import test_ligand_library as tl
from arpeggio_amd import _capi, synth
from arpeggio_amd import library_bridges as lb
from arpeggio_amd import ligand_library as ll
from arpeggio_amd import water_bridges as wb
from arpeggio_amd.core import config
from arpeggio_amd.core.interactions import InteractionComplex
from test_ligand_library import PARAMS, _ctx, _same_bytes, dock, launch, receptor

ENTRIES = ('arp_library_water_bridges_launch', 'arp_library_water_bridges_fetch', 'arp_library_water_bridges_info')
HP = wb.mask(('hbond', 'polar'))
ALL15 = wb.SIFT_ALL
COLS = tuple(k for k, _ in lb.COLUMNS)
W_TWO = (490, 502)       # two waters of receptor() 6.0 A apart, each with a polar receptor partner (490: four of them)
W_BARE = 484             # a water without a polar receptor partner


# ------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def case_waters():
    """Poses docked onto chosen waters of ``receptor()``: the amine's NZ midway between two waters that have polar receptor
    partners (one ligand atom on two waters, rows through two waters), NZ 2.9 A from the water with four such partners, NZ 2.9 A
    from a water without any (a ligand leg without a receptor leg: records, no row); a ligand without poses in the middle; a
    water ligand 2.8 A from a receptor water (a water-water record: no row)."""
    rec = receptor()
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    x = lambda a: rec.xyz[a].astype(np.float64)
    amine, halo, water = synth.ligand('amine', 3), synth.ligand('halo', 4), synth.ligand('water', 1)
    nz = amine.atom_name.index('NZ')
    hz1 = amine.h_xyz[amine.h_off[nz]] - amine.xyz[nz]
    mid = 0.5 * (x(W_TWO[0]) + x(W_TWO[1]))
    amine_poses = tl._stack(dock(amine, nz, hz1, mid, mid - centre, 0.0),
                            dock(amine, nz, hz1, x(W_TWO[0]), x(W_TWO[0]) - centre, 2.9),
                            dock(amine, nz, hz1, x(W_BARE), x(W_BARE) - centre, 2.9))
    water_poses = dock(water, 0, [1.0, 0.0, 0.0], x(W_TWO[0]), x(W_TWO[0]) - centre, 2.8)
    return rec, (amine, halo, water), [amine_poses, None, water_poses]


CASES = {'main': tl.case_main, 'waters': case_waters}


def _everything(pc):
    return np.ones(pc.n_atoms, np.uint8)


@functools.lru_cache(maxsize=None)
def receptor_bag(params):
    """The oracle's atom-atom bag of the receptor alone, everything selected."""
    oc = oracle.OracleComplex(receptor())
    oc.make_selection(_everything(receptor()))
    bag = oc.atom_contacts(*params)
    assert bag['err'] == 0
    return bag


@functools.lru_cache(maxsize=None)
def complex_bags(case, params):
    """Per global pose: the oracle's bag of a whole-structure pass over the complex with the pose in, everything selected."""
    rec, ligs, poses = CASES[case]()
    out = []
    for lig, item in zip(ligs, poses):
        for p in range(0 if item is None else len(item[0])):
            pc = ll.complex_of(rec, lig, item[0][p], item[1][p])
            oc = oracle.OracleComplex(pc)
            oc.make_selection(_everything(pc))
            bag = oc.atom_contacts(*params)
            assert bag['err'] == 0
            out.append((bag, pc.flags, pc.res_id))
    return out


def yardstick(case, params, sift_any):
    """Per global pose the rows the definition asks for, from the oracle alone."""
    n = receptor().n_atoms
    return [lb.reference_rows(wb.join(bag, flags, res_id, sift_any, same_residue=True), n) for bag, flags, res_id in complex_bags(case, params)]


def yardstick_legs(case, params, sift_any):
    """Per global pose the ligand legs, counted in the oracle's bag of the complex: a record of a receptor water and a ligand atom
    that is no water, with a wanted bit."""
    n = receptor().n_atoms
    out = []
    for bag, flags, _ in complex_bags(case, params):
        lo, hi = np.minimum(bag['i'], bag['j']).astype(np.int64), np.maximum(bag['i'], bag['j']).astype(np.int64)
        w = (np.asarray(flags).astype(np.int64) & config.F_WATER) != 0
        out.append(int(((lo < n) & (hi >= n) & w[lo] & ~w[hi] & ((bag['sift'].astype(np.int64) & sift_any) != 0)).sum()))
    return out


def differences(got, want, keys=COLS):
    """The names of what differs: columns as integers, distances as bytes."""
    bad = []
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


def check_per_pose(table, want, legs):
    """The table cut by bridge_off against the per-pose yardstick; ``waters`` against its rows, ``legs`` against the oracle's count."""
    parts = lb.split(table)
    assert len(parts) == len(want) and table['legs'].tolist() == legs and table['legs'].dtype == np.uint32
    for t, (g, w) in enumerate(zip(parts, want)):
        assert differences(g, w, [k for k in COLS if k != 'pose']) == [], t
        assert (g['pose'] == t).all() and g['pose'].dtype == np.int32
        assert int(table['waters'][t]) == len(np.unique(w['water']))
    key = [np.asarray(table[k]).astype(np.int64) for k in ('rec_atom', 'lig_atom', 'water', 'pose')]
    assert (np.diff(np.lexsort(key)) == 1).all()          # ascending by (pose, water, lig_atom, rec_atom), no row twice


# ------------------------------------------------------------------------------------------------------------- CPU
def test_the_entries_are_declared_and_bound():
    import os
    header = open(os.path.join(os.path.dirname(_capi.__file__), '..', 'include', 'arpeggio_hip.h')).read()
    for name in ENTRIES:
        assert name in _capi.SYMBOLS and ('int ' + name + '(arp_ctx* ctx') in header, name
    assert callable(_capi.Context.library_water_bridges) and callable(_capi.Context.library_water_bridges_info)
    assert callable(InteractionComplex.run_library_water_bridges) and callable(InteractionComplex.write_library_water_bridges)
    assert lb.mask is wb.mask and lb.mask() == HP and [k for k, _ in lb.COLUMNS] == list(COLS)


@functools.lru_cache(maxsize=None)
def oracle_mirror(case, sift_any):
    """``library_bridges.join`` over oracle-made library rows and the oracle's whole-receptor bag, PARAMS[0]."""
    rec, ligs, poses = CASES[case]()
    table = ll.from_rows(tl.oracle_rows(rec, ligs, poses, PARAMS[0]))
    return table, lb.join(table, receptor_bag(PARAMS[0]), rec.flags, ll.pack(ligs), sift_any)


@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('sift_any', (HP, ALL15))
def test_the_mirror_equals_the_oracle_yardstick_per_pose(case, sift_any):
    table, got = oracle_mirror(case, sift_any)
    want = yardstick(case, PARAMS[0], sift_any)
    check_per_pose(got, want, yardstick_legs(case, PARAMS[0], sift_any))
    assert int(got['bridge_off'][-1]) == len(got['pose']) == sum(len(w['water']) for w in want)
    assert [g.dtype for g in (got[k] for k, _ in lb.COLUMNS + lb.PER_POSE)] == [np.dtype(dt) for _, dt in lb.COLUMNS + lb.PER_POSE]


def test_the_oracle_alone_meets_the_coverage_condition():
    rec, ligs, poses = case_waters()
    want = yardstick('waters', PARAMS[0], HP)
    rows = lambda t: set(zip(want[t]['water'].tolist(), want[t]['lig_atom'].tolist(), want[t]['rec_atom'].tolist()))
    # a pose with rows through two waters, and one ligand atom on both
    waters_of_atom = {}
    for w, a, _ in rows(0):
        waters_of_atom.setdefault(a, set()).add(w)
    assert len({w for w, _, _ in rows(0)}) >= 2 and max(len(v) for v in waters_of_atom.values()) >= 2
    # a water with two receptor legs or more
    assert max(len({j for w, a, j in rows(1) if w == ww}) for ww in {w for w, _, _ in rows(1)}) >= 2
    # a ligand leg whose water has no receptor leg, in a pose with records but no row
    bag, flags, _ = complex_bags('waters', PARAMS[0])[2]
    n = rec.n_atoms
    legs = [(int(i), int(j)) for i, j, s in zip(bag['i'], bag['j'], bag['sift']) if min(i, j) == W_BARE and max(i, j) >= n and s & HP]
    assert legs and not rows(2)
    assert not any((s & HP) and ((i == W_BARE) != (j == W_BARE)) and max(i, j) < n and not (flags[i] & flags[j] & config.F_WATER)
                   for i, j, s in zip(bag['i'], bag['j'], bag['sift']))
    # a ligand without poses in the middle; a water ligand beside a receptor water: a record with a wanted bit, no row
    assert poses[1] is None and poses[0] is not None and poses[2] is not None
    bag, flags, _ = complex_bags('waters', PARAMS[0])[3]
    assert any(min(i, j) == W_TWO[0] and max(i, j) == n and s & HP for i, j, s in zip(bag['i'], bag['j'], bag['sift'])) and not rows(3)
    assert ligs[2].flags[0] & config.F_WATER
    # the main case: rows at all, and the ligand without poses in the middle
    main = yardstick('main', PARAMS[0], ALL15)
    assert sum(len(w['water']) for w in main) > 0 and tl.MAIN_P[3] == 0


def hand_table():
    t = dict(pose=[0, 0, 2, 2, 2], water=[7, 7, 5, 5, 9], lig_atom=[1, 1, 0, 3, 0], rec_atom=[2, 4, 4, 4, 2],
             dist_lig=[2.5, 2.5, 3.0, 3.25, 2.75], dist_rec=[3.0, 2.75, 2.5, 2.5, 3.5], sift_lig=[HP, HP, 64, 32, 96], sift_rec=[32, 64, 32, 32, 64])
    out = {k: np.asarray(t[k], dt) for k, dt in lb.COLUMNS}
    out.update(bridge_off=np.array([0, 2, 2, 5], np.uint64), waters=np.array([1, 0, 2], np.uint32), legs=np.array([1, 1, 3], np.uint32))
    return out


def test_host_functions_on_a_hand_made_table(tmp_path):
    t = hand_table()
    parts = lb.split(t)
    assert [len(p['pose']) for p in parts] == [2, 0, 3] and parts[2]['water'].tolist() == [5, 5, 9]
    sh = lb.shift(t, 10)
    assert sh['pose'].tolist() == [10, 10, 12, 12, 12] and sh['pose'].dtype == np.int32 and t['pose'].tolist() == [0, 0, 2, 2, 2]
    both = lb.concat([t, lb.empty(2), t])
    assert both['pose'].tolist() == [0, 0, 2, 2, 2, 5, 5, 7, 7, 7] and both['bridge_off'].tolist() == [0, 2, 2, 5, 5, 5, 7, 7, 10]
    assert both['waters'].tolist() == [1, 0, 2, 0, 0, 1, 0, 2] and both['legs'].tolist() == [1, 1, 3, 0, 0, 1, 1, 3]
    assert differences(lb.concat([t]), t, COLS + ('bridge_off', 'waters', 'legs')) == []
    res_id = np.array([0, 0, 1, 1, 1, 2, 2, 2, 3, 3], np.int32)
    br = lb.by_residue(t, res_id)
    assert br['pose'].tolist() == [0, 2] and br['res'].tolist() == [1, 1] and br['n_waters'].tolist() == [1, 2] and br['n_bridges'].tolist() == [2, 3]
    assert br['dist_min'].tobytes() == np.array([5.25, 5.5], np.float32).tobytes()
    rec = receptor()
    ligs = [synth.ligand('amine', 3), synth.ligand('halo', 4)]
    off = np.array([0, 1, 3], np.int64)
    records = lb.to_records(t, rec, ligs, off)
    assert len(records) == 5 and [(r['ligand'], r['pose']) for r in records] == [(0, 0), (0, 0), (1, 1), (1, 1), (1, 1)]
    assert records[0]['type'] == 'library-water-bridge' and records[0]['bgn']['contact'] == ['hbond', 'polar'] and records[0]['end']['distance'] == 3.0
    path = lb.write_library_bridges(str(tmp_path), 'x', t, rec, ligs, off)
    lines = open(path).read().splitlines()
    assert path.endswith('x.librarybridges') and lines[0] == ','.join(lb.CSV_HEADER) and len(lines) == 6
    assert lines[3].split(',')[:2] == ['1', '1'] and lines[3].split(',')[5:7] == ['3.0', '2.5']
    # ---- every refusal of the host functions, by name
    def refused(word, fn, *a):
        with pytest.raises(ValueError, match=word):
            fn(*a)
    bad = dict(t); bad.pop('legs')
    refused('no column', lb.split, bad)
    bad = dict(t, water=t['water'][:3])
    refused('differ in length', lb.split, bad)
    bad = dict(t, bridge_off=np.array([0, 2, 2, 4], np.uint64))
    refused('bridge_off must start at 0', lb.split, bad)
    bad = dict(t, waters=t['waters'][:2])
    refused(r'waters and legs \[T\]', lb.split, bad)
    refused('first_pose', lb.shift, t, -1)
    refused('no table given', lb.concat, [])
    refused('outside its own range', lb.concat, [dict(t, pose=t['pose'] + 1)])
    refused('different masks', lb.concat, [dict(t, sift_any=1), dict(t, sift_any=2)])
    refused('outside res_id', lb.by_residue, t, res_id[:3])
    refused('ligand_pose_off', lb.to_records, t, rec, ligs, np.array([0, 1, 2], np.int64))
    refused('sift_any', lb.join, ll.empty(1), dict(i=[], j=[], dist=[], sift=[]), rec.flags, ll.pack(ligs), 0)
    refused('unknown contact name', lb.mask, ['nope'])


# ------------------------------------------------------------------------------------------------------------- GPU
def bridges(ctx, rec, lib, poses, params=PARAMS[0], sift_any=HP, pass_first=True):
    """The device route on a fresh structure: the whole-receptor pass, the library launch, the join.  Returns the library
    table, the receptor's bag (both fetched) and the bridge table."""
    if pass_first:
        ctx.set_complex(rec)
        ctx.atom_contacts_launch(*params)
        ctx.set_ligand_library(lib)
    t = launch(ctx, lib, poses, params)
    b = ctx.library_water_bridges(sift_any=sift_any)
    return t, _bag(ctx), b


def _bag(ctx):
    """The resident atom-atom bag, in the order the pass left it."""
    n = C.c_int64(0)
    assert ctx._L.arp_atom_contacts_fetch(ctx._h, 0, None, None, None, None, None, C.byref(n)) in (0, _capi.ARP_E_CAPACITY)
    return ctx.atom_contacts_fetch(int(n.value), sort=False)


def equals_mirror(t, bag, b, rec, lib, sift_any):
    want = lb.join(t, bag, rec.flags, lib, sift_any)
    assert differences(b, want, COLS + ('bridge_off', 'waters', 'legs')) == []
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('params', (PARAMS[0], PARAMS[2]))
@pytest.mark.parametrize('case', sorted(CASES))
def test_cases_equal_the_mirror_and_the_oracle_yardstick(case, params):
    rec, ligs, poses = CASES[case]()
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)
    for sift_any in (HP, ALL15):
        t, bag, b = bridges(ctx, rec, lib, poses, params, sift_any)
        want = equals_mirror(t, bag, b, rec, lib, sift_any)
        check_per_pose(b, yardstick(case, params, sift_any), yardstick_legs(case, params, sift_any))
        info = ctx.library_water_bridges_info()
        assert (info['poses'], info['rows'], info['ligand_legs'], info['sift_any']) == (len(b['legs']), len(b['pose']), int(want['legs'].sum()), sift_any)
        if case == 'waters' and sift_any == HP:         # (records and ligand legs, no row: the water has no polar receptor partner)
            assert len(b['pose']) > 0 and b['legs'][2] > 0 and b['bridge_off'][3] == b['bridge_off'][2]
    ctx.close()


def _subset(counts, target):
    """Indices of a subset of ``counts`` that sums to ``target`` (ascending), or None."""
    reach = {0: []}
    for k, c in enumerate(counts):
        for s, ids in list(reach.items()):
            if s + c <= target and s + c not in reach:
                reach[s + c] = ids + [k]
    return reach.get(target)


@pytest.mark.gpu
def test_count_kernel_seams_record_counts_around_a_tile_and_a_leg_at_either_edge():
    """The chain ligand's poses come first and are trimmed so that the amine docked on a water lands where the count kernel's tile
    (2048 records) ends: totals of 2047, 2048, 2049 and 4097 records, a ligand leg as record 2047 and as record 2048."""
    rec = receptor()
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    chain, amine = synth.ligand('chain', 5, size=65), synth.ligand('amine', 3)
    lib = ll.pack((chain, amine))
    cx, ch = synth.library_poses_of(rec, chain, centre, 96, seed=13, shift=7.0)
    ax, ah = (a[1:2] for a in case_waters()[2][0])          # NZ 2.9 A from the water with four polar partners
    ctx = _capi.Context(0)
    t, bag, b = bridges(ctx, rec, lib, [(cx, ch), (ax, ah)])
    off = t['pose_off'].astype(np.int64)
    per_pose = np.diff(off)[:96].tolist()
    tail = int(off[97] - off[96])
    water = (rec.flags & config.F_WATER) != 0
    leg_at = [int(q) for q in range(int(off[96]), int(off[97])) if water[t['i'][q]] and t['sift'][q] & HP]
    assert tail > 0 and leg_at and sum(per_pose) > 4097
    first, last = leg_at[0] - int(off[96]), leg_at[-1] - int(off[96])
    targets = {'2047 records': 2047 - tail, '2048 records': 2048 - tail, '2049 records': 2049 - tail, 'two tiles crossed': 4097 - tail,
               'a leg is record 2048': 2048 - first, 'a leg is record 2047': 2047 - last}
    for name, target in targets.items():
        ids = _subset(per_pose, target)
        assert ids is not None, name
        t, bag, b = bridges(ctx, rec, lib, [(cx[ids], ch[ids]), (ax, ah)], pass_first=False)
        assert int(t['pose_off'][len(ids)]) == target, name
        want = equals_mirror(t, bag, b, rec, lib, HP)
        assert want['legs'][-1] > 0 and len(want['pose']) > 0, name
    ctx.close()


@functools.lru_cache(maxsize=None)
def dense_box():
    return synth.make_synthetic(1500, seed=7, density=0.12, water_frac=0.2)


@pytest.mark.gpu
def test_write_kernel_seams_a_water_with_more_than_64_receptor_legs():
    """A dense box under `proximal` at 6 A: one water has more than 64 receptor legs, so the rows of ONE ligand leg cross a 64-lane
    step; a 20-atom ligand on it gives more rows than the 256 a block writes a step, and two poses meet inside one tile."""
    rec = dense_box()
    prox = wb.mask(('proximal',))
    ctx = _capi.Context(0)
    ctx.set_complex(rec)
    ctx.atom_contacts_launch(*PARAMS[2])
    bag = _bag(ctx)
    water = (rec.flags & config.F_WATER) != 0
    leg = (water[bag['i']] != water[bag['j']]) & ((bag['sift'] & prox) != 0)
    per_water = np.bincount(np.where(water[bag['i']], bag['i'], bag['j'])[leg], minlength=rec.n_atoms)
    w = int(np.argmax(per_water))
    assert per_water[w] > 64
    one, many = synth.ligand('ion', 2), synth.ligand('chain', 5, size=20)
    lib = ll.pack((one, many))
    at = rec.xyz[w].astype(np.float64)
    p_one = tl._stack(dock(one, 0, [1.0, 0.0, 0.0], at, [0.0, 0.0, 1.0], 3.0), dock(one, 0, [1.0, 0.0, 0.0], at, [0.0, 1.0, 0.0], 3.2))
    p_many = synth.library_poses_of(rec, many, at, 3, seed=3, shift=1.0)
    ctx.set_ligand_library(lib)
    t, bag, b = bridges(ctx, rec, lib, [p_one, p_many], PARAMS[2], prox, pass_first=False)
    want = equals_mirror(t, bag, b, rec, lib, prox)
    assert int(t['pose_off'][2]) < 2048 and (want['legs'][:2] > 0).all()    # two poses with legs meet inside the first tile
    m_of_leg = np.diff(np.nonzero(np.r_[True, (np.diff(want['pose']) != 0) | (np.diff(want['water']) != 0) | (np.diff(want['lig_atom']) != 0), True])[0])
    assert m_of_leg.max() > 64 and len(want['pose']) > 2048 and (np.diff(want['bridge_off'].astype(np.int64)) > 256).any()
    assert (want['legs'] > 0).sum() >= 2
    # from the row prefixes: a leg's first row inside its block is its global first row less that of the first leg of its tile of
    # 2048 records; some leg's rows cross a 64-lane step, and some a 256-row step of the block
    first_row = np.r_[0, np.cumsum(m_of_leg)[:-1]]
    leg_row = np.nonzero(np.r_[True, (np.diff(want['pose']) != 0) | (np.diff(want['water']) != 0) | (np.diff(want['lig_atom']) != 0)])[0]
    record = {key: q for q, key in enumerate(zip(ll.pose_of(t).tolist(), t['i'].tolist(), t['a'].tolist()))}
    tile = np.array([record[(int(want['pose'][r]), int(want['water'][r]), int(want['lig_atom'][r]))] for r in leg_row]) // 2048
    in_block = first_row - np.array([first_row[np.nonzero(tile == tt)[0][0]] for tt in tile])
    assert (in_block % 64 + m_of_leg > 64).any() and (in_block % 256 + m_of_leg > 256).any()
    # a tile whose legs all have m = 0: a mask no receptor leg of these waters meets but `proximal` alone decides; the amine on the
    # bare water of the small receptor
    rec2, ligs2, poses2 = case_waters()
    lib2 = ll.pack(ligs2)
    only_bare = [(poses2[0][0][2:3], poses2[0][1][2:3]), None, None]
    t, bag, b = bridges(ctx, rec2, lib2, only_bare)
    want = equals_mirror(t, bag, b, rec2, lib2, HP)
    assert want['legs'].tolist() == [int(want['legs'][0])] and want['legs'][0] > 0 and len(b['pose']) == 0 and b['waters'].tolist() == [0]
    ctx.close()


@pytest.mark.gpu
def test_empties_no_water_no_leg_under_the_mask_and_one_pose():
    rec, ligs, poses = case_waters()
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)
    zeros = lambda b, T: (len(b['pose']), b['bridge_off'].tolist(), b['waters'].tolist(), b['legs'].tolist()) == (0, [0] * (T + 1), [0] * T, [0] * T)
    # a receptor without waters
    dry = synth.proteinlike(n_res=30, seed=5, n_waters=0)
    shift = rec.xyz.astype(np.float64).mean(axis=0) - dry.xyz.astype(np.float64).mean(axis=0)
    dry = copy.copy(dry)
    dry.xyz = (dry.xyz.astype(np.float64) + shift).astype(np.float32)
    dry.h_xyz = dry.h_xyz + shift
    t, bag, b = bridges(ctx, dry, lib, poses)
    assert zeros(b, 4) and ctx.library_water_bridges_info()['rows'] == 0
    # a mask no leg meets
    none = wb.mask(('covalent',))          # (a ligand has no bond to the receptor: no ligand leg)
    t, bag, b = bridges(ctx, rec, lib, poses, sift_any=none)
    assert zeros(b, 4) and differences(b, lb.join(t, bag, rec.flags, lib, none), COLS + ('bridge_off', 'waters', 'legs')) == []
    # T = 1
    one = [(poses[0][0][1:2], poses[0][1][1:2]), None, None]
    t, bag, b = bridges(ctx, rec, lib, one)
    equals_mirror(t, bag, b, rec, lib, HP)
    assert len(b['legs']) == 1 and len(b['pose']) > 0 and b['bridge_off'].tolist() == [0, len(b['pose'])]
    far = [(poses[0][0][1:2] + np.float32(500.0), poses[0][1][1:2] + 500.0), None, None]
    t, bag, b = bridges(ctx, rec, lib, far)
    assert len(t['i']) == 0 and zeros(b, 1)
    ctx.close()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.gpu
def test_contract_stored_count_another_mask_capacity_null_pointers_and_a_stream():
    from test_gpu_paths import _hip_runtime
    rec, ligs, poses = case_waters()
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)
    t, bag, b = bridges(ctx, rec, lib, poses)
    B, T = len(b['pose']), 4
    work = ctx.library_water_bridges_info()['launches']
    n = C.c_int64(-1)
    assert ctx._L.arp_library_water_bridges_launch(ctx._h, HP, C.byref(n)) == 0 and n.value == B
    assert ctx.library_water_bridges_info()['launches'] == work            # the stored count, no work
    b2 = ctx.library_water_bridges(sift_any=ALL15)                         # remade on another mask
    assert ctx.library_water_bridges_info()['launches'] == work + 1 and len(b2['pose']) > B
    equals_mirror(t, bag, b2, rec, lib, ALL15)
    assert _same_bytes({k: ctx.library_water_bridges(sift_any=HP)[k] for k in COLS}, {k: b[k] for k in COLS})
    # capacity and NULL pointers
    L = ctx._L
    fetch = lambda cap_rows, cap_poses, cols, per: L.arp_library_water_bridges_fetch(ctx._h, cap_rows, cap_poses, *cols, *per, C.byref(n))
    none8, none3 = [None] * 8, [None] * 3
    assert fetch(0, 0, none8, none3) == 0 and n.value == B
    pose = np.full(B, -1, np.int32)
    legs = np.full(T, 99, np.uint32)
    assert fetch(B - 1, T, [_p(pose)] + none8[1:], none3) == _capi.ARP_E_CAPACITY and n.value == B and (pose == -1).all()
    assert fetch(B, T - 1, none8, [None, None, _p(legs)]) == _capi.ARP_E_CAPACITY and (legs == 99).all()
    assert fetch(B, 0, [_p(pose)] + none8[1:], none3) == 0 and np.array_equal(pose, b['pose'])
    assert fetch(0, T, none8, [None, None, _p(legs)]) == 0 and np.array_equal(legs, b['legs'])
    assert L.arp_library_water_bridges_fetch(ctx._h, 0, 0, *none8, *none3, None) == _capi.ARP_E_ARG
    assert L.arp_library_water_bridges_launch(ctx._h, HP, None) == _capi.ARP_E_ARG and L.arp_library_water_bridges_info(ctx._h, None) == _capi.ARP_E_ARG
    # a caller-owned stream
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    t3, bag3, b3 = bridges(ctx, rec, lib, poses, sift_any=ALL15)
    assert differences(b3, b2, COLS + ('bridge_off', 'waters', 'legs')) == []
    ctx.use_stream(0)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0


@pytest.mark.gpu
def test_run_library_water_bridges_chunked_equals_unchunked_and_the_written_file(tmp_path):
    rec, ligs, poses = CASES['main']()
    ic = InteractionComplex(copy.copy(rec))
    whole = ic.run_library_water_bridges(ligs, poses, contacts=None)
    assert ic.library_water_bridges is whole and len(whole['pose']) > 0 and whole['ligand_pose_off'].tolist() == np.r_[0, np.cumsum(tl.MAIN_P)].tolist()
    check_per_pose(whole, yardstick('main', PARAMS[0], ALL15), yardstick_legs('main', PARAMS[0], ALL15))
    for chunk in (32, 71):                  # (both cut the first ligand's 70 poses or the ligands behind it between two launches)
        got = ic.run_library_water_bridges(ligs, poses, contacts=None, chunk=chunk)
        assert differences(got, whole, COLS + ('bridge_off', 'waters', 'legs')) == [], chunk
    rec2, ligs2, poses2 = case_waters()
    ic = InteractionComplex(copy.copy(rec2))
    t = ic.run_library_water_bridges(ligs2, poses2, chunk=2)         # (the amine's three poses are cut between two launches)
    check_per_pose(t, yardstick('waters', PARAMS[0], HP), yardstick_legs('waters', PARAMS[0], HP))
    path = ic.write_library_water_bridges(str(tmp_path))
    lines = open(path).read().splitlines()
    assert path.endswith('.librarybridges') and lines[0] == ','.join(lb.CSV_HEADER) and len(lines) == 1 + len(t['pose'])
    first = lines[1].split(',')
    assert first[:2] == ['0', '0'] and first[2].endswith('/O') and first[5] == str(t['dist_lig'][0])


def _library_state(ctx, T, L):
    """Everything the library route keeps resident, FETCHED without a launch: the records with their offsets and summary, the
    best-pose table, the fingerprint with its best table, the shortlist with its records, the clusters; and the info words."""
    import test_library_clusters as tlc
    import test_library_shortlist as tls
    return dict(records=tls._library_fetch(ctx, T), best=tls._library_best_fetch(ctx, L), fp=tls._library_fp_fetch(ctx, L),
                shortlist=tls._resident(ctx)[::2], clusters=tlc._resident(ctx)[::2],      # ((rc, arrays): not the last error's text)
                info=ctx.library_info(), fp_info=ctx.library_fingerprints_info(),
                shortlist_info=ctx.library_shortlist_info(), clusters_info=ctx.library_clusters_info())


def _refused(ctx, word=None):
    n = C.c_int64(0)
    rc = ctx._L.arp_library_water_bridges_fetch(ctx._h, 0, 0, *([None] * 11), C.byref(n))
    return rc == _capi.ARP_E_ARG


@pytest.mark.gpu
def test_making_it_voids_nothing_and_it_goes_with_its_two_sources():
    from arpeggio_amd import library_fingerprints as lfp
    rec, ligs, poses = case_waters()
    lib = ll.pack(ligs)
    ctx = _ctx(rec)
    ctx.run_launch(*PARAMS[0])
    wb5i = ctx.water_bridges(HP)
    ctx.set_ligand_library(lib)
    t = launch(ctx, lib, poses)
    r1 = ll.split(t)[0][1]
    refs = lfp.references([lfp.reference_from_records(r1['i'], r1['sift'], r1['ctype'], rec.res_id)], rec.n_residues)
    ctx.library_best(np.ones(16, np.int32))
    fp = ctx.library_fingerprints(refs, ALL15, 0x7F, by_residue=True)
    ctx.library_fingerprints_best()
    sl = ctx.library_shortlist('summary', unit='poses', k=3, weights=np.r_[np.ones(16), np.zeros(16)].astype(np.int32))
    cl = ctx.library_clusters(1 << 31)
    T, L = 4, 3
    before = tl._fetch_everything(ctx), ctx.water_bridges(HP), _library_state(ctx, T, L)
    assert _refused(ctx) and len(t['i']) > 0 and len(sl['pose']) == 3 and len(cl['pose']) == T and fp is not None
    assert tl.differences(dict(before[2]['records'], ligand_pose_off=t['ligand_pose_off']), t) == []     # (the fetch is the launch's table)
    for mask in (HP, ALL15):                                         # (both masks: the second remakes the result on its own scratch)
        b = ctx.library_water_bridges(sift_any=mask)
        after = tl._fetch_everything(ctx), ctx.water_bridges(HP), _library_state(ctx, T, L)
        assert [k for k in before[2] if not _same_bytes(before[2][k], after[2][k])] == [], mask
        assert len(b['pose']) > 0 and _same_bytes(before, after) and _same_bytes(wb5i, after[1]) and not _refused(ctx), mask
    launch(ctx, lib, poses)
    # ---- refused after each of: a new library launch, a new pass, a new library, a new structure
    assert _refused(ctx)                                             # (the launch just above replaced the library result)
    ctx.library_water_bridges(sift_any=HP)
    ctx.atom_contacts_launch(*PARAMS[0])
    assert _refused(ctx)
    ctx.library_water_bridges(sift_any=HP)
    ctx.set_ligand_library(lib)
    assert _refused(ctx)
    launch(ctx, lib, poses)
    ctx.library_water_bridges(sift_any=HP)
    ctx.set_complex(rec)
    assert _refused(ctx)
    # ---- set_selection voids the atom-atom bag, and the bridges go with it; the library result stays, and a pass with
    # everything selected brings the bridges back without another library launch
    ctx.atom_contacts_launch(*PARAMS[0])
    launch(ctx, lib, poses)
    want = ctx.library_water_bridges(sift_any=HP)
    ctx.set_selection(np.ones(rec.n_atoms, np.uint8))
    assert _refused(ctx) and ctx.library_info()['poses'] == 4
    ctx.atom_contacts_launch(*PARAMS[0])
    assert differences(ctx.library_water_bridges(sift_any=HP), want, COLS + ('bridge_off', 'waters', 'legs')) == []
    ctx.close()


@pytest.mark.gpu
def test_every_refusal_by_name_in_order():
    rec, ligs, poses = case_waters()
    lib = ll.pack(ligs)
    ctx = _capi.Context(0)

    def refused(word, sift_any=HP):
        with pytest.raises(ValueError, match=word):
            ctx.library_water_bridges(sift_any=sift_any)

    # nothing resident at all: the masks come first, then the library result, then the bag
    refused('beyond the 15 SIFt bits', 1 << 15)
    refused('sift_any of 0', 0)
    refused('no library result')
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    launch(ctx, lib, poses)
    refused('beyond the 15 SIFt bits', 1 << 15)
    refused('no atom-contact results')
    # a bag made under a partial selection
    part = np.zeros(rec.n_atoms, np.uint8)
    part[:50] = 1
    ctx.set_selection(part)
    ctx.atom_contacts_launch(*PARAMS[0])
    refused('partial selection')
    assert not ctx.library_water_bridges_info()['ready']
    # everything selected, another cutoff / another vdw_comp than the library launch's
    ctx.set_selection(np.ones(rec.n_atoms, np.uint8))
    ctx.atom_contacts_launch(4.0, 0.1, False)
    refused('cutoff or vdw_comp')
    ctx.atom_contacts_launch(5.0, 0.3, False)
    refused('cutoff or vdw_comp')
    assert not ctx.library_water_bridges_info()['ready']
    ctx.atom_contacts_launch(5.0, 0.1, True)             # (include_sequence_adjacent need not match)
    assert ctx.library_water_bridges_info()['ready']
    before = _bag(ctx)
    refused('sift_any of 0', 0)
    assert _same_bytes(_bag(ctx), before) and _refused(ctx)
    assert len(ctx.library_water_bridges(sift_any=HP)['pose']) > 0
    # a pass that was not waited for
    ctx.run_enqueue(*PARAMS[0])
    refused('no atom-contact results')
    ctx.run_wait()
    ctx.close()
