"""Shard assembly and ownership on their seams (tests/shard_cases.py builds the structures).

A  the device assembly (csrc/arp_shard.h: k_face_flags, k_scan_segments, k_face_write, k_merge_positions, k_merge_fill,
   k_merge_groups) against the host assembly (sharding.make_shard_local / assemble_shard, plain NumPy): home lists on the
   4 096-element chunk seam of the scans, items on the face bounds and on the cuts, merges whose three lists interleave.
B  the ownership rule at the cuts (M_HOME of the bgn atom in k_search, ring_home / am_home of the first item in the ring and
   amide loops) and the three-stage selection exchange against the ORACLE on the whole unsharded structure: the ranks' records
   concatenated, nothing removed, must be the oracle's — every record once.
C  the same cases without a GPU: host shards, the oracle per shard, the ownership rule; and every case reaches the edge it was
   built for.

One GPU, one context per emulated rank, at most five contexts open at a time."""
import numpy as np
import pytest

import shard_cases as sc
from arpeggio_amd import sharding


@pytest.fixture(scope='module')
def capi():
    from arpeggio_amd import _capi
    return _capi


@pytest.fixture(scope='module')
def cases():
    return {c.name: c for c in sc.ownership_cases()}


@pytest.fixture(scope='module')
def references():
    """(case name, whole) -> the oracle's bags of the unsharded structure, computed once and left unchanged."""
    memo = {}

    def get(case, whole):
        key = (case.name, whole)
        if key not in memo:
            memo[key] = sc.oracle_reference(case, whole)
        return memo[key]
    return get


OWNERSHIP = [('thin', 2), ('on_cut', 2), ('on_cut', 3), ('on_cut', 4), ('cutoff6', 2), ('cutoff6', 3), ('reach', 2), ('res_sets', 2),
             ('planes', 2), ('planes', 3), ('narrow3', 3), ('merge_interleave', 3)]


# ---- A: device assembly against host assembly ----------------------------------------------------------------------------------
def _check_assembly(capi, case, world, sel=None):
    whole = sel is None
    bounds = case.tags.get('bounds')
    hss = sc.host_shards(case, world, sel, bounds)
    ctxs, dss = sc.device_shards(capi, case, world, sel, whole, bounds)
    ref = capi.Context(0)
    blobs = []
    try:
        for r, (c, ds, hs) in enumerate(zip(ctxs, dss, hss)):
            blobs.append(sc.assert_device_shard_equals_host(capi, c, ds, hs, (case.name, r)))
            sc.assert_pass_equal(c, ds, ref, hs, whole, case.cutoff, (case.name, r))
    finally:
        for c in ctxs + [ref]:
            c.close()
    return dss, hss, blobs


@pytest.mark.gpu
@pytest.mark.parametrize('n_home,face,n_rings,n_amides,many_radii', sc.scan_cases())
def test_scan_seams(capi, n_home, face, n_rings, n_amides, many_radii):
    """A1: rank 0's home lists sized on the chunk seam of k_scan_segments (and 0, 1, 65 rings / amides; one list of rings and one
    of amides past 4 096), its right face holding all of them, none, or the two items at indices 4 095 / 4 096; hydrogen and bond
    counts that make the three atom scans carry different sums.  Both ranks' shards against the host assembly."""
    case = sc.scan_case(n_home, face, n_rings, n_amides, many_radii)
    dss, hss, blobs = _check_assembly(capi, case, 2)
    a_own = case.owners(2)[0]
    assert int((a_own == 0).sum()) == n_home
    want = {'all': n_home, 'none': 0, 'two': len(sc._picked(n_home, 'two', first=1))}[face]
    assert int((dss[1].origin == -1).sum()) == want                  # what rank 1 received from rank 0's right face
    if n_home > 4097:
        home = hss[0]
        hc, bc = np.diff(home.pc.h_off)[home.is_home == 1], np.diff(home.pc.bond_off)[home.is_home == 1]
        assert len({4096, int(hc[:4096].sum()), int(bc[:4096].sum())}) == 3       # three different carries across the seam
    if many_radii:
        assert all((b['rad_idx'] == sc.RAD_NONE).any() for b in blobs), 'more radius pairs than the table holds: 0xFFFF must occur'
        assert all((b['rad_idx'] != sc.RAD_NONE).any() for b in blobs)


def _expect_in_face(x, side, bound):
    return float(x) >= bound if side > 0 else float(x) <= bound


@pytest.mark.gpu
@pytest.mark.parametrize('exact', [False, True])
@pytest.mark.parametrize('world', [2, 3])
def test_face_membership(capi, world, exact):
    """A2: atoms, ring centres and amide centres on the face bounds, one step inside and one step outside, and on the cuts: which
    of them each neighbour's shard holds, by global id, and the blanket comparison with the host assembly.  exact: the faces cut
    with the float32 number next to the halo's bound, so that atoms and amide centres sit ON the bound (both ends are inclusive)."""
    case = sc.face_case(world, exact)
    dss, hss, _ = _check_assembly(capi, case, world)
    pc, t = case.pc, case.tags
    for items, x_of, gid_of in ((t['bound_atoms'], lambda i: pc.xyz[i, 0], lambda ds: ds.global_id),
                                (t['bound_rings'], lambda i: pc.ring_center[i, 0], lambda ds: ds.ring_gid),
                                (t['bound_amides'], lambda i: pc.amide_center[i, 0], lambda ds: ds.amide_gid)):
        for i, k, side, bd in items:
            # side +1: rank k - 1 sends to rank k what has x >= bd; side -1: rank k sends to rank k - 1 what has x <= bd
            receiver = k if side > 0 else k - 1
            inside = _expect_in_face(x_of(i), side, bd)
            assert (i in set(gid_of(dss[receiver]).tolist())) == inside, (i, k, side, bd, float(x_of(i)))
    for i, k, x in t['cut_atoms']:
        owner = k if x >= case.cuts[world][k - 1] else k - 1                        # an atom exactly on a cut belongs to the right slab
        for r, ds in enumerate(dss):
            at = np.nonzero(ds.global_id == i)[0]
            if r == owner:
                assert len(at) == 1 and ds.origin[at[0]] == 0, (i, r)
            elif abs(r - owner) == 1 and r in (k, k - 1):
                assert len(at) == 1 and ds.origin[at[0]] == (owner - r), (i, r)         # in the other side's halo
    if exact:
        return
    # and _face_sets, the host counterpart of k_face_flags, says the same
    halo = sharding.halo_width()
    edges, a_own, r_own, m_own = sharding._partition(pc, world, halo)
    for r, ds in enumerate(dss):
        rings, amides = [], []
        for side, nb in ((-1, r - 1), (+1, r + 1)):
            if 0 <= nb < world:
                ai, ri, mi = sharding._face_sets(pc, edges, a_own, r_own, m_own, nb, -side, halo)
                assert np.array_equal(ds.global_id[ds.origin == side], ai), (r, side)
                rings.append(ri)
                amides.append(mi)
        assert np.array_equal(ds.ring_gid[ds.ring_home == 0], np.sort(np.concatenate(rings))), r
        assert np.array_equal(ds.amide_gid[ds.amide_home == 0], np.sort(np.concatenate(amides))), r


@pytest.mark.gpu
@pytest.mark.parametrize('kind,selected', [('interleave', False), ('interleave', True), ('empty_home', False), ('one_halo', False)])
def test_merges_that_interleave(capi, kind, selected):
    """A3: ids that cycle over the three slabs, so that the middle rank's three lists interleave element by element; a rank with an
    empty home list and two halos; a rank with exactly one empty halo; bonds inside a list, across the cut, to atoms beyond the
    halo (dropped), hydrogens on halo atoms, single-bond neighbours that are not local."""
    case = sc.merge_case(kind)
    sel = sc._thirds(case.pc) if selected else None
    dss, hss, blobs = _check_assembly(capi, case, 3, sel)
    mid = dss[1]
    if kind == 'interleave':
        o = mid.origin.astype(int)
        runs = np.diff(np.nonzero(np.diff(o) != 0)[0])
        assert (o == 0).sum() >= 40 and (o == -1).sum() >= 40 and (o == 1).sum() >= 40
        assert (runs == 1).sum() >= 60, 'the three lists must interleave element by element'
        assert len(mid.ring_gid) > 20 and len(mid.amide_gid) > 20
        assert len(set(np.diff(np.nonzero(mid.ring_home == 1)[0]).tolist()) - {1}) > 0         # home rings lie between halo rings
        h = hss[1]
        full_deg, local_deg = np.diff(case.pc.bond_off)[h.global_id], np.diff(h.pc.bond_off)
        assert (local_deg < full_deg).any() and (local_deg == 0).any() and (local_deg > 0).any()       # partners beyond the halo vanished
        assert np.diff(h.pc.h_off)[h.is_home == 0].sum() > 0                                           # hydrogens on halo atoms
        for nb, d, a in case.tags['xbond']:
            assert nb not in set(h.global_id.tolist()) and h.sb_has[np.nonzero(h.global_id == d)[0][0]] == 1
    elif kind == 'empty_home':
        assert (mid.origin == 0).sum() == 0 and (mid.origin == -1).sum() >= 40 and (mid.origin == 1).sum() >= 40
        assert (blobs[1]['rad_idx'] == sc.RAD_NONE).all()               # an empty home list brings an empty radius table
    else:
        assert (mid.origin == 0).sum() >= 40 and (mid.origin == -1).sum() >= 40 and (mid.origin == 1).sum() == 0


# ---- B: ownership at the cuts against the oracle -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('flow', ['whole', 'staged'])
@pytest.mark.parametrize('name,world', OWNERSHIP)
def test_union_of_the_ranks_is_the_oracle(capi, cases, references, name, world, flow):
    """Device-assembled shards, one context per rank; 'whole': run_shard_whole_structure; 'staged': arp_run_stage 0 / 1 / 2 with the
    plus bits and the residue sets moved between the contexts.  The ranks' records, concatenated without removing anything,
    are the oracle's records of the unsharded structure."""
    case = cases[name]
    whole = flow == 'whole'
    exp, _ = references(case, whole)
    per_rank, sets = sc.gpu_union(capi, case, world, whole)
    sc.assert_ranks_and_union_equal(case, world, per_rank, exp, (name, world, flow))
    if name == 'res_sets' and not whole:
        merged = np.maximum.reduce(sets)
        assert any(not np.array_equal(s, merged) for s in sets), 'the reduction of the residue sets is not exercised'


# ---- C: the cases reach their edges; the reference side on its own (no GPU) ----------------------------------------------------
@pytest.mark.parametrize('name,world', OWNERSHIP)
def test_cases_reach_their_edges_on_the_cpu(cases, references, name, world):
    case = cases[name]
    pc = case.pc
    for whole in (True, False):
        exp, oc = references(case, whole)
        out = sc.cpu_union(case, world, whole)
        sc.assert_ranks_and_union_equal(case, world, out['per_rank'], exp, (name, world, 'whole' if whole else 'staged'))
        cross = sc.crossing(case, world, exp)
        if name in ('thin', 'on_cut', 'cutoff6', 'planes', 'narrow3', 'merge_interleave'):
            assert min(cross['atom_atom']) > 0, cross                # both ways: the bgn atom left of the cut, and right of it
        if name in ('thin', 'planes', 'narrow3'):
            for bag in sc.BAGS:
                assert sum(cross[bag]) > 0, (bag, cross)
        if name == 'planes' and whole:
            assert all(min(cross[bag]) > 0 for bag in sc.BAGS), cross
            assert (pc.ring_center[:, 0] == np.array(case.cuts[world])[:, None]).any()          # a ring centre on a cut
            r_own, a_own = case.owners(world)[1], case.owners(world)[0]
            res_owner = np.array([np.bincount(a_own[pc.res_id == r]).argmax() for r in pc.ring_res])
            assert (res_owner != r_own).any()                                                   # a ring whose residue lies across the cut
        if name == 'thin':
            assert all(sh.pc.n_atoms == pc.n_atoms - 1 for sh in out['shards'])                 # both hold all but the other's sentinel
        if name == 'on_cut' and whole:
            aa = set(zip(exp['atom_atom']['i'].tolist(), exp['atom_atom']['j'].tolist()))
            cuts = case.cuts[world]
            for i, j in case.tags['pairs']:
                if any(min(pc.xyz[i, 0], pc.xyz[j, 0]) <= c <= max(pc.xyz[i, 0], pc.xyz[j, 0]) for c in cuts):
                    assert (min(i, j), max(i, j)) in aa or (max(i, j), min(i, j)) in aa, (i, j)
        if name == 'cutoff6' and whole:
            d = exp['atom_atom']
            for i, j in case.tags['pairs']:
                hit = ((d['i'] == min(i, j)) & (d['j'] == max(i, j))) | ((d['i'] == max(i, j)) & (d['j'] == min(i, j)))
                assert hit.sum() == 1 and d['dist'][hit][0] >= 5.99, (i, j)
        if name == 'reach' and not whole:
            d = exp['atom_atom']
            for trio, s, m, t in case.tags['trios']:
                assert case.sel[s] == 1 and case.sel[m] == 0 and oc.in_plus[m] == 1, trio
                only_s = np.nonzero(case.sel)[0]
                dist = np.linalg.norm(pc.xyz[only_s].astype(np.float64) - pc.xyz[m].astype(np.float64), axis=1)
                assert (dist <= 6.0).sum() == 1 and only_s[dist <= 6.0][0] == s, trio              # M is in selection_plus because of S alone
                assert (((d['i'] == m) & (d['j'] == t)) | ((d['i'] == t) & (d['j'] == m))).sum() == 1, trio
                if trio.startswith('beyond'):       # the rank that owns T cannot know M's bit without the exchange
                    rank_t = int(case.owners(world)[0][t])
                    sh = out['shards'][rank_t]
                    at = np.nonzero(sh.global_id == m)[0][0]
                    assert sh.is_home[at] == 0 and out['local_plus'][rank_t][at] == 0 and out['masks'][rank_t]['plus'][at] == 1, trio
        if name == 'res_sets' and not whole:
            merged = np.maximum.reduce(out['sets'])
            assert any(not np.array_equal(s, merged) for s in out['sets'])
            ring_sel_local = [np.where(sh.pc.ring_res >= 0, s[:sh.n_res_global][np.maximum(sh.pc.ring_res, 0)], 0) for sh, s in zip(out['shards'], out['sets'])]
            assert any((m['ring_sel'][sh.ring_home == 1] != loc[sh.ring_home == 1]).any()
                       for sh, m, loc in zip(out['shards'], out['masks'], ring_sel_local)), 'a home ring whose set membership comes from another rank'
            assert len(exp['plane_plane']['bgn']) + len(exp['atom_plane']['atom']) > 0
        if name == 'narrow3':
            mid = case.owners(3)[0] == 1
            assert mid.sum() > 10
            for r in (0, 2):
                assert set(np.nonzero(mid)[0].tolist()) <= set(out['shards'][r].global_id.tolist())          # in both neighbours' halos
        assert len(exp['atom_atom']['i']) > 20


def test_designed_inputs_sit_on_their_seams():
    """The conditions the cases of A exist for, checked on the host assembly."""
    for world in (2, 3):
        exact = sc.face_case(world, True)             # atoms and amide centres exactly on the bounds in force, at every bound
        assert exact.tags['on_bound'] == 2 * (world - 1) and len(exact.tags['bounds']) == 2 * (world - 1)
        for i, k, side, bd in exact.tags['bound_atoms'] + exact.tags['bound_amides']:
            assert float(np.float32(bd)) == bd
        assert sum(float(exact.pc.xyz[i, 0]) == bd for i, k, side, bd in exact.tags['bound_atoms']) == 4 * (world - 1)
        assert sum(float(exact.pc.amide_center[i, 0]) == bd for i, k, side, bd in exact.tags['bound_amides']) == 2 * (world - 1)
        case = sc.face_case(world)
        pc, t = case.pc, case.tags
        bounds = sc.face_bounds(case.edges(world))
        assert len(bounds) == 2 * (world - 1)
        for k, side, bd in bounds:
            assert not (float(np.float32(bd)) == bd), 'the bounds are not float32 numbers: no atom can sit on one'
            xs = sorted({float(pc.xyz[i, 0]) for i, kk, s, b in t['bound_atoms'] if (kk, s) == (k, side)})[1:]
            assert len(xs) == 2 and xs[0] < bd < xs[1] and np.nextafter(np.float32(xs[0]), np.float32(np.inf)) == np.float32(xs[1])
            xa = sorted({float(pc.amide_center[i, 0]) for i, kk, s, b in t['bound_amides'] if (kk, s) == (k, side)})[1:]
            assert xa == xs
            xr = sorted(float(pc.ring_center[i, 0]) for i, kk, s, b in t['bound_rings'] if (kk, s) == (k, side))
            assert xr == [np.nextafter(bd, -np.inf), bd, np.nextafter(bd, np.inf)]              # ring centres: on the bound exactly
        for k in range(1, world):
            cut = case.cuts[world][k - 1]
            xs = sorted(x for i, kk, x in t['cut_atoms'] if kk == k)
            assert xs == [float(np.nextafter(np.float32(cut), np.float32(-np.inf))), cut, float(np.nextafter(np.float32(cut), np.float32(np.inf)))]
        a_own = case.owners(world)[0]
        for i, k, x in t['cut_atoms']:
            assert a_own[i] == (k if x >= case.cuts[world][k - 1] else k - 1)
    # the radius case: more distinct pairs than the record header's table holds, in every rank's shard
    case = sc.scan_case(700, 'two', 1, 1, True)
    for sh in sc.host_shards(case, 2, None):      # a shard's table is that of its home records: 0xFFFF is expected on both ranks
        key = np.stack([sh.pc.vdw, sh.pc.cov], axis=1).view(np.uint64)
        home = {tuple(k) for k in key[sh.is_home == 1].tolist()}
        assert sc.rad_capacity() == 256
        assert len(home) > sc.rad_capacity() or any(tuple(k) not in home for k in key[sh.is_home == 0].tolist()), sh.rank
    # the scan cases: counts on the seam, the three carries differ
    case = sc.scan_case(8193, 'two', 0, 0)
    a_own = case.owners(2)[0]
    home = np.nonzero(a_own == 0)[0]
    assert len(home) == 8193
    hc, bc = np.diff(case.pc.h_off)[home], np.diff(case.pc.bond_off)[home]
    assert np.array_equal(hc, np.arange(8193) % 4) and np.array_equal(bc[:8190], np.arange(8190) % 3)
    face = sharding.make_shard_local(case.pc, 0, 2).send_right
    assert np.array_equal(face, home[[4095, 4096]])
