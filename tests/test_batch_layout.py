"""The batch grid (arp_set_batch): where its members are placed, and what runs on top of the placement.

CPU: the placement itself (csrc/arp_batchgrid.h through arp_batch_layout — host arithmetic, served by the host library where
the HIP library is not built) on seeded random boxes and on directed cases that each assert they are what they claim.
GPU: batches on the seams of that placement — adversarial members, the two limits that make the cell edge grow, the fifth
radius that starts a resident batch's grid tables over, and the queries with caller-given centres — every comparison
bit-exact (floats as integer views), no tolerance anywhere.  profiles/batch_layout.md lists the mutants of the placement the
CPU tests were run against and the measured time of every GPU test."""
import numpy as np
import pytest

import batch_cases as bc
from arpeggio_amd import _capi, batch

BAGS = ('atom_plane', 'plane_plane', 'group_group', 'group_plane')
GRID_CELLS = 1 << 26
AXIS_CELLS = 4096


# ===================================================================================================================== CPU
def _stencils_stay_apart(cell, n):
    """No member's cells lie in another member's cell box inflated by one cell on every side — what a 27-cell stencil
    around any of its cells can reach.  (Inflating BOTH boxes would ask for two empty cells between neighbours; the
    placement promises one, and one is what the stencil needs.)  Plain interval tests over all pairs, no shelving logic."""
    lo, hi = cell.astype(np.int64), (cell + n).astype(np.int64)              # half-open [lo, hi)
    ilo, ihi = lo - 1, hi + 1
    overlap = np.ones((len(lo), len(lo)), bool)
    for a in range(3):
        overlap &= (ilo[:, None, a] < hi[None, :, a]) & (lo[None, :, a] < ihi[:, None, a])
    np.fill_diagonal(overlap, False)
    return not overlap.any(), np.argwhere(overlap)[:3]


def _check_layout(boxes, r, L):
    boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
    cell, n, (NX, NY, NZ), edge = L['cell'], L['n'], L['dims'], L['edge']
    assert edge >= r * (1.0 + 1e-6)
    assert np.array_equal(n, (np.floor((boxes[:, 3:] - boxes[:, :3]) / edge) + 1).astype(np.int64)), 'cells per member'
    assert (n >= 1).all() and (n < AXIS_CELLS).all()
    assert NX * NY * NZ <= GRID_CELLS
    assert (cell >= 0).all() and ((cell + n) <= np.array([NX, NY, NZ])).all(), 'a member leaves the grid'
    ok, where = _stencils_stay_apart(cell, n)
    assert ok, ('members within one cell of each other', where.tolist())
    # the grid is no larger than its members need
    assert tuple((cell + n).max(axis=0)) == (NX, NY, NZ)


def _random_boxes(rng, r):
    B = int(rng.integers(1, 21)) if rng.random() < 0.6 else int(rng.integers(21, 301))
    e = bc.EDGE(r)
    kind = rng.integers(0, 7, B)
    ext = np.zeros((B, 3))
    for k in range(B):
        t = kind[k]
        if t == 0:                                                    # a single point
            pass
        elif t == 1:                                                  # a flat, one cell thick
            ext[k] = rng.random(3) * 12 * e
            ext[k, rng.integers(3)] = rng.random() * 0.999 * e
        elif t == 2:                                                  # a needle
            ext[k] = rng.random(3) * 0.999 * e
            ext[k, rng.integers(3)] = rng.random() * 60 * e
        elif t == 3:                                                  # a cube
            ext[k] = rng.random() * 10 * e
        elif t == 4:                                                  # exact multiples of the edge
            ext[k] = rng.integers(0, 9, 3) * e
        elif t == 5:                                                  # some extents of zero
            ext[k] = rng.random(3) * 8 * e * (rng.random(3) < 0.5)
        else:
            ext[k] = rng.random(3) * 15 * e
    lo = (rng.random((B, 3)) - 0.5) * 2000.0
    return np.concatenate([lo, lo + ext], axis=1)


def test_placement_properties_on_random_boxes():
    rng = np.random.default_rng(20240611)
    wrapped_rows = wrapped_layers = 0
    for case in range(3000):
        r = float(rng.choice([0.5, 1.0, 3.0, 5.0, 6.0, 7.5, 12.0])) if case % 2 else float(0.5 + rng.random() * 11.5)
        boxes = _random_boxes(rng, r)
        L = _capi.batch_layout(boxes, r)
        _check_layout(boxes, r, L)
        L2 = _capi.batch_layout(boxes.copy(), r)                       # deterministic
        assert np.array_equal(L['cell'], L2['cell']) and np.array_equal(L['n'], L2['n']) and L['dims'] == L2['dims'] and L['edge'] == L2['edge']
        wrapped_rows += len(np.unique(L['cell'][:, 1])) > 1
        wrapped_layers += len(np.unique(L['cell'][:, 2])) > 1
    assert wrapped_rows > 1000 and wrapped_layers > 300      # the cases are not all single shelves


def test_directed_rows_and_layers():
    r = 5.0
    # seven cubes of 4 cells: vol = 7 * 125 -> side 10: two to a shelf (4 + 1 + 4 <= 10), two shelves to a layer
    boxes = bc.cube_boxes(7, 4, r)
    L = _capi.batch_layout(boxes, r)
    _check_layout(boxes, r, L)
    assert (L['n'] == 4).all() and L['edge'] == bc.EDGE(r)
    first_layer = L['cell'][:, 2] == 0
    assert len(np.unique(L['cell'][first_layer, 1])) >= 2, 'at least two rows'
    assert len(np.unique(L['cell'][:, 2])) >= 2, 'at least two layers'
    # a new row and a new layer begin at x = 0 (and the layer at y = 0), one empty cell beyond the tallest before them
    assert L['cell'][0].tolist() == [0, 0, 0] and L['cell'][1].tolist() == [5, 0, 0] and L['cell'][2].tolist() == [0, 5, 0]
    assert L['cell'][4].tolist() == [0, 0, 5]


def test_directed_members_that_exactly_fill_a_shelf_or_a_layer():
    """Nine members, cell counts chosen by hand so that one ends exactly at the shelf's length, one row exactly at the layer's
    depth, a low row follows a tall one and a shallow layer a deep one.  Expected offsets worked out on paper from the
    description of the placement: members in order along x, a new row one empty cell below the tallest member of the row
    before, a new layer one empty cell behind the deepest member of the layer before, shelf length and layer depth =
    ceil(cbrt(sum of (n + 1) products)) = 10 here."""
    r = 5.0
    cells = np.array([[4, 4, 2], [5, 2, 6], [6, 1, 1], [5, 3, 1], [4, 2, 1], [3, 1, 4], [4, 9, 1], [3, 3, 3], [5, 5, 6]])
    assert 9 ** 3 < (cells + 1).prod(axis=1).sum() <= 10 ** 3 and cells[:, :2].max() <= 10
    boxes = np.concatenate([np.zeros((9, 3)), (cells - 0.5) * bc.EDGE(r)], axis=1)
    L = _capi.batch_layout(boxes, r)
    _check_layout(boxes, r, L)
    assert np.array_equal(L['n'], cells)
    expect = [[0, 0, 0], [5, 0, 0],      # 5 + 5 = 10: still on the shelf
              [0, 5, 0],                 # below the TALLER of the two (4 cells + 1)
              [0, 7, 0],                 # below a row one cell high (not below the first row's height again); 7 + 3 = 10: still in the layer
              [6, 7, 0],                 # 6 + 4 = 10
              [0, 0, 7],                 # behind the deepest of the first layer (6 cells + 1)
              [4, 0, 7],
              [0, 0, 12],                # behind a layer 4 cells deep (not 6 again)
              [4, 0, 12]]
    assert L['cell'].tolist() == expect and L['dims'] == (10, 10, 18)


def test_directed_axis_limit_grows_the_edge():
    r = 5.0
    boxes = np.array([[0, 0, 0, 30, 30, 30], [0, 0, 0, 4095 * bc.EDGE(r) + 1.0, 8, 8], [5, 5, 5, 25, 40, 25]], float)
    assert np.floor(boxes[1, 3] / bc.EDGE(r)) + 1 >= AXIS_CELLS, 'the member has 4096 cells at the asked radius'
    L = _capi.batch_layout(boxes, r)
    _check_layout(boxes, r, L)
    assert L['edge'] == bc.EDGE(r) * 1.26 and L['n'][1, 0] < AXIS_CELLS
    # one cell fewer: no growth
    boxes[1, 3] = 4094 * bc.EDGE(r) + 1.0
    L = _capi.batch_layout(boxes, r)
    _check_layout(boxes, r, L)
    assert L['edge'] == bc.EDGE(r) and L['n'][1, 0] == 4095


def test_directed_three_needles_grow_the_edge_several_steps():
    r = 5.0
    boxes = bc.needle_boxes()
    n0 = np.floor((boxes[:, 3:] - boxes[:, :3]) / bc.EDGE(r)) + 1
    assert (n0 < AXIS_CELLS).all() and n0.max() ** 3 > 100 * GRID_CELLS, 'no axis limit; a common grid far beyond 2^26 cells'
    L = _capi.batch_layout(boxes, r)
    _check_layout(boxes, r, L)
    steps = np.log(L['edge'] / bc.EDGE(r)) / np.log(1.26)
    assert abs(steps - round(steps)) < 1e-9 and round(steps) >= 3, steps
    assert np.prod(L['dims']) > GRID_CELLS / 1.26 ** 3 / 1.5, 'the growth stopped as soon as the grid fitted'


def test_directed_single_member_and_wide_member():
    r = 6.0
    boxes = np.array([[-3.0, 4.0, 9.0, 40.0, 4.0, 30.0]])
    L = _capi.batch_layout(boxes, r)
    _check_layout(boxes, r, L)
    assert L['cell'].tolist() == [[0, 0, 0]] and L['dims'] == tuple(L['n'][0].tolist()) and L['n'][0, 1] == 1
    # a member wider than the cube root of the volume: the shelf is as long as that member
    boxes = np.concatenate([bc.cube_boxes(5, 3, r), [[0, 0, 0, 200.5 * bc.EDGE(r), 2.0, 2.0]], bc.cube_boxes(4, 3, r)])
    L = _capi.batch_layout(boxes, r)
    _check_layout(boxes, r, L)
    vol = ((L['n'] + 1).prod(axis=1)).sum()
    assert L['n'][5, 0] == 201 and L['n'][5, 0] > np.ceil(np.cbrt(vol)) and L['dims'][0] == 201
    assert L['cell'][5, 0] == 0, 'the wide member begins a shelf'
    # no members at all, and boxes the library refuses
    assert _capi.batch_layout(np.zeros((0, 6)), r)['dims'] == (1, 1, 1)
    for bad in ([[0, 0, 0, 1, -1, 1]], [[0, 0, 0, np.inf, 1, 1]], [[np.nan, 0, 0, 1, 1, 1]], [[-1e308, 0, 0, 1e308, 1, 1]]):
        with pytest.raises(ValueError):
            _capi.batch_layout(np.array(bad, float), r)


def test_the_gpu_batches_are_what_they_claim():
    """The wrap and growth claims of the GPU cases below, asserted where no GPU is needed."""
    pcs, boxes, tags = bc.adversarial_members()
    assert 38 <= len(pcs) <= 45 and sum(p.n_atoms for p in pcs) < 5000
    own = bc.own_boxes(pcs)
    for r in (5.0, 6.0, 7.5):
        L = _capi.batch_layout(boxes, r)
        _check_layout(boxes, r, L)
        assert L['edge'] == bc.EDGE(r)
        assert len(np.unique(L['cell'][L['cell'][:, 2] == 0, 1])) >= 2 and len(np.unique(L['cell'][:, 2])) >= 2, 'a row and a layer wrap'
    c = tags['corners'][0]
    x = pcs[c].xyz.astype(np.float64)
    assert np.array_equal(x[1], own[c, 3:]) and np.array_equal(x[0], own[c, :3]), 'the second atom is the max corner of its box'
    assert 4.98 < np.linalg.norm(x[1] - x[0]) < 5.0
    assert pcs[tags['one_atom'][0]].n_atoms == 1 and pcs[tags['planes_only'][0]].n_atoms == 0 and pcs[tags['planes_only'][0]].n_rings > 0
    for name, axis in (('flat', 2), ('needle', 1), ('needle', 2)):
        k = tags[name][0]
        assert (own[k, 3 + axis] - own[k, axis]) < 4.5 and _capi.batch_layout(boxes, 5.0)['n'][k, axis] == 1, 'one cell thick'
    m = tags['multiple'][0]
    assert (boxes[m, 3:] - boxes[m, :3]).tolist() == [3 * bc.EDGE(5.0), 2 * bc.EDGE(7.5), bc.EDGE(6.0)]
    i3 = tags['identical']
    assert len(i3) == 3 and all(np.array_equal(pcs[i3[0]].xyz, pcs[k].xyz) for k in i3)
    lg, sm = tags['box_larger'][0], tags['box_smaller'][0]
    assert (boxes[lg, :3] < own[lg, :3] - 5).all() and (boxes[lg, 3:] > own[lg, 3:] + 5).all()
    xs = pcs[sm].xyz.astype(np.float64)
    outside = ((xs < boxes[sm, :3]) | (xs > boxes[sm, 3:])).any(axis=1)
    assert outside.sum() > pcs[sm].n_atoms // 2, 'most atoms of the member lie outside its declared box'
    # the two limits
    pcs, boxes = bc.axis_limit_batch()
    assert np.floor((boxes[1, 3] - boxes[1, 0]) / bc.EDGE(5.0)) + 1 >= AXIS_CELLS
    L = _capi.batch_layout(boxes, 5.0)
    _check_layout(boxes, 5.0, L)
    assert L['edge'] > bc.EDGE(5.0)
    pcs, boxes = bc.three_needles_batch()
    n0 = np.floor((boxes[:, 3:] - boxes[:, :3]) / bc.EDGE(5.0)) + 1
    assert (n0 < AXIS_CELLS).all() and sorted(n0.max(axis=0).tolist()) == [3000, 3000, 3000]
    L = _capi.batch_layout(boxes, 5.0)
    _check_layout(boxes, 5.0, L)
    assert L['edge'] >= bc.EDGE(5.0) * 1.26 ** 3
    # the query members: two boxes that overlap in world coordinates, one far away
    pc, xyz, _, _ = bc.overlapping_members()
    lo, hi = xyz.min(axis=1).astype(np.float64), xyz.max(axis=1).astype(np.float64)
    assert (lo[0] < hi[1]).all() and (lo[1] < hi[0]).all() and (lo[2] > hi[0] + 100).any()


# ===================================================================================================================== GPU
def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        if x.dtype.kind == 'f':
            assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint64), y.view(np.uint32 if y.dtype == np.float32 else np.uint64)), (what, k)
        else:
            assert np.array_equal(x, y), (what, k)


def _declare(ctx, pcs, boxes, selections=None):
    big, off = batch.concat_complexes(pcs)
    off['boxes'] = np.ascontiguousarray(boxes, np.float64)
    ctx.set_complex(big)
    ctx.declare_batch(off)
    if selections is not None:
        ctx.set_selection(np.concatenate(selections).astype(np.uint8))
    return big, off


def _single(ctx, pc, params, sel=None):
    ctx.set_complex(pc)
    if sel is not None:
        ctx.set_selection(sel)
    counts = ctx.run_launch(*params)
    out = dict(atom_atom=ctx.atom_contacts_fetch(counts['atom_atom']))
    for b in BAGS:
        out[b] = ctx.fetch_bag(b)
    return out


def _five(ctx, counts):
    out = dict(atom_atom=ctx.atom_contacts_fetch(counts['atom_atom']))
    for b in BAGS:
        out[b] = ctx.fetch_bag(b)
    return out


@pytest.fixture()
def two_contexts():
    a, b = _capi.Context(0), _capi.Context(0)
    yield a, b
    a.close()
    b.close()


ORACLE_IDS = {'atom_plane': ('atom', 'ring'), 'plane_plane': ('bgn', 'end'), 'group_group': ('bgn', 'end'), 'group_plane': ('amide', 'ring')}


@pytest.mark.gpu
def test_adversarial_members_equal_their_single_runs_and_the_oracle(two_contexts):
    """3a.  Every member's five bags against its own run on a second context (bit for bit) and, for the special members,
    against the oracle by brute force: the atom-atom bag whole (distances as bits), the ring / amide bags by their ids and
    types (the float columns of those are held against the single run, which shares no grid with the batch)."""
    import oracle
    ctx, other = two_contexts
    pcs, boxes, tags = bc.adversarial_members()
    _declare(ctx, pcs, boxes)
    special = sorted(k for name, ks in tags.items() if name != 'filler' for k in ks)
    n_rec = 0
    for params in ((5.0, 0.1, False, 6.0), (7.5, 0.1, False, 6.0)):
        got = ctx.run_batch(*params)
        assert len(got) == len(pcs)
        for k, pc in enumerate(pcs):
            single = _single(other, pc, params)
            for name in ('atom_atom',) + BAGS:
                _same(got[k][name], single[name], (params[0], k, name))
            n_rec += len(single['atom_atom']['i'])
        for k in special:
            oc = oracle.OracleComplex(pcs[k])
            oc.make_selection(None)
            exp = oc.atom_contacts(params[0], params[1], params[2], use_grid=False)
            aa = got[k]['atom_atom']
            for col in ('i', 'j', 'sift', 'ctype'):
                assert np.array_equal(aa[col], exp[col]), (params[0], k, col)
            assert np.array_equal(aa['dist'].view(np.uint32), exp['dist'].view(np.uint32)), (params[0], k)
            for name, exp in (('atom_plane', oc.atom_plane()), ('plane_plane', oc.plane_plane()), ('group_group', oc.group_group()),
                              ('group_plane', oc.group_plane())):
                for col in ORACLE_IDS[name] + ('ctype',):
                    assert np.array_equal(got[k][name][col], exp[col]), (params[0], k, name, col)
    c = tags['corners'][0]
    assert len(got[c]['atom_atom']['i']) == 1, 'the pair across the box diagonal'
    assert n_rec > 20_000


def _limit_case(two_contexts, pcs, boxes, params):
    ctx, other = two_contexts
    _declare(ctx, pcs, boxes)
    got = ctx.run_batch(*params)
    L = _capi.batch_layout(boxes, params[0])
    assert ctx.stats()['cells'] == int(np.prod(L['dims'])) and L['edge'] > params[0]
    assert L['edge'] > bc.EDGE(params[0]), 'the edge grew'
    n_rec = 0
    for k, pc in enumerate(pcs):
        single = _single(other, pc, params)
        for name in ('atom_atom',) + BAGS:
            _same(got[k][name], single[name], (k, name))
        n_rec += len(single['atom_atom']['i'])
    assert n_rec > 500
    return L


@pytest.mark.gpu
def test_member_of_4096_cells_grows_the_edge(two_contexts):
    """3b.  A member with two clusters 25 000 A apart beside two ordinary ones."""
    pcs, boxes = bc.axis_limit_batch()
    _limit_case(two_contexts, pcs, boxes, (5.0, 0.1, False, 6.0))


@pytest.mark.gpu
def test_three_needles_grow_the_edge_to_the_cell_limit(two_contexts):
    """3b.  Three needles along x, y and z: the common grid is held to 2^26 cells (histograms of a few hundred MB)."""
    pcs, boxes = bc.three_needles_batch()
    L = _limit_case(two_contexts, pcs, boxes, (5.0, 0.1, False, 6.0))
    assert np.prod(L['dims']) > GRID_CELLS // 8


# ---- 3c: a fifth radius on a resident batch -----------------------------------------------------------------------------
CUTOFFS = (4.0, 4.5, 5.0, 5.5, 6.5, 7.5)
EXPANDS = (6.0, 7.0, 8.0, 9.0)


def _eviction_sequence():
    """(cutoff, expand radius) of 14 passes, seeded; passes 5 and 11 repeat the cutoff of the pass before them with an expand
    radius that no pass before used, and earlier radii come back."""
    rng = np.random.default_rng(63)
    seq = [(5.0, 6.0), (4.0, 6.0), (6.5, 7.0), (4.5, 7.0)]
    seq.append((4.5, 8.0))                                  # pass 5: cutoff of pass 4 (cached), a new expand radius
    for _ in range(5):
        seq.append((float(rng.choice(CUTOFFS)), float(rng.choice(EXPANDS[:3]))))
    seq.append((seq[-1][0], 9.0))                           # pass 11: the same again, 9.0 is new
    seq += [(5.0, 6.0), (7.5, 8.0), (4.0, 9.0)]
    return seq, (4, 10)


def _partial_selections(pcs, seed=9):
    rs = np.random.RandomState(seed)
    sels = []
    for pc in pcs:
        m = np.zeros(pc.n_atoms, np.uint8)
        picked = rs.choice(pc.n_residues, size=max(2, pc.n_residues // 6), replace=False)
        m[np.isin(pc.res_id, picked)] = 1
        sels.append(m)
    return sels


def _results(ctx, params, complete):
    from arpeggio_amd import contact_filter
    counts = ctx.run_launch(*params)
    out = _five(ctx, counts)
    acc = ctx.atom_accumulators()
    out['acc'] = dict(sift=acc['sift'], counts=acc['counts'])
    if complete:
        out['residue_pairs'] = ctx.residue_pairs()
        out['water_bridges'] = ctx.water_bridges(contact_filter.SPECIFIC[0])
    return out


def _compare_results(a, b, what):
    assert set(a) == set(b)
    for name in a:
        _same(a[name], b[name], (what, name))


@pytest.mark.gpu
def test_fifth_radius_on_a_resident_batch(two_contexts):
    """3c.  One batch, declared once; fourteen passes whose radii outnumber the four cached tables.  After every pass the
    results equal those of a fresh declaration given that pass alone."""
    ctx, other = two_contexts
    pcs, boxes = bc.eviction_batch()
    sels = _partial_selections(pcs)
    seq, repeats = _eviction_sequence()
    assert len(seq) >= 12 and len({e for _, e in seq}) == 4 and len({c for c, _ in seq}) >= 4
    for k in repeats:
        assert seq[k][0] == seq[k - 1][0] and all(seq[k][1] != e for _, e in seq[:k]), k
    _declare(ctx, pcs, boxes, sels)
    assert ctx.stats()['batch_restarts'] == 0
    n_rec = 0
    for k, (cutoff, expand) in enumerate(seq):
        params = (cutoff, 0.1, False, expand)
        before = ctx.stats()['batch_restarts']
        got = _results(ctx, params, complete=False)
        rose = ctx.stats()['batch_restarts'] - before
        if k in repeats:
            assert rose >= 1, ('the tables started over in a pass whose cutoff was cached', k)
        _declare(other, pcs, boxes, sels)
        _compare_results(got, _results(other, params, complete=False), (k, params))
        n_rec += len(got['atom_atom']['i'])
    assert ctx.stats()['batch_restarts'] >= 3
    assert n_rec > 10_000


@pytest.mark.gpu
def test_fifth_cutoff_on_a_resident_whole_structure_batch(two_contexts):
    """3c.  The same sequence with every atom selected, arp_set_whole_structure and grid reuse on: only the cutoff varies
    (and 6 A for the ring / amide grids); the passes are complete, so the residue-pair table and the water bridges are
    compared too."""
    ctx, other = two_contexts
    pcs, boxes = bc.eviction_batch()
    seq, _ = _eviction_sequence()
    for c in (ctx, other):
        c.set_grid_reuse(True)
    _declare(ctx, pcs, boxes)
    ctx.set_whole_structure(True)
    for k, (cutoff, _) in enumerate(seq):
        params = (cutoff, 0.1, False, 6.0)
        got = _results(ctx, params, complete=True)
        _declare(other, pcs, boxes)
        other.set_whole_structure(True)
        _compare_results(got, _results(other, params, complete=True), (k, params))
        assert len(got['residue_pairs']['res_a']) > 100
    assert ctx.stats()['batch_restarts'] >= 1


@pytest.mark.gpu
def test_search_all_radii_between_two_passes(two_contexts):
    """3c.  search_all at three new radii between two identical passes: the tables start over under the second pass's grids,
    and it must equal the first."""
    ctx, _ = two_contexts
    pcs, boxes = bc.eviction_batch()
    _declare(ctx, pcs, boxes, _partial_selections(pcs))
    params = (5.0, 0.1, False, 7.0)
    first = _results(ctx, params, complete=False)
    pairs = [ctx.search_all(r) for r in (3.5, 4.25, 8.5)]
    assert all(len(p[0]) > 0 for p in pairs) and len(pairs[2][0]) > len(pairs[0][0])
    assert ctx.stats()['batch_restarts'] >= 1
    _compare_results(first, _results(ctx, params, complete=False), 'after search_all')
    _compare_results(first, _results(ctx, params, complete=False), 'once more')


# ---- 3d: queries on a resident batch and on resident models -----------------------------------------------------------
def _query_centres(xyz):
    """Inside each member, between members, on box faces, 500 A outside (as test_search_around_centres_equals_brute_force)."""
    rng = np.random.default_rng(3)
    x = xyz.astype(np.float64)
    parts = []
    for m in x:
        lo, hi = m.min(axis=0), m.max(axis=0)
        parts += [lo + rng.random((60, 3)) * (hi - lo), m[rng.choice(len(m), 20)], [lo, hi, lo - 2.0, hi + 3.9, [lo[0], hi[1], (lo[2] + hi[2]) / 2]]]
    mid01, mid02 = (x[0].mean(axis=0) + x[1].mean(axis=0)) / 2, (x[0].mean(axis=0) + x[2].mean(axis=0)) / 2
    parts += [[mid01, mid02, x.reshape(-1, 3).max(axis=0) + 500.0, x.reshape(-1, 3).min(axis=0) - 500.0], x[0][:5] + [3.0, 0.0, 0.0]]
    return np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p in parts])


def _check_queries(ctx, xyz_all, res_all, member_pairs, offsets):
    from oracle import ref_py
    x = xyz_all.astype(np.float64)
    centres = _query_centres(xyz_all.reshape(3, -1, 3))
    before = _five(ctx, ctx.run_launch())
    n_hits = 0
    for radius in (3.0, 6.0, 9.5):
        oc, oa = ctx.search(centres, radius)
        d = x[None, :, :] - centres[:, None, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        ec, ea = np.nonzero(d2 <= radius * radius)
        assert np.array_equal(oc, ec) and np.array_equal(oa, ea), radius
        n_hits += len(ec)
        # hits in every member, and centres that see atoms of two members at once
        member = np.searchsorted(offsets, ea, side='right') - 1
        assert set(member.tolist()) == {0, 1, 2}
        if radius > 3.0:
            assert any(len(set(member[ec == c].tolist())) > 1 for c in np.unique(ec)), 'a centre with hits in two members'
    assert n_hits > 3000
    res, dist = ctx.ring_residues(centres)
    eres, edist = ref_py.ring_residues(xyz_all, res_all, centres)
    assert np.array_equal(res, eres) and (eres >= 0).sum() > 50 and (eres < 0).sum() > 3
    assert np.array_equal(dist.view(np.uint64), edist.view(np.uint64))
    # search_all: a batch is independent structures — exactly each member's own pairs, although pairs across the
    # overlapping members exist in world coordinates
    gi, gj = ctx.search_all(5.0)
    ei = np.concatenate([p[0] + offsets[k] for k, p in enumerate(member_pairs)])
    ej = np.concatenate([p[1] + offsets[k] for k, p in enumerate(member_pairs)])
    o = np.lexsort((ej, ei))
    assert np.array_equal(gi, ei[o]) and np.array_equal(gj, ej[o])
    n0 = offsets[1]
    d = x[:n0, None, :] - x[None, n0:2 * n0, :]
    cross = ((d * d).sum(axis=2) <= 25.0).sum()
    assert cross > 100, 'pairs across members exist by brute force over the world coordinates'
    _compare_results(before, _five(ctx, ctx.run_launch()), 'the pass after the queries')


def _brute_pairs(xyz, radius):
    x = xyz.astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    i, j = np.nonzero(np.triu(d2 <= radius * radius, 1))
    return i.astype(np.int64), j.astype(np.int64)


@pytest.mark.gpu
def test_centre_queries_on_a_resident_batch(two_contexts):
    """3d.  search / ring_residues with caller-given centres answer over ALL resident atoms in world coordinates; search_all
    keeps the members apart; the pass after them equals the pass before."""
    ctx, _ = two_contexts
    pc, xyz, h_xyz, pcs = bc.overlapping_members()
    big, off = _declare(ctx, pcs, bc.own_boxes(pcs))
    _check_queries(ctx, big.xyz, big.res_id, [_brute_pairs(p.xyz, 5.0) for p in pcs], off['atom'])


@pytest.mark.gpu
def test_centre_queries_on_resident_models(two_contexts):
    """3d.  The same three coordinate sets as F = 3 models of one topology."""
    ctx, _ = two_contexts
    pc, xyz, h_xyz, _ = bc.overlapping_members()
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    n = pc.n_atoms
    res_all = np.concatenate([pc.res_id + f * pc.n_residues for f in range(3)]).astype(np.int32)
    _check_queries(ctx, xyz.reshape(-1, 3), res_all, [_brute_pairs(xyz[f], 5.0) for f in range(3)], np.arange(4) * n)
