"""The grid build of a whole-structure pass reads its block bases from a table made from the spatial order (k_keep_bases,
k_compact_atoms<ROWS, true>) instead of looking back over the blocks before — from the second such build over an order on: the
first one looks back, and a structure that is evaluated once never pays for the table.  Every case runs the pass both ways in ONE context
— the static order is the same then, so even the order of the records inside a cell is — and compares, bit for bit: the five
bags in canonical order, the statistics, selection_plus and the ring / amide sets made from the residue sets, and the start
table of the grid.  Which way a build went is read back (ARP_BUF_KEEP_BASE answers only after a build that read the table).

The table itself is held against a NumPy prefix sum on structures whose cells are all hydrogens or none (the order of the rows
inside a cell is not fixed, their number per cell is), and against what every structure allows: it starts at zero, never falls,
rises by at most a block's rows, and ends at the atoms the pass binned.

The 1024-row variant is reached in process by no structure this small: the `compact_1024` configuration of
test_gpu_paths.py runs its corpus through it (whole passes there read a table of 1024-row blocks) against the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

BAGS = ('atom_plane', 'plane_plane', 'group_group', 'group_plane')
ROWS = 512          # rows per block of k_compact_atoms up to 150 000 atoms


@pytest.fixture(scope='module')
def capi():
    from arpeggio_amd import _capi
    return _capi


@pytest.fixture(scope='module')
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def hip(capi):
    """The HIP runtime the library runs on (device -> host copies of the two debug buffers)."""
    capi.load()
    for line in open('/proc/self/maps'):
        if 'libamdhip64' in line:
            L = C.CDLL(line.split()[-1])
            L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return L
    raise RuntimeError('the HIP runtime is not loaded')


def _read_i32(hip, cx, which):
    ptr, nb = cx.device_buffer(which)
    out = np.empty(nb // 4, np.int32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), nb, 2) == 0      # device -> host
    return out


def _table(hip, cx):
    """The table the last grid build read, or None if it looked back."""
    try:
        return _read_i32(hip, cx, cx.BUF_KEEP_BASE)
    except ValueError:
        return None


def _snapshot(hip, cx, cutoff=5.0, comp=0.1, seq=False):
    counts = cx.run_launch(cutoff, comp, seq)
    snap = {'counts': dict(counts), 'stats': cx.stats(), 'mask': cx.make_selection_masks(),
            'start': _read_i32(hip, cx, cx.BUF_GRID_START), 'table': _table(hip, cx),
            'atom_atom': cx.atom_contacts_fetch(counts['atom_atom'])}
    for bag in BAGS:
        snap[bag] = cx.fetch_bag(bag)
    return snap


def _assert_same(a, b, where):
    assert a['counts'] == b['counts'], (where, a['counts'], b['counts'])
    for k in ('binned', 'cells', 'candidates', 'accepted', 'emitted'):
        assert a['stats'][k] == b['stats'][k], (where, k, a['stats'], b['stats'])
    for m in a['mask']:
        assert np.array_equal(a['mask'][m], b['mask'][m]), (where, 'mask', m)
    assert np.array_equal(a['start'], b['start']), (where, 'start table')
    for bag in ('atom_atom',) + BAGS:
        assert a[bag].keys() == b[bag].keys()
        for col in a[bag]:
            x, y = np.ascontiguousarray(a[bag][col]), np.ascontiguousarray(b[bag][col])
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (where, bag, col)


def _check_table(tab, n, binned, where):
    assert tab is not None, (where, 'the build looked back')
    nb = (n + ROWS - 1) // ROWS
    assert tab.shape == (nb + 1,), (where, tab.shape)
    assert tab[0] == 0 and tab[-1] == binned, (where, tab[0], tab[-1], binned)
    d = np.diff(tab)
    assert np.all(d >= 0) and np.all(d <= ROWS), (where, d.min(), d.max())


def _both_ways(hip, cx, n, where, **kw):
    """The first pass over a new order (it looks back), one by the table, one with the look-back forced, one by the table again;
    all equal.  Returns the table."""
    cx.set_grid_reuse(False)
    cx.set_compact_lookback(False)
    first = _snapshot(hip, cx, **kw)      # (no table yet, unless the pass ran twice: a contact list that outgrew its buffers)
    a = _snapshot(hip, cx, **kw)
    _check_table(a['table'], n, a['stats']['binned'], where)
    cx.set_compact_lookback(True)
    b = _snapshot(hip, cx, **kw)
    assert b['table'] is None, (where, 'look-back was asked for')
    cx.set_compact_lookback(False)
    c = _snapshot(hip, cx, **kw)
    _assert_same(first, b, (where, 'first'))
    _assert_same(a, b, where)
    _assert_same(c, b, (where, 'again'))
    assert np.array_equal(a['table'], c['table']), where
    return a['table']


def _soup(n, seed, hyd=0.3):
    """n atoms of every type at protein density, `hyd` of them hydrogens (as atoms: F_HYDROGEN), three atoms per residue, some
    hydrogens attached to donors, a few rings and amides with residues of their own."""
    from arpeggio_amd.core import config
    from helpers import tiny_complex
    rng = np.random.default_rng(seed)
    box = max(6.0, (n / 0.1) ** (1.0 / 3.0))
    xyz = (rng.random((n, 3)) * box).astype(np.float32)
    tm = np.zeros(n, np.uint16)
    for b in range(12):
        tm |= ((rng.random(n) < 0.3).astype(np.uint16) << b)
    tm &= ~np.uint16(config.ATOM_TYPE_BIT['xbond donor'])      # (they need a bonded neighbour, and nothing here is bonded)
    fl = (rng.random(n) < 0.4).astype(np.uint16) * config.F_ELEM_C
    fl |= (rng.random(n) < 0.1).astype(np.uint16) * config.F_WATER
    is_h = rng.random(n) < hyd
    fl[is_h] = config.F_HYDROGEN
    res_id = (np.arange(n) // 3).astype(np.int32)
    nres = int(res_id.max()) + 1
    h = {}
    for i in np.nonzero(rng.random(n) < 0.3)[0].tolist():
        v = rng.standard_normal((1 + i % 2, 3))
        h[i] = (xyz[i].astype(np.float64) + v / np.linalg.norm(v, axis=1, keepdims=True)).tolist()
    nr, na = max(1, n // 40), max(1, n // 30)

    def planes(k, dt):
        c = (rng.random((k, 3)) * box).astype(dt)
        v = rng.standard_normal((k, 3))
        return c, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dt), rng.integers(0, nres, k).astype(np.int32)
    return tiny_complex(xyz, vdw=rng.choice([1.2, 1.52, 1.7, 1.8], n), cov=rng.choice([0.31, 0.66, 0.76, 1.05], n), type_mask=tm, flags=fl,
                        res_id=res_id, res_flags=np.full(nres, config.R_POLYPEPTIDE | config.R_HAS_SEQ, np.uint8),
                        res_prev=np.arange(nres) - 1, res_next=np.where(np.arange(nres) < nres - 1, np.arange(nres) + 1, -1), h=h,
                        rings=planes(nr, np.float64), amides=planes(na, np.float32))


def _chain(hydrogen_clusters, n_clusters=220, per=7, seed=5):
    """Clusters of `per` atoms every 10 A along x, 3 A across: a cell (5 A) holds atoms of one cluster only, the cells go with
    x, and most cells are empty.  The clusters named are hydrogens throughout, so every cell is hydrogens or none and the rows
    before each block are known whatever order a cell's atoms took.  220 x 7 = 1540 rows: three blocks and a few rows."""
    from arpeggio_amd.core import config
    from helpers import tiny_complex
    rng = np.random.default_rng(seed)
    n = n_clusters * per
    cl = np.arange(n) // per
    xyz = (rng.random((n, 3)) * 3.0).astype(np.float32)
    xyz[:, 0] += (10.0 * cl).astype(np.float32)
    order = rng.permutation(n)            # (the upload order says nothing about the cells)
    xyz, cl = xyz[order], cl[order]
    is_h = np.isin(cl, np.asarray(list(hydrogen_clusters), np.int64))
    fl = np.where(is_h, config.F_HYDROGEN, config.F_ELEM_C).astype(np.uint16)
    tm = (rng.integers(0, 1 << 12, n) & ~int(config.ATOM_TYPE_BIT['xbond donor'])).astype(np.uint16)
    pc = tiny_complex(xyz, type_mask=tm, flags=fl, res_id=(np.arange(n) // 2).astype(np.int32))
    kept_sorted = (~is_h[np.argsort(cl, kind='stable')]).astype(np.int64)
    nb = (n + ROWS - 1) // ROWS
    pre = np.concatenate([[0], np.cumsum(kept_sorted)])
    expect = pre[np.minimum(np.arange(nb + 1) * ROWS, n)].astype(np.int32)
    return pc, expect


@pytest.mark.parametrize('n', [1, 63, 64, 65, 511, 512, 513, 1023, 1025])
def test_row_counts_around_one_wave_and_one_block(ctx, hip, n):
    pc = _soup(n, seed=100 + n)
    ctx.set_complex(pc)
    _both_ways(hip, ctx, n, ('soup', n))
    assert n < 63 or ctx.stats()['emitted'] > 0
    _both_ways(hip, ctx, n, ('soup', n, '4 A'), cutoff=4.0)      # another cell edge: a new order, a new table


# clusters per block: 512 / 7 = 73.14 — cluster 73 lies across the first block boundary, 146 across the second, 219 across the third
CHAINS = {
    'no_hydrogens': (),
    'a_whole_block_of_hydrogens': range(73, 147),              # rows 511 ... 1028: block 1 keeps nothing
    'first_block_hydrogens': range(0, 74),
    'last_blocks_hydrogens': range(146, 220),                  # the last kept row lies before 740 cells that keep nothing
    'all_hydrogens': range(0, 220),
    'every_third_cluster': range(0, 220, 3),
    'only_the_last_cluster_kept': range(0, 219),
}


@pytest.mark.parametrize('name', list(CHAINS))
def test_blocks_of_hydrogens_and_the_table_against_a_prefix_sum(ctx, hip, name):
    pc, expect = _chain(CHAINS[name])
    ctx.set_complex(pc)
    tab = _both_ways(hip, ctx, pc.n_atoms, name)
    assert np.array_equal(tab, expect), (name, tab, expect)


def test_protein_in_its_box_a_batch_of_two_and_two_models(capi, hip):
    """Runs of empty cells between kept rows (a protein in its bounding box, explicit hydrogens among its atoms); two structures
    side by side with an empty layer of cells between them; two models of one topology."""
    from arpeggio_amd import synth
    from arpeggio_amd.core import config
    cx = capi.Context(0)
    prot = synth.proteinlike(n_res=150, n_waters=60, seed=72)
    assert ((prot.flags & config.F_HYDROGEN) != 0).sum() > 500
    cx.set_complex(prot)
    _both_ways(hip, cx, prot.n_atoms, 'proteinlike')
    other = synth.proteinlike(n_res=90, n_waters=20, seed=73)
    cx.set_batch([prot, other])
    _both_ways(hip, cx, prot.n_atoms + other.n_atoms, 'batch of two')
    top = synth.make_synthetic(700, seed=9, box=(28.0, 28.0, 28.0), n_rings=12, n_amides=16)
    top.flags[::5] = config.F_HYDROGEN
    xyz, h_xyz = synth.models_of(top, 2, seed=4, jitter=0.2)
    cx.set_topology(top)
    cx.set_models(xyz, h_xyz)
    _both_ways(hip, cx, 2 * top.n_atoms, 'two models')
    cx.close()


def test_the_table_follows_the_structure_and_steps_aside_for_other_selections(capi, hip):
    """whole pass -> ligand selection (look-back; against the oracle) -> whole pass -> new hydrogens by the setter -> whole
    pass -> new atoms -> whole pass, each pass run twice (the second build over an order is the one that makes and reads the
    table): every pass equals the same pass on a fresh context given the same inputs, and the whole passes read a table that
    belongs to the structure of the moment."""
    import oracle
    from arpeggio_amd.core import config
    from helpers import assert_planes_equal
    cx = capi.Context(0)
    cx.set_grid_reuse(False)
    pc = _soup(1300, seed=7)
    sel = (pc.res_id % 11 == 4).astype(np.uint8)
    h2 = np.asarray(pc.h_xyz, np.float64) + 0.05
    pc2 = _soup(1300, seed=7)
    pc2.flags[:] = np.roll(pc.flags, 97)            # the same atoms, other hydrogens among them
    pc3 = _soup(900, seed=8, hyd=0.1)

    def fresh(setup):
        f = capi.Context(0)
        f.set_grid_reuse(False)
        setup(f)
        s = _snapshot(hip, f), _snapshot(hip, f)
        f.close()
        return s

    def step(setup_more, all_setup, whole, where):
        setup_more(cx)
        got = _snapshot(hip, cx), _snapshot(hip, cx)
        want = fresh(all_setup)
        for k in (0, 1):
            _assert_same(got[k], want[k], (where, k))
            if not whole:
                assert got[k]['table'] is None and want[k]['table'] is None, (where, 'a partial selection reads no table')
        if whole:
            _check_table(got[1]['table'], cx.n, got[1]['stats']['binned'], where)
            _check_table(want[1]['table'], cx.n, want[1]['stats']['binned'], (where, 'fresh'))
        return got[1]

    def hydrogens(c, hx):
        c._check(c._L.arp_set_hydrogens(c._h, capi._p(pc.h_off), capi._p(hx)), 'arp_set_hydrogens')

    step(lambda c: c.set_complex(pc), lambda c: c.set_complex(pc), True, 'whole')
    got = step(lambda c: c.set_selection(sel), lambda c: (c.set_complex(pc), c.set_selection(sel)), False, 'ligand')
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel)
    exp = oc.atom_contacts(5.0, 0.1, False)
    assert np.array_equal(got['mask']['plus'], plus)
    for k in ('i', 'j', 'sift', 'ctype'):
        assert np.array_equal(got['atom_atom'][k], exp[k]), k
    assert np.array_equal(got['atom_atom']['dist'].view(np.uint32), exp['dist'].view(np.uint32))
    ones = np.ones(pc.n_atoms, np.uint8)
    step(lambda c: c.set_selection(ones), lambda c: (c.set_complex(pc), c.set_selection(ones)), True, 'whole again')
    step(lambda c: hydrogens(c, h2), lambda c: (c.set_complex(pc), hydrogens(c, h2)), True, 'new hydrogens')
    a = step(lambda c: c.set_complex(pc2), lambda c: c.set_complex(pc2), True, 'new atoms, as many')
    assert a['stats']['binned'] == int(((pc2.flags & config.F_HYDROGEN) == 0).sum())
    b = step(lambda c: c.set_complex(pc3), lambda c: c.set_complex(pc3), True, 'new atoms, fewer')
    assert b['stats']['binned'] == int(((pc3.flags & config.F_HYDROGEN) == 0).sum())
    cx.close()
