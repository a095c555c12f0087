"""Only the atom-atom records a caller asks for: the bag filtered on the device, then sorted and fetched
(arp_contacts_filter_launch / arp_fetch_packed_filtered, Context.contacts_filter / fetch_packed_filtered,
arpeggio_amd.contact_filter, InteractionComplex.set_contact_filter).

The yardstick is never the new code: it is the canonical bag ``fetch_packed()`` returns — and once the oracle's bag —
masked with the plain NumPy expression of ``_masked`` below.  Every column is compared as bytes.  No tolerance anywhere."""
import copy
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, batch, contact_filter, synth
from arpeggio_amd.core import config
from helpers import tiny_complex
from test_models import _same
from test_persistence import PARAMS
from test_residue_pairs import _mask, _oracle_pass, planes_packs

AA = ('i', 'j', 'dist', 'sift', 'ctype')
PLANES = ('plane_plane', 'atom_plane', 'group_group', 'group_plane')
BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
FEATURES = 0x7FE0
WATERS = (1 << CT['SELECTION_WATER']) | (1 << CT['WATER_WATER'])


def _masked(bag, sift_any, ctype_mask):
    """The yardstick: the records of a canonical bag with (sift & sift_any) != 0 && ((1 << ctype) & ctype_mask) != 0."""
    s = np.asarray(bag['sift']).astype(np.int64)
    c = np.asarray(bag['ctype']).astype(np.int64)
    m = ((s & int(sift_any)) != 0) & (((1 << c) & int(ctype_mask)) != 0)
    return {k: np.asarray(bag[k])[m] for k in AA}


def _bytes(bag, keys=None):
    return {k: np.asarray(bag[k]).tobytes() for k in (keys or bag)}


def _hdr():
    return open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()


# ---- the seam structures: every atom a residue of its own (no sequence-adjacency filter), clusters 20 A apart whose atoms are
# all within 5 A of each other: 64 + 8 + 3 + 2 atoms give C(64,2) + C(8,2) + C(3,2) + 1 = 2048 records, one more pair 2049
def _cluster(m, origin, spacing=0.9):
    g = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)], np.float64)[:m] * spacing
    return g + np.asarray(origin, np.float64)


def seam_one_tile():
    return tiny_complex(np.concatenate([_cluster(64, (0, 0, 0)), _cluster(8, (20, 0, 0)), _cluster(3, (40, 0, 0)), _cluster(2, (60, 0, 0))]))


def seam_one_tile_and_a_record():
    return tiny_complex(np.concatenate([_cluster(64, (0, 0, 0)), _cluster(8, (20, 0, 0)), _cluster(3, (40, 0, 0)), _cluster(2, (60, 0, 0)),
                                        _cluster(2, (80, 20, 20))]))


@functools.lru_cache(maxsize=None)
def _protein():
    return synth.proteinlike()


@functools.lru_cache(maxsize=None)
def _config3():
    return synth.config3(20000)


@functools.lru_cache(maxsize=None)
def _hub():
    return synth.proteinlike(n_res=40, seed=21, n_waters=20)


def _selection(pc, sel):
    """None: the whole structure; 'range': twelve consecutive residues; else a selector of the reference's syntax."""
    if sel is None:
        return np.ones(pc.n_atoms, np.uint8)
    if sel == 'range':
        r = pc.n_residues // 3
        return ((pc.res_id >= r) & (pc.res_id < r + 12)).astype(np.uint8)
    return _mask(pc, [sel])


@functools.lru_cache(maxsize=None)
def _oracle_sorted(make, sel=None):
    """The oracle's atom-atom bag of a whole pass at PARAMS[0], sorted by (i, j)."""
    pc = make()
    pc.ensure_labels()
    aa = _oracle_pass(pc, PARAMS[0], None if sel is None else _selection(pc, sel))['atom_atom']
    order = np.lexsort((aa['j'], aa['i']))
    return {k: np.asarray(aa[k])[order] for k in AA}


# ------------------------------------------------------------------------------------------------------------- CPU
def test_masks_give_the_headers_bit_for_every_single_name():
    hdr = _hdr()
    for k, name in enumerate(config.SIFT_NAMES):
        bit = int(re.search(r'#define\s+ARP_S_%s\s+\(1u << (\d+)\)' % name.upper(), hdr).group(1))
        assert contact_filter.masks([name]) == (1 << bit, 0x7F) and bit == k, name
        assert contact_filter.masks(name) == (1 << bit, 0x7F), name
    for name in config.CONTACT_TYPE_NAMES:
        val = int(re.search(r'#define\s+ARP_CT_%s\s+(\d+)' % name, hdr).group(1))
        assert contact_filter.masks(None, [name]) == (0x7FFF, 1 << val), name
    assert contact_filter.masks() == (0x7FFF, 0x7F) == (contact_filter.SIFT_ALL, contact_filter.CTYPE_ALL)
    assert int(re.search(r'#define\s+ARP_FILTER_SIFT_ALL\s+0x([0-9A-Fa-f]+)u', hdr).group(1), 16) == contact_filter.SIFT_ALL
    assert int(re.search(r'#define\s+ARP_FILTER_CTYPE_ALL\s+0x([0-9A-Fa-f]+)u', hdr).group(1), 16) == contact_filter.CTYPE_ALL
    assert contact_filter.masks(['hbond', 'ionic'], ['INTER', 'WATER_WATER']) == ((1 << 5) | (1 << 8), (1 << 2) | (1 << 5))
    assert 'arp_contacts_filter_launch' in _capi.SYMBOLS and 'arp_fetch_packed_filtered' in _capi.SYMBOLS


def test_presets():
    assert contact_filter.SPECIFIC == (0x7FFF & ~BIT['proximal'], 0x7F) == (0x7FEF, 0x7F)
    # interactions.py:166 of the reference: ('INTER', 'INTRA_SELECTION', 'SELECTION_WATER', 'WATER_WATER')
    assert contact_filter.BINDING_SITE == (0x7FFF, (1 << 2) | (1 << 1) | (1 << 3) | (1 << 5))
    from arpeggio_amd.core import export
    assert contact_filter.BINDING_SITE[1] == sum(1 << CT[t] for t in export._BS_CONTACT_TYPES)


def test_unknown_and_empty_names():
    with pytest.raises(ValueError, match='hbonds'):
        contact_filter.masks(['hbond', 'hbonds'])
    with pytest.raises(ValueError, match='INTRA'):
        contact_filter.masks(None, ['INTRA'])
    with pytest.raises(ValueError, match='empty'):
        contact_filter.masks([])
    with pytest.raises(ValueError, match='empty'):
        contact_filter.masks(['hbond'], [])
    from arpeggio_amd.core import InteractionComplex
    ic = InteractionComplex(_hub())
    with pytest.raises(ValueError, match='nothing_like_it'):
        ic.set_contact_filter(contacts=['nothing_like_it'])
    ic.set_contact_filter(contacts=['hbond'])
    assert ic._contact_filter == (BIT['hbond'], 0x7F)
    ic.set_contact_filter()
    assert ic._contact_filter is None


def test_apply_on_a_hand_made_bag():
    H, P, V, I = BIT['hbond'], BIT['proximal'], BIT['vdw'], BIT['ionic']
    bag = dict(i=np.array([0, 0, 1, 2, 3, 5], np.int32), j=np.array([1, 4, 2, 3, 4, 6], np.int32),
               dist=np.array([3.0, 4.5, 2.5, 3.25, 4.0, 4.75], np.float32), sift=np.array([H | P, P, V, I | V, P | H, P], np.uint16),
               ctype=np.array([2, 1, 2, 0, 5, 6], np.uint8))
    got = contact_filter.apply(bag, *contact_filter.SPECIFIC)
    assert got['i'].tolist() == [0, 1, 2, 3] and got['j'].tolist() == [1, 2, 3, 4] and got['dist'].tolist() == [3.0, 2.5, 3.25, 4.0]
    assert [got[k].dtype for k in AA] == [bag[k].dtype for k in AA] and list(got) == list(AA)
    assert contact_filter.apply(bag, H | I, 0x7F)['ctype'].tolist() == [2, 0, 5]
    assert contact_filter.apply(bag, H | I, 1 << 2)['j'].tolist() == [1]
    assert contact_filter.apply(bag, 0x7FFF, contact_filter.BINDING_SITE[1])['i'].tolist() == [0, 0, 1, 3]
    assert contact_filter.apply(bag, BIT['xbond'], 0x7F)['i'].tolist() == []
    _same(contact_filter.apply(bag, 0x7FFF, 0x7F), bag, 'everything')
    for sa, cm in ((H, 0x7F), (0x7FFF, 1 << 6), (P | V, (1 << 1) | (1 << 2))):
        _same(contact_filter.apply(bag, sa, cm), _masked(bag, sa, cm), (sa, cm))
    # a rows bag gives its i
    rows = _capi.RowsBag(row=np.array([0, 2, 3, 4, 5, 5, 6, 6], np.int32), **{k: bag[k] for k in AA[1:]})
    _same(contact_filter.apply(rows, H | I, 0x7F), _masked(bag, H | I, 0x7F), 'rows')


def test_the_seam_structures_are_what_they_claim():
    """By the oracle, on the CPU: exactly one tile of the filter (2048 records), and one record more."""
    for make, k in ((seam_one_tile, 2048), (seam_one_tile_and_a_record, 2049)):
        pc = make()
        aa = _oracle_pass(pc)['atom_atom']
        assert len(aa['i']) == k and not (np.asarray(aa['sift']) & BIT['hbond']).any()
        # a selection of two atoms in contact: their record alone is INTRA_SELECTION
        sel = np.zeros(pc.n_atoms, np.uint8)
        sel[[pc.n_atoms - 2, pc.n_atoms - 1]] = 1
        oc = oracle.OracleComplex(pc, sel, np.ones(pc.n_atoms, np.uint8))
        assert int((np.asarray(oc.atom_contacts(*PARAMS[0])['ctype']) == CT['INTRA_SELECTION']).sum()) == 1


def test_the_parity_structures_run_both_sides_of_the_small_sort_threshold():
    """By the oracle: config3(20 000) keeps 36 387 records under the feature bits (above the 32 768 of k_sort_small) and
    4 132 under hbond alone (below); proteinlike has 17 938 records, a partial last tile."""
    aa = _oracle_sorted(_config3)
    assert len(aa['i']) == 240949 and (len(aa['i']) + 2047) // 2048 == 118
    assert len(_masked(aa, FEATURES, 0x7F)['i']) == 36387 and len(_masked(aa, BIT['hbond'], 0x7F)['i']) == 4132
    assert len(_oracle_sorted(_protein)['i']) == 17938 and 17938 % 2048 != 0


# ------------------------------------------------------------------------------------------------------------- GPU
def _ctx(pc, sort_after=False):
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(sort_after)
    ctx.set_complex(pc)
    return ctx


def _full(ctx):
    """fetch_packed() in the records layout, copied out of its buffer: the yardstick bags."""
    ctx.set_packed_layout(False)
    bags, _ = ctx.fetch_packed()
    return {name: {k: np.array(v) for k, v in b.items()} for name, b in bags.items()}


def _check(ctx, full, sift_any, ctype_mask, what, n=None):
    """Both layouts of the filtered fetch against the masked yardstick; returns k'."""
    want = _masked(full['atom_atom'], sift_any, ctype_mask)
    n = ctx.n if n is None else n
    for rows in (False, True):
        ctx.set_packed_layout(rows)
        assert ctx.contacts_filter(sift_any, ctype_mask) == len(want['i']), (what, rows)
        got, _ = ctx.fetch_packed_filtered(sift_any, ctype_mask)
        aa = got['atom_atom']
        assert got['atom_atom_total'] == len(full['atom_atom']['i']), (what, rows)
        if rows:
            assert isinstance(aa, _capi.RowsBag) and 'i' not in aa
            row = np.asarray(aa['row'])
            assert row.dtype == np.int32 and row.tobytes() == np.searchsorted(want['i'], np.arange(n + 1)).astype(np.int32).tobytes(), (what, 'row')
            assert _bytes(aa, AA[1:]) == _bytes(want, AA[1:]), (what, rows)
            assert np.asarray(aa['i']).tobytes() == want['i'].tobytes(), (what, 'i from row')
        else:
            assert not isinstance(aa, _capi.RowsBag) and _bytes(aa, AA) == _bytes(want, AA), (what, rows)
        for name in PLANES:
            assert _bytes(got[name]) == _bytes(full[name]), (what, rows, name)
    ctx.set_packed_layout(False)
    return len(want['i'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['proteinlike', 'config3_20000', 'proteinlike_508', 'proteinlike_range'])
def test_parity_with_the_masked_canonical_bag(name):
    """The atom-atom bag never holds INTRA_BINDING_SITE (the reference gives that type to ring / amide records only, and the
    pairs inside one residue are not records), so '/A/508/' brings INTER and the water types; the residue range adds
    INTRA_SELECTION."""
    make = _config3 if name == 'config3_20000' else _protein
    sel = {'proteinlike_508': '/A/508/', 'proteinlike_range': 'range'}.get(name)
    pc = make()
    pc.ensure_labels()
    ctx = _ctx(pc)
    ctx.set_selection(_selection(pc, sel))
    ctx.run_launch(*PARAMS[0])
    full = _full(ctx)
    aa = full['atom_atom']
    # the yardstick itself, against the oracle's bag sorted by (i, j)
    orc = _oracle_sorted(make, sel)
    assert _bytes(aa, AA) == _bytes(orc, AA), name
    occurring = [b for b in range(15) if (aa['sift'] & (1 << b)).any()]
    if sel is None:
        assert len(aa['i']) == (240949 if make is _config3 else 17938)
        filters = [contact_filter.SPECIFIC, (FEATURES, 0x7F), (0x7FFF, WATERS)] + [(1 << b, 0x7F) for b in occurring]
        assert (aa['ctype'] == CT['SELECTION_WATER']).any() and (aa['ctype'] == CT['WATER_WATER']).any()
    else:
        for t in ('INTER', 'INTRA_NON_SELECTION') + (('INTRA_SELECTION',) if sel == 'range' else ()):
            assert (aa['ctype'] == CT[t]).any(), t
        assert not (aa['ctype'] == CT['INTRA_BINDING_SITE']).any()
        filters = [contact_filter.BINDING_SITE, (FEATURES, contact_filter.BINDING_SITE[1]), (0x7FFF, 1 << CT['INTER'])]
    kept = {}
    for sa, cm in filters:
        kept[(sa, cm)] = _check(ctx, full, sa, cm, (name, hex(sa), hex(cm)))
        # once more against the oracle's bag, masked
        ctx.set_packed_layout(False)
        got, _ = ctx.fetch_packed_filtered(sa, cm)
        assert _bytes(got['atom_atom'], AA) == _bytes(_masked(orc, sa, cm), AA), (name, hex(sa), hex(cm), 'oracle')
    print(name, 'records', len(aa['i']), 'kept', {(hex(a), hex(b)): v for (a, b), v in kept.items()})
    if make is _config3:      # both sides of the small-sort threshold (32 768 records) ran
        assert kept[(FEATURES, 0x7F)] == 36387 > 32768 and kept[(BIT['hbond'], 0x7F)] == 4132 < 32768
    assert all(v > 0 for v in kept.values())
    ctx.close()


@pytest.mark.gpu
def test_seams_all_none_and_the_tile_boundary():
    for make, k in ((seam_one_tile, 2048), (seam_one_tile_and_a_record, 2049)):
        pc = make()
        ctx = _ctx(pc)
        ctx.run_launch(*PARAMS[0])
        full = _full(ctx)
        assert len(full['atom_atom']['i']) == k
        # all kept: the result is fetch_packed()'s
        assert _check(ctx, full, 0x7FFF, 0x7F, (k, 'all')) == k
        got, _ = ctx.fetch_packed_filtered(0x7FFF, 0x7F)
        assert _bytes(got['atom_atom'], AA) == _bytes(full['atom_atom'], AA)
        # a ladder bit splits the tile
        assert 0 < _check(ctx, full, BIT['vdw_clash'], 0x7F, (k, 'vdw_clash')) < k
        # none kept: a bit that does not occur
        assert _check(ctx, full, BIT['hbond'], 0x7F, (k, 'none')) == 0
        ctx.close()


@pytest.mark.gpu
def test_none_kept_still_delivers_the_plane_bags():
    pc, _ = planes_packs()[9]
    ctx = _ctx(pc)
    ctx.run_launch(*PARAMS[0])
    full = _full(ctx)
    assert all(len(full[name][next(iter(full[name]))]) > 0 for name in PLANES)
    # (every SIFt bit occurs in this bag; a contact type the atom-atom bag never holds keeps nothing)
    absent = 1 << CT['INTRA_BINDING_SITE']
    assert not (full['atom_atom']['ctype'] == CT['INTRA_BINDING_SITE']).any() and len(full['atom_atom']['i']) > 0
    assert _check(ctx, full, 0x7FFF, absent, 'absent type') == 0
    ctx.set_packed_layout(True)
    got, _ = ctx.fetch_packed_filtered(0x7FFF, absent)
    assert len(got['atom_atom']['row']) == pc.n_atoms + 1 and not np.asarray(got['atom_atom']['row']).any()
    assert len(got['atom_atom']['j']) == 0
    assert _check(ctx, full, 0x7FFF, 0x7F, 'all') == len(full['atom_atom']['i'])
    ctx.close()


@pytest.mark.gpu
def test_exactly_one_kept_record_the_last_of_the_unsorted_bag():
    """2049 records: the last one is alone in the second tile.  The unsorted bag is read (no sort has run), the two atoms of
    its last record become the selection of an installed selection state (selection_plus stays every atom: the same grid, the
    same pair list), and after the pass over that state the record — the last of the bag again — is the one INTRA_SELECTION
    record.  The filter on that type keeps it alone."""
    pc = seam_one_tile_and_a_record()
    n = pc.n_atoms
    ctx = _ctx(pc, sort_after=False)
    one = np.ones(n, np.uint8)
    none = np.zeros(0, np.uint8)
    ctx.set_selection_state(one, one, none, none, none, none)
    k = ctx.atom_contacts_launch(*PARAMS[0])
    assert k == 2049
    raw = ctx.atom_contacts_fetch(k, sort=False)
    last = (int(raw['i'][-1]), int(raw['j'][-1]))
    sel = np.zeros(n, np.uint8)
    sel[list(last)] = 1
    ctx.set_selection_state(sel, one, none, none, none, none)
    assert ctx.atom_contacts_launch(*PARAMS[0]) == 2049
    raw = ctx.atom_contacts_fetch(k, sort=False)
    assert (int(raw['i'][-1]), int(raw['j'][-1])) == last      # (the order of the pair list did not change with the selection)
    assert int(raw['ctype'][-1]) == CT['INTRA_SELECTION'] and int((raw['ctype'] == CT['INTRA_SELECTION']).sum()) == 1
    want = {key: np.asarray(raw[key])[-1:] for key in AA}
    for rows in (False, True):
        ctx.set_packed_layout(rows)
        assert ctx.contacts_filter(0x7FFF, 1 << CT['INTRA_SELECTION']) == 1
        got, _ = ctx.fetch_packed_filtered(0x7FFF, 1 << CT['INTRA_SELECTION'])
        assert _bytes(got['atom_atom'], AA) == _bytes(want, AA), rows
        if rows:
            assert np.array_equal(got['atom_atom']['row'], np.searchsorted(want['i'], np.arange(n + 1)))
    # ... and everything but that record
    ctx.set_packed_layout(False)
    full = _full(ctx)
    assert _check(ctx, full, 0x7FFF, 0x7F & ~(1 << CT['INTRA_SELECTION']), 'all but the last') == 2048
    ctx.close()


@pytest.mark.gpu
def test_twenty_random_mask_pairs_keep_what_numpy_counts():
    pc = _config3()
    ctx = _ctx(pc)
    ctx.run_launch(*PARAMS[0])
    full = _full(ctx)
    rs = np.random.RandomState(20)
    counts = []
    for _ in range(20):
        sa, cm = int(rs.randint(1, 1 << 15)), int(rs.randint(1, 1 << 7))
        want = _masked(full['atom_atom'], sa, cm)
        got, _ = ctx.fetch_packed_filtered(sa, cm)
        assert len(got['atom_atom']['i']) == len(want['i']) == ctx.contacts_filter(sa, cm), (hex(sa), hex(cm))
        assert _bytes(got['atom_atom'], AA) == _bytes(want, AA), (hex(sa), hex(cm))
        counts.append(len(want['i']))
    assert len(set(counts)) > 10 and min(counts) < 32768 < max(counts)
    ctx.close()


@pytest.mark.gpu
def test_a_batch_splits_into_the_single_runs_masked_bags():
    pcs = [synth.proteinlike(), synth.proteinlike(seed=5, id='variant5'), synth.proteinlike(seed=9, id='variant9')]
    filters = (contact_filter.SPECIFIC, (BIT['hbond'] | BIT['ionic'], 0x7F))
    singles = []
    for pc in pcs:
        ctx = _ctx(pc)
        ctx.run_launch(*PARAMS[0])
        singles.append(_full(ctx))
        ctx.close()
    ctx = _capi.Context(0)
    off = ctx.set_batch(pcs)
    assert ctx.n > 12288      # (beyond k_sort_small's ids: the radix passes run whatever the count)
    ctx.run_launch(*PARAMS[0])
    for sa, cm in filters:
        got, _ = ctx.fetch_packed_filtered(sa, cm)
        parts = batch.split_atom_contacts({k: np.asarray(got['atom_atom'][k]) for k in AA}, off)
        for s in range(3):
            want = _masked(singles[s]['atom_atom'], sa, cm)
            assert len(want['i']) > 0 and _bytes(parts[s], AA) == _bytes(want, AA), (hex(sa), s)
        for name in PLANES:
            for s, part in enumerate(batch.split_bag(name, {k: np.asarray(v) for k, v in got[name].items()}, off)):
                assert _bytes(part) == _bytes(singles[s][name]), (name, s)
    full = _full(ctx)
    _check(ctx, full, *filters[1], 'batch, both layouts')
    ctx.close()


@pytest.mark.gpu
def test_models_split_and_the_tables_do_not_notice():
    pc = copy.copy(_hub())
    pc.ensure_labels()
    F = 8
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    ctx = _capi.Context(0)
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    ctx.run_launch(*PARAMS[0])
    tables = lambda: (ctx.residue_pairs(), ctx.models_persistence(), ctx.models_residue_persistence())
    before = tables()
    whole = _capi.split_models(_full(ctx), ctx._models)
    sa, cm = contact_filter.SPECIFIC
    for rows in (False, True):
        ctx.set_packed_layout(rows)
        got, _ = ctx.fetch_packed_filtered(sa, cm)
        per = _capi.split_models(got, ctx._models)
        assert len(per) == F
        for f in range(F):
            want = _masked(whole[f]['atom_atom'], sa, cm)
            assert len(want['i']) > 0 and _bytes(per[f]['atom_atom'], AA) == _bytes(want, AA), (rows, f)
            for name in PLANES:
                assert _bytes(per[f][name]) == _bytes(whole[f][name]), (rows, f, name)
    ctx.set_packed_layout(False)
    for a, b in zip(before, tables()):
        assert _bytes(a) == _bytes(b)
    # the tables made first after a new pass, the filtered fetch second
    ctx.run_launch(*PARAMS[0])
    ctx.fetch_packed_filtered(sa, cm)
    for a, b in zip(before, tables()):
        assert _bytes(a) == _bytes(b)
    ctx.close()


@pytest.mark.gpu
def test_contract():
    pc = _hub()
    L = _capi.load()
    ctx = _capi.Context(0)
    h = ctx._h
    kept = C.c_int64(-1)
    counts, offs, used = (C.c_int64 * 5)(), (C.c_uint64 * 53)(), C.c_uint64(0)
    buf = _capi.pinned_empty(1 << 20, np.uint8)
    launch = lambda sa=0x7FEF, cm=0x7F: L.arp_contacts_filter_launch(h, sa, cm, C.byref(kept))
    fetch = lambda nbytes=None: L.arp_fetch_packed_filtered(h, _capi._p(buf), buf.nbytes if nbytes is None else nbytes, counts, offs, C.byref(used))
    # no results
    assert launch() == _capi.ARP_E_ARG and fetch() == _capi.ARP_E_ARG
    ctx.set_complex(pc)
    assert launch() == _capi.ARP_E_ARG and fetch() == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    # a fetch without a launch; masks with bits out of range; a zero mask
    assert fetch() == _capi.ARP_E_ARG
    assert launch(0x8000) == _capi.ARP_E_ARG and launch(0x7FFF, 0x80) == _capi.ARP_E_ARG and launch(0x17FFF) == _capi.ARP_E_ARG
    assert launch(0, 0x7F) == _capi.ARP_E_ARG and launch(0x7FFF, 0) == _capi.ARP_E_ARG
    assert b'keeps nothing' in L.arp_last_error(h)
    assert fetch() == _capi.ARP_E_ARG
    with pytest.raises(ValueError):
        ctx.contacts_filter(0x7FFF, 0x100)
    # a launch; the second one with the same masks returns the stored count (the library's profiling slots cover the kernels
    # of a pass, not these: only the count is asserted)
    full = _full(ctx)
    want = _masked(full['atom_atom'], 0x7FEF, 0x7F)
    assert launch() == _capi.ARP_OK and kept.value == len(want['i']) > 0
    kept.value = -1
    assert launch() == _capi.ARP_OK and kept.value == len(want['i'])
    # other masks re-make it
    assert launch(BIT['hbond']) == _capi.ARP_OK and kept.value == len(_masked(full['atom_atom'], BIT['hbond'], 0x7F)['i'])
    assert launch() == _capi.ARP_OK and kept.value == len(want['i'])
    # a host buffer that is too small: ARP_E_CAPACITY with bytes_used, then the fetch
    assert fetch(64) == _capi.ARP_E_CAPACITY and used.value > 64
    need = int(used.value)
    assert fetch(need - 1) == _capi.ARP_E_CAPACITY and used.value == need
    assert fetch(need) == _capi.ARP_OK and used.value == need and counts[0] == len(want['i'])
    assert np.frombuffer(buf, np.int32, counts[0], int(offs[0])).tobytes() == want['i'].tobytes()
    small = _capi.pinned_empty(64, np.uint8)      # (the binding grows the buffer)
    got, grown = ctx.fetch_packed_filtered(0x7FEF, 0x7F, buf=small)
    assert grown.nbytes >= need and _bytes(got['atom_atom'], AA) == _bytes(want, AA)
    # voided by a new pass
    ctx.run_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and fetch() == _capi.ARP_OK
    # ... by set_selection (and made again after the pass that follows)
    ctx.set_selection(np.ones(pc.n_atoms, np.uint8))
    assert fetch() == _capi.ARP_E_ARG and launch() == _capi.ARP_E_ARG
    ctx.run_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and kept.value == len(want['i']) and fetch() == _capi.ARP_OK
    # ... by a change of the layout (setting the same layout again changes nothing)
    ctx.set_packed_layout(False)
    assert fetch() == _capi.ARP_OK
    ctx.set_packed_layout(True)
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and fetch() == _capi.ARP_OK
    ctx.set_packed_layout(False)
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and fetch() == _capi.ARP_OK
    # ... by the re-run of one ring bag
    ctx.launch_bag('plane_plane')
    assert fetch() == _capi.ARP_E_ARG
    assert launch() == _capi.ARP_OK and fetch() == _capi.ARP_OK
    # ... by the atom-atom launch alone
    ctx.atom_contacts_launch(*PARAMS[0])
    assert fetch() == _capi.ARP_E_ARG
    # a shard
    ctx.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    assert launch() == _capi.ARP_E_ARG and b'shard' in L.arp_last_error(h)
    ctx.close()


@pytest.mark.gpu
def test_the_unfiltered_fetch_does_not_notice():
    pc = _hub()
    for rows in (False, True):
        for sort_after in (False, True):
            plain = _ctx(pc, sort_after)
            plain.set_packed_layout(rows)
            plain.run_launch(*PARAMS[0])
            ref = {name: _bytes(b) for name, b in plain.fetch_packed()[0].items()}
            plain.close()
            ctx = _ctx(pc, sort_after)
            ctx.set_packed_layout(rows)
            ctx.run_launch(*PARAMS[0])
            packed = lambda: {name: _bytes(b) for name, b in ctx.fetch_packed()[0].items()}
            before = packed()
            k = ctx.contacts_filter(*contact_filter.SPECIFIC)
            got, _ = ctx.fetch_packed_filtered(*contact_filter.SPECIFIC)
            assert 0 < k == len(got['atom_atom']['j'])
            assert before == packed() == ref, (rows, sort_after)
            # the filtered fetch first after a pass, the unfiltered one after it; the separate columns likewise
            ctx.run_launch(*PARAMS[0])
            got2, _ = ctx.fetch_packed_filtered(*contact_filter.SPECIFIC)
            assert _bytes(got2['atom_atom'], AA[1:]) == _bytes(got['atom_atom'], AA[1:]), (rows, sort_after)
            assert packed() == ref, (rows, sort_after, 'filtered first')
            ctx.close()


def _python_filtered(records, names):
    return [r for r in records if r['type'] != 'atom-atom' or set(r['contact']) & set(names)]


@pytest.mark.gpu
def test_interaction_complex_with_a_contact_filter(tmp_path):
    from arpeggio_amd.core import InteractionComplex
    names = ['hbond', 'ionic']
    plain = InteractionComplex(copy.copy(_protein()))
    plain.run_arpeggio([], *PARAMS[0])
    everything = plain.get_contacts()
    want = _python_filtered(everything, names)
    n_aa = sum(r['type'] == 'atom-atom' for r in want)
    assert 0 < n_aa < sum(r['type'] == 'atom-atom' for r in everything) and len(want) > n_aa      # (the other four bags are there)
    ic = InteractionComplex(copy.copy(_protein()))
    ic.set_contact_filter(contacts=names)
    ic.run_arpeggio([], *PARAMS[0])
    assert ic.get_contacts() == want
    assert len(ic.atom_contacts) == n_aa == ic._bags['atom_atom_total'] - (len(everything) - len(want))
    path = tmp_path / 'filtered.json'
    ic.write_json(str(path))
    assert path.read_text() == json.dumps(want, indent=4, sort_keys=True)
    # what is made from the resident bag is the unfiltered run's
    a, b = ic.atom_sifts(), plain.atom_sifts()
    assert _bytes(a) == _bytes(b)
    assert ic.atom_integer_sifts().tobytes() == plain.atom_integer_sifts().tobytes()
    _same(ic.residue_contacts(), plain.residue_contacts(), 'residue_contacts')
    assert np.array_equal(ic.selection_plus, plain.selection_plus)
    ic.write_contacts([], str(tmp_path))
    with open(tmp_path / (ic.id + '_contacts.csv')) as fh:
        assert len(fh.read().splitlines()) == n_aa + 1
    # clearing the filter restores the full bag
    ic.set_contact_filter()
    ic.run_arpeggio([], *PARAMS[0])
    assert ic.get_contacts() == everything and 'atom_atom_total' not in ic._bags


@pytest.mark.gpu
def test_ensemble_complex_with_a_contact_filter():
    from arpeggio_amd.core import EnsembleComplex
    names = ['hbond', 'ionic']
    pc = copy.copy(_hub())
    pc.ensure_labels()
    F = 4
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    plain = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    plain.run_arpeggio([], *PARAMS[0])
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.set_contact_filter(contacts=names)
    ens.run_arpeggio([], *PARAMS[0])
    kept = 0
    for f in range(F):
        want = _python_filtered(plain.model(f).get_contacts(), names)
        assert ens.model(f).get_contacts() == want, f
        kept += sum(r['type'] == 'atom-atom' for r in want)
    assert kept > 0
    ens.set_contact_filter()
    ens.run_arpeggio([], *PARAMS[0])
    assert ens.model(1).get_contacts() == plain.model(1).get_contacts()
