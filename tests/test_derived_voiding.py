"""Which event voids which derived result: the matrix "event x result" of the seven results made on the device from the bags of
a pass (arp_api.hip, ``void_results``) — contact persistence, the residue-pair table, residue persistence, the filtered
atom-atom bag, water bridges, water-bridge persistence and the similarity matrix, the last once at atom level and once at
residue level.

Per case: a pass, all seven made, every fetch entry point called through ctypes (the bytes "before"), the event, every fetch
again: ``ARP_OK`` with the same bytes, or ``ARP_E_ARG``.  The expectations are what each result reads:

    persist, bridges                the atom-atom bag
    bridgepersist                   the bridge table
    respair, respersist, filtered   all five bags (filtered also the packed layout)
    similarity                      the bags of its level

No tolerance anywhere: bytes or a return code."""
import ctypes as C
import functools

import numpy as np
import pytest

from arpeggio_amd import _capi, contact_filter, similarity, synth, tables
from arpeggio_amd.core import config
from test_persistence import _ctx_with_models

F = 3
BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
SPECIFIC = contact_filter.SPECIFIC[0]
HP = BIT['hbond'] | BIT['polar']
PLANES = similarity.planes(None, ('atom_atom',))
RESULTS = ('persist', 'respair', 'respersist', 'filtered', 'bridges', 'bridgepersist', 'similarity')
OK, E_ARG = _capi.ARP_OK, _capi.ARP_E_ARG


@functools.lru_cache(maxsize=None)
def _input():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    pc.ensure_labels()
    return (pc,) + tuple(synth.models_of(pc, F, seed=4))


def _table_fetch(ctx, name, spec, U):
    t = tables.alloc(spec, U, np.zeros)
    n = C.c_int64(-1)
    rc = getattr(ctx._L, name)(ctx._h, U, *(_capi._p(t[k]) for k, _ in spec.columns), C.byref(n))
    return rc, b''.join(t[k].tobytes() for k, _ in spec.columns)


def _filtered_fetch(ctx):
    buf = _capi.pinned_empty(1 << 20, np.uint8)
    counts, offs, used = (C.c_int64 * 5)(), (C.c_uint64 * 53)(), C.c_uint64(0)
    rc = ctx._L.arp_fetch_packed_filtered(ctx._h, _capi._p(buf), buf.nbytes, counts, offs, C.byref(used))
    if rc != OK:
        return rc, b''
    bags = ctx._packed_views(buf, counts, offs)
    cols = lambda b: b._asdict() if hasattr(b, '_asdict') else b
    return rc, bytes(counts) + b''.join(np.asarray(v).tobytes() for name in sorted(bags) for _, v in sorted(cols(bags[name]).items()))


def _similarity_fetch(ctx):
    inter = np.zeros((F, F), np.uint32)
    n = C.c_int64(-1)
    return ctx._L.arp_models_similarity_fetch(ctx._h, F, _capi._p(inter), C.byref(n)), inter.tobytes()


def _make_all(by_residue):
    """A context with a pass and all seven results made; {result: fetch()} with fetch() -> (return code, bytes)."""
    pc, xyz, h_xyz = _input()
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    counts = ctx.run_launch(5.0)
    assert all(counts[k] > 0 for k in ('atom_atom', 'atom_plane', 'group_group')), counts      # (records of rings and of amides)
    bspec = tables.BRIDGES
    rows = dict(persist=len(ctx.models_persistence()['a']), respair=len(ctx.residue_pairs()['res_a']),
                respersist=len(ctx.models_residue_persistence()['res_a']), filtered=ctx.contacts_filter(SPECIFIC, 0x7F),
                bridges=len(ctx.water_bridges(SPECIFIC)['water']), bridgepersist=len(ctx.models_water_bridge_persistence(SPECIFIC)['a']))
    inter = ctx.models_similarity(PLANES, by_residue=by_residue)
    assert all(v > 0 for v in rows.values()) and np.diagonal(inter).min() > 0, rows
    fetch = dict(
        persist=lambda: _table_fetch(ctx, 'arp_models_persistence_fetch', tables.PERSIST, rows['persist']),
        respair=lambda: _table_fetch(ctx, 'arp_residue_pairs_fetch', tables.RESPAIR, rows['respair']),
        respersist=lambda: _table_fetch(ctx, 'arp_models_residue_persistence_fetch', tables.RESPERSIST, rows['respersist']),
        filtered=lambda: _filtered_fetch(ctx),
        bridges=lambda: _table_fetch(ctx, 'arp_water_bridges_fetch', bspec, rows['bridges']),
        bridgepersist=lambda: _table_fetch(ctx, 'arp_models_water_bridge_persistence_fetch', tables.BRIDGEPERSIST_ATOM, rows['bridgepersist']),
        similarity=lambda: _similarity_fetch(ctx))
    return ctx, fetch, rows, bspec


# event -> (what it does to the context, the results it voids; 'similarity@residue': the matrix only when made by residue)
def _toggle_layout(ctx):
    ctx.set_packed_layout(True)


EVENTS = {
    'none': (lambda ctx: None, ()),
    'run_launch': (lambda ctx: ctx.run_launch(5.0), RESULTS),
    'plane_bag_alone': (lambda ctx: ctx.launch_bag('plane_plane'), ('respair', 'respersist', 'filtered', 'similarity@residue')),
    'amide_bag_alone': (lambda ctx: ctx.launch_bag('group_group'), ('respair', 'respersist', 'filtered', 'similarity@residue')),
    'set_selection': (lambda ctx: ctx.set_selection(np.ones(ctx.n, np.uint8)), RESULTS),
    'packed_layout': (_toggle_layout, ('filtered',)),
    'bridges_same_arguments': (lambda ctx: ctx.water_bridges(SPECIFIC), ()),
}


@pytest.mark.gpu
@pytest.mark.parametrize('by_residue', (False, True), ids=('sim_atom', 'sim_residue'))
@pytest.mark.parametrize('event', list(EVENTS))
def test_an_event_voids_exactly_the_results_that_read_what_it_replaced(event, by_residue):
    ctx, fetch, _, _ = _make_all(by_residue)
    before = {r: fetch[r]() for r in RESULTS}
    assert all(rc == OK and len(b) > 0 for rc, b in before.values()), {r: rc for r, (rc, _) in before.items()}
    apply, voided = EVENTS[event]
    apply(ctx)
    gone = {r for r in RESULTS if r in voided or (by_residue and r + '@residue' in voided)}
    for r in RESULTS:
        rc, b = fetch[r]()
        if r in gone:
            assert rc == E_ARG, (event, r, rc)
        else:
            assert rc == OK and b == before[r][1], (event, r, rc)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('by_residue', (False, True), ids=('sim_atom', 'sim_residue'))
def test_another_bridge_table_replaces_it_and_voids_bridge_persistence_alone(by_residue):
    ctx, fetch, rows, bspec = _make_all(by_residue)
    before = {r: fetch[r]() for r in RESULTS}
    other = ctx.water_bridges(HP)
    assert len(other['water']) > 0
    rc, b = _table_fetch(ctx, 'arp_water_bridges_fetch', bspec, len(other['water']))
    assert rc == OK and b == b''.join(other[k].tobytes() for k, _ in bspec.columns) and b != before['bridges'][1]
    for r in RESULTS:
        if r == 'bridges':
            continue
        rc, b = fetch[r]()
        if r == 'bridgepersist':
            assert rc == E_ARG, rc
        else:
            assert rc == OK and b == before[r][1], (r, rc)
    ctx.close()
