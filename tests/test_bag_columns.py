"""The four ring / amide bags have ONE description (``arpeggio_amd.tables.BAGS``; PLANE_TABLES in csrc/arp_bag_table.h): what derives
from it agrees with it, ``batch.split_bag`` cuts as its if-chain did, and the library packs, stages and fetches exactly the
columns it names.  The GPU part needs a real MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from arpeggio_amd import _capi, batch, poses, synth, tables

NAMES = ('atom_plane', 'plane_plane', 'group_group', 'group_plane')
PACKED = ('plane_plane', 'atom_plane', 'group_group', 'group_plane')      # counts[1..4] and b of arp_fetch_packed
PARAMS = (5.0, 0.1, False, 6.0)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_one_description_everywhere():
    assert tables.PLANE_BAGS == NAMES == poses.PLANE_TABLES == tuple(_capi.Context._BAGS)
    assert tuple(name for name, _ in _capi.Context._PACKED_BAGS) == PACKED == tables.PACKED_ORDER
    packed = dict(_capi.Context._PACKED_BAGS)
    for name in NAMES:
        mk, keys, order = _capi.Context._BAGS[name]
        ids, vals, byts, vdt = poses.PLANE_COLUMNS[name]
        dtypes = [np.dtype(np.int32)] * 2 + [np.dtype(vdt)] * len(vals) + [np.dtype(np.uint8)] * len(byts)
        assert keys == ids + vals + byts == tuple(k for k, _, _ in packed[name]) == tuple(c for c, _ in poses.plane_columns(name))
        assert [a.dtype for a in mk(3)] == dtypes == [np.dtype(dt) for _, _, dt in packed[name]] == [np.dtype(dt) for _, dt in poses.plane_columns(name)]
        assert all(len(a) == 3 for a in mk(3))
        assert order == poses.PLANE_ORDER[name] and set(order) == set(ids)
        # slots: ids 0 and 1, float64 values from 2, float32 values from 6, bytes from 9; none twice
        slots = [q for _, q, _ in packed[name]]
        v0 = {8: 2, 4: 6}[np.dtype(vdt).itemsize]
        assert slots == [0, 1] + list(range(v0, v0 + len(vals))) + list(range(9, 9 + len(byts)))
        assert len(set(slots)) == len(slots) and max(slots) < 12 and len(vals) <= (4 if v0 == 2 else 3) and len(byts) <= 3
    assert poses.PLANE_ORDER['atom_plane'] == ('ring', 'atom')


def test_buffers_match_the_pointer_arguments_of_the_c_entries():
    L = _capi.load()
    for name in NAMES:
        n_buffers = len(_capi.Context._BAGS[name][0](1))
        for fn in (getattr(L, f'arp_{name}_fetch'), getattr(L, f'arp_{name}')):
            at = fn.argtypes
            assert at is not None and at[0] is C.c_void_p and at[1] is C.c_int64 and at[-1] == C.POINTER(C.c_int64)
            assert len(at) - 3 == n_buffers and all(a is C.c_void_p for a in at[2:-1]), (name, at)


OFF = {'atom': np.array([0, 10, 25]), 'ring': np.array([0, 3, 7]), 'amide': np.array([0, 2, 6])}
F8, F4, U1, I4 = np.float64, np.float32, np.uint8, np.int32
HAND = {      # a bag of each kind over two structures, and what the if-chain of split_bag returned for it before the table
    'atom_plane': (
        dict(atom=([12, 3, 24, 0], I4), ring=([4, 2, 6, 0], I4), dist=([1.5, 2.5, 3.5, 4.5], F8), theta=([10., 20., 30., 40.], F8),
             mask=([1, 2, 3, 4], U1), ctype=([5, 6, 5, 6], U1)),
        [dict(atom=([3, 0], I4), ring=([2, 0], I4), dist=([2.5, 4.5], F8), theta=([20., 40.], F8), mask=([2, 4], U1), ctype=([6, 6], U1)),
         dict(atom=([2, 14], I4), ring=([1, 3], I4), dist=([1.5, 3.5], F8), theta=([10., 30.], F8), mask=([1, 3], U1), ctype=([5, 5], U1))]),
    'plane_plane': (
        dict(bgn=([3, 0, 5, 1], I4), end=([6, 2, 4, 0], I4), dist=([1., 2., 3., 4.], F8), dihedral=([5., 6., 7., 8.], F8),
             theta_bgn=([9., 10., 11., 12.], F8), theta_end=([13., 14., 15., 16.], F8), type1=([0, 1, 2, 3], U1), type2=([3, 2, 1, 0], U1),
             ctype=([5, 5, 6, 6], U1)),
        [dict(bgn=([0, 1], I4), end=([2, 0], I4), dist=([2., 4.], F8), dihedral=([6., 8.], F8), theta_bgn=([10., 12.], F8),
              theta_end=([14., 16.], F8), type1=([1, 3], U1), type2=([2, 0], U1), ctype=([5, 6], U1)),
         dict(bgn=([0, 2], I4), end=([3, 1], I4), dist=([1., 3.], F8), dihedral=([5., 7.], F8), theta_bgn=([9., 11.], F8),
              theta_end=([13., 15.], F8), type1=([0, 2], U1), type2=([3, 1], U1), ctype=([5, 6], U1))]),
    'group_group': (
        dict(bgn=([5, 0, 2, 1], I4), end=([3, 1, 4, 0], I4), dist=([1., 2., 3., 4.], F4), dihedral=([5., 6., 7., 8.], F4),
             theta=([9., 10., 11., 12.], F4), ctype=([5, 6, 5, 6], U1)),
        [dict(bgn=([0, 1], I4), end=([1, 0], I4), dist=([2., 4.], F4), dihedral=([6., 8.], F4), theta=([10., 12.], F4), ctype=([6, 6], U1)),
         dict(bgn=([3, 0], I4), end=([1, 2], I4), dist=([1., 3.], F4), dihedral=([5., 7.], F4), theta=([9., 11.], F4), ctype=([5, 5], U1))]),
    'group_plane': (
        dict(amide=([4, 1, 0, 3], I4), ring=([6, 0, 2, 3], I4), dist=([1., 2., 3., 4.], F8), dihedral=([5., 6., 7., 8.], F8),
             theta=([9., 10., 11., 12.], F8), ctype=([6, 5, 6, 5], U1)),
        [dict(amide=([1, 0], I4), ring=([0, 2], I4), dist=([2., 3.], F8), dihedral=([6., 7.], F8), theta=([10., 11.], F8), ctype=([5, 6], U1)),
         dict(amide=([2, 1], I4), ring=([3, 0], I4), dist=([1., 4.], F8), dihedral=([5., 8.], F8), theta=([9., 12.], F8), ctype=([6, 5], U1))]),
}


def test_split_bag_cuts_as_the_if_chain_did():
    assert set(HAND) == set(NAMES)
    for name, (bag, want) in HAND.items():
        got = batch.split_bag(name, {k: np.array(v, dt) for k, (v, dt) in bag.items()}, OFF)
        assert len(got) == len(want) == 2
        for g, w in zip(got, want):
            assert list(g) == list(w) == list(bag)
            for k, (v, dt) in w.items():
                assert g[k].dtype == np.dtype(dt) and g[k].tolist() == v, (name, k)
    with pytest.raises(KeyError):
        batch.split_bag('atom_atom', {}, OFF)


# ------------------------------------------------------------------------------------------------------------- GPU
def _structures():
    return (('proteinlike', synth.proteinlike()), ('config5_600_500', synth.config5(600, 500)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _al(v, a):
    return (v + a - 1) // a * a


@pytest.mark.gpu
def test_packed_offsets_name_exactly_the_columns_a_bag_has():
    """arp_fetch_packed reports an offset for exactly the columns ``tables.BAGS`` names, and ``bytes_used`` counts only those.
    (Before the bags were laid out from the table this failed in two clauses and no other: "0 for the other slots" — atom-plane
    reported offsets for slots 4, 5 and 11, group-group for 10 and 11, group-plane for 5, 10 and 11 — and the ``bytes_used``
    equality, 275 136 against 274 096 on ``proteinlike()``.)"""
    ctx = _capi.Context(0)
    slots = {name: {q: np.dtype(dt).itemsize for _, q, dt in cols} for name, cols in ctx._PACKED_BAGS}
    for sid, pc in _structures():
        ctx.set_complex(pc)
        ran = ctx.run_launch(*PARAMS)
        buf = _capi.pinned_empty(16 << 20, np.uint8)
        counts, offs, used = (C.c_int64 * 5)(), (C.c_uint64 * 53)(), C.c_uint64(0)
        assert ctx._L.arp_fetch_packed(ctx._h, _capi._p(buf), buf.nbytes, counts, offs, C.byref(used)) == 0
        assert counts[0] > 0 and [int(counts[1 + b]) for b in range(4)] == [ran[name] for name in PACKED]
        # the atom-atom columns: five offsets, the last column one byte a record, each column rounded up to 256 bytes
        aa_bytes = int(offs[4]) + _al(int(counts[0]), 256)
        want_bytes, last, report = aa_bytes, aa_bytes - 1, []
        for b, name in enumerate(PACKED):
            m = int(counts[1 + b])
            got = [int(offs[5 + 12 * b + q]) for q in range(12)]
            report.append((name, m, got))
            if m == 0:
                assert got == [0] * 12, (sid, name)
                continue
            for q in range(12):
                if q in slots[name]:
                    want_bytes += _al(m * slots[name][q], 16)
                    assert got[q] != 0 and got[q] % 16 == 0 and got[q] > last, (sid, name, q, got)
                    last = got[q]
        print(sid, 'bytes_used', int(used.value), 'named columns give', want_bytes, report)
        if sid == 'config5_600_500':
            assert all(int(counts[1 + b]) > 0 for b in range(4))
        for name, m, got in report:      # a slot the table does not name: the bag has no such array
            assert all(got[q] == 0 for q in range(12) if q not in slots[name]), (sid, name, got)
        assert int(used.value) == want_bytes, (sid, int(used.value), want_bytes)
    ctx.close()


@pytest.mark.gpu
def test_staged_and_unstaged_fetch_bag_agree_with_the_packed_fetch():
    ctx = _capi.Context(0)
    for sid, pc in _structures():
        ctx.set_complex(pc)
        ran = ctx.run_launch(*PARAMS)
        plain = {name: {k: v.copy() for k, v in ctx.fetch_bag(name, sort=False).items()} for name in NAMES}
        pinned = {name: ctx.fetch_bag(name, sort=False, out=ctx.pinned_bag_buffers(name, ran[name])) for name in NAMES}
        packed, _ = ctx.fetch_packed()
        for name in NAMES:
            mk, keys, order = ctx._BAGS[name]
            assert tuple(plain[name]) == tuple(pinned[name]) == keys
            o = np.lexsort((plain[name][order[1]], plain[name][order[0]]))
            for k in keys:
                assert len(plain[name][k]) == ran[name] and plain[name][k].dtype == packed[name][k].dtype, (sid, name, k)
                assert np.array_equal(_bits(plain[name][k]), _bits(pinned[name][k])), (sid, name, k)
                assert np.array_equal(_bits(plain[name][k][o]), _bits(packed[name][k])), (sid, name, k)
        if sid == 'config5_600_500':      # (the staged path: every bag has records, all of them well under BAG_STAGE_MAX = 4 MiB)
            assert all(ran[name] > 0 for name in NAMES)
            assert sum(ran[name] * sum(a.itemsize for a in ctx._BAGS[name][0](1)) for name in NAMES) < 1 << 20
    ctx.close()


@pytest.mark.gpu
def test_launch_and_fetch_wrapper_with_too_small_a_capacity():
    ctx = _capi.Context(0)
    ctx.set_complex(synth.config5(600, 500))
    ran = ctx.run_launch(*PARAMS)
    real = ran['plane_plane']
    assert real > 1
    fn = ctx._L.arp_plane_plane

    def call(cap, n):
        arrs = ctx._BAGS['plane_plane'][0](n)
        cnt = C.c_int64(-7)
        return fn(ctx._h, cap, *[_capi._p(a) for a in arrs], C.byref(cnt)), int(cnt.value), arrs
    rc, cnt, _ = call(1, 1)
    assert rc == _capi.ARP_E_CAPACITY and cnt == real
    rc, cnt, arrs = call(cnt, cnt)
    assert rc == _capi.ARP_OK and cnt == real
    want = ctx.fetch_bag('plane_plane', sort=False)
    for k, a in zip(ctx._BAGS['plane_plane'][1], arrs):
        assert np.array_equal(_bits(a), _bits(want[k])), k
    rc, _, _ = call(-1, 1)
    assert rc == _capi.ARP_E_ARG
    ctx.close()
