"""Which event voids which result of the ligand-pose family: the matrix "event x result" of the four results made on the device
from uploaded poses (arp_api.hip, ``void_pose_results``) — the poses result, the poses-planes result with its plane atoms, the
fingerprint and the shortlist, the last two once made from the poses result alone and once with the poses-planes result read
as well (class planes / a ring table).

Per case: all four made, every fetch entry point called through ctypes (the bytes "before"), the event, every fetch again:
``ARP_OK`` with the same bytes, or ``ARP_E_ARG``; and whether ``poses_planes_info()['plane_atoms']`` still says yes.  The
expectations are what each result reads:

    plane atoms                     the structure
    poses-planes                    the structure, the selection, the plane atoms (through the movable set-up)
    poses                           the structure, the selection
    fingerprint, shortlist          the poses result; the poses-planes result when made with class planes / a ring table

    event                           poses   planes  fingerprint  shortlist   plane atoms
    none                            .       .       .            .           .
    contacts launch, same poses     same    .       x            x           .
    planes launch, same poses       .       same    with planes  with planes .
    set_plane_atoms again           .       x       with planes  with planes again
    set_selection, same mask        x       x       x            x           .
    set_complex                     x       x       x            x           x
    run_launch (a pass)             .       .       .            .           .
    fingerprint, other arguments    .       .       same         .           .
    a refused launch of any         .       .       .            .           .

(x: the fetch refuses; same: made again, the same bytes; with planes: x only for the kind that read the poses-planes result.)
No tolerance anywhere: bytes or a return code."""
import ctypes as C
import functools

import numpy as np
import pytest

from arpeggio_amd import _capi, pose_fingerprints as fp, pose_shortlist as sl, poses, synth
from arpeggio_amd.core import utils

P = 5
PARAMS = (5.0, 0.1, False)
ALL15 = 0x7FFF
RESULTS = ('poses', 'planes', 'fingerprint', 'shortlist')
OK, E_ARG = _capi.ARP_OK, _capi.ARP_E_ARG
_p = _capi._p


@functools.lru_cache(maxsize=None)
def _input():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    x, h = synth.poses_of(pc, idx, P, seed=11, shift=3.0, jitter=0.2)
    mask = np.zeros(pc.n_atoms, np.uint8)
    mask[idx] = 1
    return pc, mask, x, h


def _planes_of(with_planes):
    return fp.planes(classes='all') if with_planes else ALL15


def _make_all(with_planes):
    """A context with all four results made; {result: fetch()} with fetch() -> (return code, bytes)."""
    pc, mask, x, h = _input()
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(mask)
    ctx.set_plane_atoms(pc)
    table = ctx.poses_contacts(x, h, *PARAMS)
    ptable = ctx.poses_planes(x)
    rows = {name: len(ptable[name]['ctype']) for name in poses.PLANE_TABLES}
    assert len(table['i']) > 0 and sum(rows.values()) > 0, rows
    f = ctx.poses_fingerprints(_planes_of(with_planes), n_refs=1)
    tables = ('atom_atom', 'atom_plane') if with_planes else ('atom_atom',)
    s = ctx.poses_shortlist('summary', weights=sl.weights(atom_atom={'records': 1}), k=3, tables=tables)
    K, kept = len(s['pose']), len(s['i'])
    assert len(f['ids']) > 0 and K == 3 and kept > 0
    L, hd = ctx._L, ctx._h

    def fetch_poses():
        t = dict(pose_off=np.zeros(P + 1, np.uint64), i=np.zeros(len(table['i']), np.int32), dist=np.zeros(len(table['i']), np.float32),
                 summary=np.zeros((P, 16), np.uint32))
        n = C.c_int64(-1)
        rc = L.arp_poses_contacts_fetch(hd, len(t['i']), _p(t['pose_off']), _p(t['i']), None, _p(t['dist']), None, None, _p(t['summary']), C.byref(n))
        return rc, b''.join(v.tobytes() for v in t.values())

    def fetch_planes():
        out = []
        for t, name in enumerate(poses.PLANE_TABLES):
            off, first, ct = np.zeros(P + 1, np.uint64), np.zeros(rows[name], np.int32), np.zeros(rows[name], np.uint8)
            byte = [None] * 3
            byte[poses.PLANE_COLUMNS[name][2].index('ctype')] = _p(ct)
            n = C.c_int64(-1)
            rc = L.arp_poses_planes_fetch(hd, t, rows[name], _p(off), _p(first), None, None, None, None, None, *byte, None, C.byref(n))
            if rc != OK:
                return rc, b''
            out += [off.tobytes(), first.tobytes(), ct.tobytes()]
        return OK, b''.join(out)

    def fetch_fingerprint():
        ids, count, cross = np.zeros(len(f['ids']), np.int32), np.zeros(P, np.uint32), np.zeros((P, 1), np.uint32)
        n = C.c_int64(-1)
        rc = L.arp_poses_fingerprints_fetch(hd, len(ids), _p(ids), _p(count), _p(cross), None, None, None, C.byref(n))
        return rc, ids.tobytes() + count.tobytes() + cross.tobytes()

    def fetch_shortlist():
        pose, score, off, i = np.zeros(K, np.int32), np.zeros(K, np.int64), np.zeros(K + 1, np.uint64), np.zeros(kept, np.int32)
        n, m = C.c_int64(-1), C.c_int64(-1)
        rc = L.arp_poses_shortlist_fetch(hd, K, kept, _p(pose), _p(score), None, None, _p(off), _p(i), None, None, None, None, C.byref(n), C.byref(m))
        got = pose.tobytes() + score.tobytes() + off.tobytes() + i.tobytes()
        if rc == OK and with_planes:
            first, poff = np.zeros(len(s['atom_plane']['ctype']), np.int32), np.zeros(K + 1, np.uint64)
            rc = L.arp_poses_shortlist_planes_fetch(hd, 0, K, len(first), _p(poff), _p(first), *([None] * 8), C.byref(m))
            got += first.tobytes() + poff.tobytes()
        return rc, got
    return ctx, dict(poses=fetch_poses, planes=fetch_planes, fingerprint=fetch_fingerprint, shortlist=fetch_shortlist)


def _refused(rc, ctx, word):
    msg = ctx._L.arp_last_error(ctx._h).decode()
    assert rc == E_ARG and word in msg, (rc, msg)


def _other_fingerprint(ctx, with_planes):
    before = ctx.poses_fingerprints_info()['launches']
    ctx.poses_fingerprints(_planes_of(with_planes), n_refs=1, all_pairs=True)      # (the same columns and scores, the matrix besides)
    assert ctx.poses_fingerprints_info()['launches'] == before + 1


def _refused_contacts(ctx, with_planes):
    _, _, x, h = _input()
    n = C.c_int64(0)
    x32 = np.ascontiguousarray(x, np.float32)
    _refused(ctx._L.arp_poses_contacts_launch(ctx._h, P, _p(x32), _p(np.ascontiguousarray(h)), 7.0, 0.1, 0, C.byref(n)), ctx, 'cutoff must be in')


def _refused_planes(ctx, with_planes):
    _refused(ctx._L.arp_poses_planes_launch(ctx._h, P, None, _p(np.zeros(4, np.int64))), ctx, 'xyz missing')


def _refused_fingerprint(ctx, with_planes):
    _refused(ctx._L.arp_poses_fingerprints_launch(ctx._h, 0, 0x7F, 1, 1, _p(np.zeros(8, np.int64))), ctx, 'planes mask of 0')


def _refused_shortlist(ctx, with_planes):
    w = np.zeros(32, np.int32)
    _refused(ctx._L.arp_poses_shortlist_launch(ctx._h, 1, _p(w), 0, None, 0, 0, 3, -(1 << 63), 0, 0, 0x7F, _p(np.zeros(8, np.int64))), ctx, 'tables must be')


# event -> (what it does to the context, the results it voids ('r@planes': only the kind that read the poses-planes result),
#           whether plane atoms are resident afterwards)
EVENTS = {
    'none': (lambda ctx, wp: None, (), True),
    'contacts_again': (lambda ctx, wp: ctx.poses_summary(_input()[2], _input()[3], *PARAMS), ('fingerprint', 'shortlist'), True),
    'planes_again': (lambda ctx, wp: ctx.poses_planes_summary(_input()[2]), ('fingerprint@planes', 'shortlist@planes'), True),
    'set_plane_atoms': (lambda ctx, wp: ctx.set_plane_atoms(_input()[0]), ('planes', 'fingerprint@planes', 'shortlist@planes'), True),
    'set_selection': (lambda ctx, wp: ctx.set_selection(_input()[1]), RESULTS, True),
    'set_complex': (lambda ctx, wp: ctx.set_complex(_input()[0]), RESULTS, False),
    'run_launch': (lambda ctx, wp: ctx.run_launch(5.0), (), True),
    'fingerprint_other_arguments': (_other_fingerprint, (), True),
    'refused_contacts': (_refused_contacts, (), True),
    'refused_planes': (_refused_planes, (), True),
    'refused_fingerprint': (_refused_fingerprint, (), True),
    'refused_shortlist': (_refused_shortlist, (), True),
}


@pytest.mark.gpu
@pytest.mark.parametrize('with_planes', (False, True), ids=('from_poses', 'with_planes'))
@pytest.mark.parametrize('event', list(EVENTS))
def test_an_event_voids_exactly_the_pose_results_that_read_what_it_replaced(event, with_planes):
    ctx, fetch = _make_all(with_planes)
    before = {r: fetch[r]() for r in RESULTS}
    assert all(rc == OK and len(b) > 0 for rc, b in before.values()), {r: rc for r, (rc, _) in before.items()}
    assert ctx.poses_planes_info()['plane_atoms'] is True
    apply, voided, plane_atoms = EVENTS[event]
    apply(ctx, with_planes)
    gone = {r for r in RESULTS if r in voided or (with_planes and r + '@planes' in voided)}
    for r in RESULTS:
        rc, b = fetch[r]()
        if r in gone:
            assert rc == E_ARG, (event, r, rc)
        else:
            assert rc == OK and b == before[r][1], (event, r, rc)
    assert ctx.poses_planes_info()['plane_atoms'] is plane_atoms
    ctx.close()
