"""Library clusters (arp_library_clusters_launch / _fetch / _info, Context.library_clusters, arpeggio_amd.library_clusters,
InteractionComplex.run_library_clusters; csrc/arp_library_clusters.h).

The yardstick is written here and shares no code with ``library_clusters.py`` or ``pose_clusters.py``: ``pose_fingerprints.unpack``
of a ``bits=True`` library-fingerprint fetch gives a Python ``set`` of (node column, plane) per row; global pose t is row Q + t;
t = ``len(a & b)``, q in Python integers; the plain sequential walk — join the FIRST similar leader, else lead while fewer than
``max_clusters`` leaders exist, else stay unassigned.  ``windows_of`` derives, from the yardstick's own answer, the rounds the
window form has to take.  Every comparison is exact, dtypes and shapes included: no tolerance, no time.

Controlled fingerprints come from one-atom ligands on a line of receptor atoms 6 A apart (``line_launch``, ``pool``): pose S(i) sits 3 A
beside atom i and touches it alone; pose P(i) sits midway between atoms i and i + 1, 3 A from both.  Every record is the same
atom pair at the same distance, so q(S(i), S(i)) = q(P(i), P(i)) = 1, q(S(i), P(i)) = q(S(i + 1), P(i)) = 1/2, q(P(i), P(i + 1)) =
1/3 and everything else 0 — asserted on the yardstick where a test relies on it."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_library_planes as tp
import test_library_shortlist as tls
import test_ligand_library as tl
from arpeggio_amd import _capi, synth
from arpeggio_amd import library_clusters as lcl
from arpeggio_amd import library_fingerprints as lfp
from arpeggio_amd import library_shortlist as lsl
from arpeggio_amd import ligand_library as ll
from arpeggio_amd import pose_fingerprints as fp
from arpeggio_amd.core.interactions import InteractionComplex
from helpers import tiny_complex
from test_library_shortlist import ALL15, BIT, PARAMS, _ctx, _p, _same_bytes

ONE = 1 << 32
HALF = 1 << 31
THIRD = 1431655765            # floor(2^32 / 3)
ARRAYS = ('pose', 'ligand', 'cluster', 'similarity', 'leader', 'leader_position', 'size')
ENTRIES = ('arp_library_clusters_launch', 'arp_library_clusters_fetch', 'arp_library_clusters_info')
ALL, LIST, SHORTLIST = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------- yardstick
def feature_sets(result):
    """(sets of the T poses, sets of the Q references) of a library fingerprint fetched with ``bits=True``: pose t is row Q + t."""
    on = fp.unpack(result)
    Q = int(result['n_refs'])
    sets = [set(zip(*(a.tolist() for a in np.nonzero(on[p])))) for p in range(len(on))]
    assert [len(s) for s in sets] == np.asarray(result['count']).tolist()
    return sets[Q:], sets[:Q]


def q_of(a, b):
    t = len(a & b)
    u = len(a) + len(b) - t
    return ONE if u == 0 else (t << 32) // u


def walk(sets, thr, pos, lig_of, max_clusters=256):
    """The sequential definition over the positions ``pos`` (global poses)."""
    cluster, sim, lead, lead_pos, size = [], [], [], [], []
    for m, p in enumerate(pos):
        for c, lp in enumerate(lead):
            v = q_of(sets[p], sets[lp])
            if v >= thr:
                cluster.append(c); sim.append(v); size[c] += 1
                break
        else:
            if len(lead) < max_clusters:
                cluster.append(len(lead)); sim.append(ONE); lead.append(p); lead_pos.append(m); size.append(1)
            else:
                cluster.append(-1); sim.append(-1)
    return dict(pose=np.array(pos, np.int32).reshape(-1), ligand=np.array([lig_of[p] for p in pos], np.int32).reshape(-1),
                cluster=np.array(cluster, np.int32).reshape(-1), similarity=np.array(sim, np.int64).reshape(-1),
                leader=np.array(lead, np.int32).reshape(-1), leader_position=np.array(lead_pos, np.int32).reshape(-1),
                size=np.array(size, np.uint32).reshape(-1), threshold_q32=int(thr), max_clusters=int(max_clusters), unassigned=cluster.count(-1))


def windows_of(want, max_clusters, window=32):
    """The starts of the rounds that elect a leader, from the yardstick's answer alone: a round starts at the lowest position
    that no leader in front of the round's window has taken, and resolves the ``window`` positions from there."""
    cl, lp = want['cluster'].tolist(), want['leader_position'].tolist()
    starts, s, made = [], 0, 0
    while s is not None and made < max_clusters:
        starts.append(s)
        made += sum(1 for x in lp if s <= x < s + window)
        s = next((m for m in range(s + window, len(cl)) if cl[m] < 0 or lp[cl[m]] >= s + window), None)
    return starts


def differences(got, want, keys=ARRAYS + ('threshold_q32', 'max_clusters', 'unassigned')):
    out = []
    for k in keys:
        a, b = got[k], want[k]
        if isinstance(b, np.ndarray):
            if not isinstance(a, np.ndarray) or a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
                out.append(k)
        elif a != b:
            out.append(k)
    return out


def check(ctx, sets, lig_of, thr, order=None, max_clusters=256, source=None):
    """One launch against the yardstick; also the invariants of the result and the rounds ``windows_of`` asks for."""
    source = source or ('all' if order is None else 'list')
    got = ctx.library_clusters(thr, source=source, order=order if source == 'list' else None, max_clusters=max_clusters)
    want = walk(sets, thr, list(range(len(sets))) if order is None else [int(p) for p in order], lig_of, max_clusters)
    assert differences(got, want) == [], (thr, order, max_clusters)
    assert int(got['size'].sum()) + got['unassigned'] == len(got['pose'])
    assert (np.diff(got['leader_position']) > 0).all() and got['leader_position'][0] == 0
    info = ctx.library_clusters_info()
    assert (info['positions'], info['clusters'], info['unassigned'], info['max_clusters'], info['threshold_q32']) == \
        (len(want['pose']), len(want['leader']), want['unassigned'], max_clusters, thr)
    assert info['rounds'] == len(windows_of(want, max_clusters)), (info, windows_of(want, max_clusters))
    return got, want


def pair_values(sets, pos):
    ids = sorted(set(pos))
    return sorted(q_of(sets[a], sets[b]) for k, a in enumerate(ids) for b in ids[k + 1:])


def telling_threshold(sets, pos, lig_of, fracs=(0.5, 0.75, 0.625, 0.875, 0.375, 0.25, 0.9, 0.95)):
    """The first quantile of the yardstick's pair values at which its own clustering has 2 <= C <= M - 1 and a member of a leader
    that is not the latest one: what tells 'first similar' from 'last' or 'most similar'.  Nothing of the code under test is asked."""
    values = pair_values(sets, pos)
    for frac in fracs:
        thr = values[int(frac * (len(values) - 1))]
        w = walk(sets, thr, pos, lig_of, 4096)
        lp, cl = w['leader_position'].tolist(), w['cluster'].tolist()
        # (the latest leader when position m is met is the last one in front of m)
        not_latest = any(cl[m] >= 0 and m not in lp and cl[m] != max(c for c, x in enumerate(lp) if x < m) for m in range(len(cl)))
        if 2 <= len(lp) <= len(pos) - 1 and not_latest:
            return thr, w
    raise AssertionError('no quantile makes this case telling')


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_result():
    """Q = 2 references and T = 4 poses over 3 nodes and one plane, by hand (one word a row):
            row 0  ref 0    {0, 1, 2}
            row 1  ref 1    {2}
            row 2  pose 0   {0, 1}
            row 3  pose 1   {0}
            row 4  pose 2   {2}
            row 5  pose 3   {}
    With the offset forgotten, 'pose 0' would be ref 0 and 'pose 1' ref 1."""
    rows = [0b111, 0b100, 0b011, 0b001, 0b100, 0b000]
    bits = np.array(rows, np.uint64).reshape(6, 1, 1)
    return dict(ids=np.array([3, 7, 9], np.int32), count=np.array([3, 1, 2, 1, 1, 0], np.uint32), cross=np.zeros((6, 2), np.uint32),
                occupancy=np.zeros((3, 1), np.uint32), bits=bits, planes=1, n_refs=2, level='residue')


def test_leader_on_the_hand_made_result():
    r = hand_result()
    lig = [0, 0, 2, 2]                      # ligand 1 has no pose
    assert lcl.ligands_of([0, 2, 2, 4]).tolist() == lig and lcl.ligands_of([0, 2, 2, 4]).dtype == np.int32
    # q(pose 0, pose 1) = 1 / 2; everything else among the poses is 0 (the empty pose 3 against a full one: 0 / n)
    got = lcl.leader(r, HALF, ligand_of=lig)
    assert got['pose'].tolist() == [0, 1, 2, 3] and got['ligand'].tolist() == lig
    assert got['cluster'].tolist() == [0, 0, 1, 2] and got['similarity'].tolist() == [ONE, HALF, ONE, ONE]
    assert got['leader'].tolist() == [0, 2, 3] and got['leader_position'].tolist() == [0, 2, 3] and got['size'].tolist() == [2, 1, 1]
    assert (got['threshold_q32'], got['max_clusters'], got['unassigned']) == (HALF, 256, 0)
    assert all(got[k].dtype == lcl.DTYPES[k] for k in ARRAYS)
    # the same walk over rows 0 ... 3 (the offset forgotten) gives another answer: ref 0 {0, 1, 2} takes pose 0 at 2 / 3
    sets = [{0, 1, 2}, {2}, {0, 1}, {0}]
    wrong = walk(sets, HALF, [0, 1, 2, 3], lig)
    assert wrong['cluster'].tolist() == [0, 1, 0, 2] and wrong['cluster'].tolist() != got['cluster'].tolist()
    # one above 1 / 2: pose 1 stands alone; an order with a repeat; the cap
    assert lcl.leader(r, HALF + 1, ligand_of=lig)['cluster'].tolist() == [0, 1, 2, 3]
    got = lcl.leader(r, HALF, order=[3, 1, 3, 0, 2], ligand_of=lig, max_clusters=2)
    assert got['pose'].tolist() == [3, 1, 3, 0, 2] and got['ligand'].tolist() == [2, 0, 2, 0, 2]
    assert got['cluster'].tolist() == [0, 1, 0, 1, -1] and got['similarity'].tolist() == [ONE, ONE, ONE, HALF, -1]
    assert got['leader'].tolist() == [3, 1] and got['size'].tolist() == [2, 2] and got['unassigned'] == 1
    assert differences(got, walk([{0, 1}, {0}, {2}, set()], HALF, [3, 1, 3, 0, 2], lig, 2)) == []
    assert 'ligand' not in lcl.leader(r, HALF)
    for bad in (dict(order=[4]), dict(order=[-1]), dict(order=[]), dict(ligand_of=[0, 0, 2])):
        with pytest.raises(ValueError):
            lcl.leader(r, HALF, **bad)
    with pytest.raises(ValueError):
        lcl.leader(dict(r, n_refs=6), HALF)


def test_leader_ligands_records_and_the_csv_text(tmp_path):
    lig = [0, 0, 2, 2]
    got = lcl.leader(hand_result(), HALF, order=[3, 1, 3, 0, 2], ligand_of=lig, max_clusters=2)
    assert lcl.leader_ligands(got).tolist() == [2, 0] and lcl.leader_ligands(got).dtype == np.int32
    rec = lcl.to_records(got)
    assert rec[0] == {'type': 'library-cluster', 'position': 0, 'pose': 3, 'ligand': 2, 'cluster': 0, 'leader': 3, 'leader_ligand': 2, 'similarity': 1.0, 'size': 2}
    assert rec[3] == {'type': 'library-cluster', 'position': 3, 'pose': 0, 'ligand': 0, 'cluster': 1, 'leader': 1, 'leader_ligand': 0, 'similarity': 0.5, 'size': 2}
    assert rec[4] == {'type': 'library-cluster', 'position': 4, 'pose': 2, 'ligand': 2, 'cluster': -1, 'leader': None, 'leader_ligand': None,
                      'similarity': None, 'size': 0}
    path = lcl.write_library_clusters(str(tmp_path), 'x', got)
    assert path.endswith('x.libraryclusters')
    assert open(path).read().splitlines() == ['position,pose,ligand,cluster,leader,leader_ligand,similarity,size', '0,3,2,0,3,2,1.0,2', '1,1,0,1,1,0,1.0,2',
                                              '2,3,2,0,3,2,1.0,2', '3,0,0,1,1,0,0.5,2', '4,2,2,-1,,,,0']
    assert lcl.members(got, 1).tolist() == [1, 0] and [a.tolist() for a in lcl.representatives(got)] == [[3, 1], [2, 2]]
    assert lcl.shift(got, 10)['leader'].tolist() == [13, 11] and lcl.threshold_q32(0.5) == HALF and lcl.pair_q32([3], [1], 2, 1) == HALF


def test_the_header_the_binding_and_the_module_agree():
    root = os.path.join(os.path.dirname(__file__), '..')
    hdr = open(os.path.join(root, 'include', 'arpeggio_hip.h')).read()
    src = open(os.path.join(root, 'arpeggio_amd', 'csrc', 'arp_library_clusters.h')).read()
    for s in ENTRIES:
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    assert '#define ARP_LIBCL_WINDOW %d' % lcl.WINDOW in hdr and '#define LCL_WINDOW %d ' % lcl.WINDOW in src
    assert '#define ARP_LIBCL_LDS_WORDS %d' % lcl.LDS_WORDS in hdr and '#define LCL_LDS_WORDS %d ' % lcl.LDS_WORDS in src
    assert (_capi.LIBCL_WINDOW, _capi.LIBCL_LDS_WORDS) == (lcl.WINDOW, lcl.LDS_WORDS) == (32, 2048)
    for code, name in enumerate(('ALL', 'LIST', 'SHORTLIST')):
        assert '#define ARP_LIBCL_%s %d' % (name, code) in hdr and '#define LCL_%s %d' % (name, code) in src
        assert getattr(_capi, 'LIBCL_' + name) == code and lcl.SOURCES[code] == name.lower()
    assert lcl.MAX_CLUSTERS == _capi.POSECL_MAX_CLUSTERS and lcl.MAX_POSES == _capi.POSES_MAX_POSES


def test_run_library_clusters_refuses_a_library_that_one_launch_does_not_hold():
    lig = synth.ligand('ion', 10)
    lib = ll.pack([lig, lig])
    ic = InteractionComplex(synth.config3(500, seed=1))
    too_many = np.array([0, 1 << 19, (1 << 20) + 1], np.int64)
    assert len(ll.chunk_plan(too_many, _capi.POSES_MAX_POSES)) == 2
    with pytest.raises(ValueError, match='does not decompose over launches'):      # (before any array is read or a context made)
        ic.run_library_clusters(lib, too_many, None, None, 5)
    assert ic._ctx is None
    for bad in (dict(by='best'), dict(unit='atoms'), dict(k=0), dict(threshold=1.5), dict(level='chain')):
        kw = dict(k=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            ic.run_library_clusters(lib, np.array([0, 1, 2]), None, None, kw.pop('k'), **kw)


# ------------------------------------------------------------------------------------------------------------- GPU: the pool
def line_receptor(N):
    """N atoms on a line 6 A apart, a residue each."""
    return tiny_complex(np.stack([6.0 * np.arange(N), np.zeros(N), np.zeros(N)], axis=1))


def S(i):
    return ('S', i)


def Pr(i):
    return ('P', i)


FAR = ('far', 0)


def _point(kind):
    name, i = kind
    return {'S': [6.0 * i, 3.0, 0.0], 'P': [6.0 * i + 3.0, 0.0, 0.0], 'far': [0.0, 100.0, 0.0]}[name]


def line_launch(N, kinds, ligand_sizes=None):
    """A context with the line receptor and one-atom ligands (all the same ion) holding the poses ``kinds`` in order, cut into
    ligands of ``ligand_sizes`` poses (default: one ligand); the library result is resident.  Returns (ctx, lig_of, off, x, h)."""
    sizes = [len(kinds)] if ligand_sizes is None else list(ligand_sizes)
    assert sum(sizes) == len(kinds)
    ion = synth.ligand('ion', 10)
    assert ion.n_atoms == 1
    pts = np.array([_point(k) for k in kinds], np.float64).reshape(-1, 3)
    at = np.concatenate([[0], np.cumsum(sizes)])
    ps = [None if b == a else tls._one_atom_poses(pts[a:b]) for a, b in zip(at[:-1], at[1:])]
    lib = ll.pack([ion] * len(sizes))
    ctx = _ctx(line_receptor(N))
    ctx.set_ligand_library(lib)
    off, x, h = ll.flatten_poses(lib, ps)
    ctx.library_summary(off, x, h, *PARAMS)
    lig_of = np.repeat(np.arange(len(sizes)), sizes).tolist()
    return ctx, lig_of, off, x, h


POOL_N = 140


@functools.lru_cache(maxsize=None)
def pool_kinds():
    """Pose i = S(i) for i < 140, pose 140 + i = P(i) for i < 139, then two poses far away (no feature)."""
    return tuple([S(i) for i in range(POOL_N)] + [Pr(i) for i in range(POOL_N - 1)] + [FAR, FAR])


def P(i):
    return POOL_N + i


EMPTY = 2 * POOL_N - 1


def pool(n_refs=0, planes=ALL15):
    """The pool, cut into 41 ligands (ligand 7 without poses); its fingerprint at atom level is resident and fetched."""
    kinds = pool_kinds()
    sizes = [7] * 7 + [0] + [7] * 32 + [len(kinds) - 7 * 39]
    ctx, lig_of, off, x, h = line_launch(POOL_N, kinds, sizes)
    refs = lfp.references([{}] * n_refs) if n_refs else None
    f = ctx.library_fingerprints(refs, planes, by_residue=False, bits=True)
    sets, _ = feature_sets(f)
    # what the docstring of this file says, on the yardstick
    assert q_of(sets[3], sets[3]) == ONE and q_of(sets[3], sets[4]) == 0 and q_of(sets[3], sets[P(3)]) == HALF and q_of(sets[4], sets[P(3)]) == HALF
    assert q_of(sets[P(3)], sets[P(4)]) == THIRD and q_of(sets[P(3)], sets[P(5)]) == 0 and not sets[EMPTY] and not sets[EMPTY + 1] and sets[0]
    assert len(f['ids']) == POOL_N and 7 not in lig_of
    return ctx, lig_of, sets, (off, x, h)


@pytest.mark.gpu
def test_window_seams():
    ctx, lig_of, sets, _ = pool()
    rng = np.random.default_rng(7)
    for M in (1, 2, 31, 32, 33, 63, 64, 65, 97, 130):
        # every position leads: C = M, a round every 32 positions
        got, want = check(ctx, sets, lig_of, 1, order=list(range(M)), max_clusters=4096)
        assert len(want['leader']) == M and ctx.library_clusters_info()['rounds'] == (M + 31) // 32
        # threshold 0: one cluster, one round
        got, want = check(ctx, sets, lig_of, 0, order=list(range(M)))
        assert want['size'].tolist() == [M] and ctx.library_clusters_info()['rounds'] == 1
        # mixed: singles of a few sites with repeats, and pairs that are similar to two sites at once
        few = max(M // 4, 2)
        order = [int(rng.integers(0, few)) if rng.random() < 0.7 else P(int(rng.integers(0, few))) for _ in range(M)]
        got, want = check(ctx, sets, lig_of, HALF, order=order, max_clusters=4096)
        assert M < 3 or len(want['leader']) < M
    ctx.close()


@pytest.mark.gpu
def test_hand_made_window_cases():
    ctx, lig_of, sets, _ = pool()
    first32 = list(range(32))
    # a window position that joins the SECOND leader of its own window
    order = [0, 1, 1]
    got, want = check(ctx, sets, lig_of, HALF, order=order)
    assert want['cluster'].tolist() == [0, 1, 1]
    # a window position already assigned by an earlier sweep: window 1 starts at 32 (site 40); 33 joined site 5 in round 0
    order = first32 + [40, 5, 40, 41]
    got, want = check(ctx, sets, lig_of, HALF, order=order)
    assert windows_of(want, 256) == [0, 32] and want['cluster'].tolist()[32:] == [32, 5, 32, 33]
    # a position behind the window similar to TWO leaders of one window joins the first — in either order of the two
    for a, b in ((10, 11), (11, 10)):
        order = [a if m == 3 else b if m == 20 else 50 + m for m in range(32)] + [P(10), 90]
        assert q_of(sets[P(10)], sets[10]) >= HALF and q_of(sets[P(10)], sets[11]) >= HALF and q_of(sets[10], sets[11]) < HALF
        got, want = check(ctx, sets, lig_of, HALF, order=order)
        assert want['cluster'][32] == 3 and want['leader'][3] == a and want['similarity'][32] == HALF
    # ... and the same inside one window
    got, want = check(ctx, sets, lig_of, HALF, order=[7, 11, 10, P(10), 12])
    assert want['cluster'].tolist() == [0, 1, 2, 1, 3]
    # a position similar to a leader of a LATER window only
    order = first32 + [50] + [m % 32 for m in range(40)] + [50, 51]
    got, want = check(ctx, sets, lig_of, HALF, order=order)
    assert windows_of(want, 256) == [0, 32, 74] and want['cluster'][73] == 32 and want['leader_position'][32] == 32
    # a window whose start lands on M - 1
    order = first32 + [m % 32 for m in range(50)] + [99]
    got, want = check(ctx, sets, lig_of, HALF, order=order)
    assert windows_of(want, 256) == [0, len(order) - 1] and want['leader_position'][-1] == len(order) - 1
    # the similarity is the first similar leader's, not the best one's: S(10) leads, P(10) joins it at 1/2 although P(10) follows
    got, want = check(ctx, sets, lig_of, THIRD, order=[10, P(9), P(10), P(9)])
    assert want['cluster'].tolist() == [0, 0, 0, 0] and want['similarity'].tolist() == [ONE, HALF, HALF, HALF]
    ctx.close()


@pytest.mark.gpu
def test_cap_seams():
    ctx, lig_of, sets, _ = pool()
    inside = behind = after_cap = False
    for C0 in (32, 33, 40):
        # C0 sites in front, then repeats of the latest sites, then of all
        order = list(range(C0)) + [C0 - 1 - (j % 3) for j in range(40)] + [j % C0 for j in range(12)]
        free = walk(sets, HALF, order, lig_of, 4096)
        assert len(free['leader']) == C0 and free['unassigned'] == 0
        for mc in (1, C0 - 1, C0, C0 + 1, 4096):
            want = walk(sets, HALF, order, lig_of, mc)
            starts = windows_of(want, mc)
            away = np.nonzero(want['cluster'] < 0)[0]
            assert (len(away) > 0) == (mc < C0) and len(want['leader']) == min(mc, C0)
            inside |= bool(((away >= starts[-1]) & (away < starts[-1] + 32)).any())
            behind |= bool((away >= starts[-1] + 32).any())
            after_cap |= mc < C0 and len(starts) < len(windows_of(free, 4096))      # (a round the free walk takes does nothing here)
            got, _ = check(ctx, sets, lig_of, HALF, order=order, max_clusters=mc)
            gone = got['cluster'] < 0
            assert (got['similarity'][gone] == -1).all() and (got['similarity'][~gone] >= HALF).all()
    assert inside and behind and after_cap
    ctx.close()


# (N atoms, planes of the mask): W = planes * ceil(N / 64) words.  32 * 64 words are the LDS stage (LDS_WORDS): W = 64 is the
# last staged one, W = 65 the first that comes from L2; at W = 270 a lane of the sweep no longer keeps its row in registers.
WORD_SEAMS = [(63, 1, 1), (63, 2, 2), (63, 3, 3), (63, 5, 5), (64, 15, 15), (500, 8, 64), (300, 13, 65), (1100, 15, 270)]


def test_the_word_seams_stand_on_both_sides_of_the_stage():
    ws = {w for _, _, w in WORD_SEAMS}
    assert ws >= {1, 2, 3, 5, 15, 64, 65, 270} and lcl.LDS_WORDS // lcl.WINDOW in ws and lcl.LDS_WORDS // lcl.WINDOW + 1 in ws
    src = open(os.path.join(os.path.dirname(__file__), '..', 'arpeggio_amd', 'csrc', 'arp_library_clusters.h')).read()
    assert '#define LCL_ROW_REGS 4' in src and max(ws) > 4 * 64


@pytest.mark.gpu
@pytest.mark.parametrize('N,n_planes,W', WORD_SEAMS, ids=[f'N{n}-W{w}' for n, _, w in WORD_SEAMS])
def test_word_seams(N, n_planes, W):
    kinds = [Pr(i) for i in range(N - 1)] + [S(i) for i in range(N)]
    ctx, lig_of, off, x, h = line_launch(N, kinds)
    table = ctx.library_contacts(off, x, h, *PARAMS)
    common = int(np.bitwise_and.reduce(table['sift'].astype(np.int64)))
    assert common != 0                                          # every record is the same pair at the same distance
    mask = common & -common                                     # one bit every record has, then filler bits
    for k in range(15):
        if bin(mask).count('1') < n_planes:
            mask |= 1 << k
    assert bin(mask).count('1') == n_planes
    f = ctx.library_fingerprints(None, mask, by_residue=False, bits=True)
    assert f['bits'].shape == (2 * N - 1, n_planes, (N + 63) // 64) and len(f['ids']) == N
    sets, _ = feature_sets(f)
    T = 2 * N - 1
    few = 256 if N <= 64 else 40      # (the long lines: two rounds, the rest unassigned — the yardstick stays quick)
    for order in (None, list(range(T - 1, -1, -1))):
        got, want = check(ctx, sets, lig_of, HALF, order=order, max_clusters=few)
        assert ctx.library_clusters_info()['words'] == W and len(want['leader']) >= 2 and int(want['size'].max()) >= 2
        if order is not None:
            # descending: S(N - 1) leads, and P(N - 2) — whose shared bit is the LAST bit of the last word — joins it
            assert order[0] == T - 1 and want['cluster'][order.index(N - 2)] == 0 and want['similarity'][order.index(N - 2)] == HALF
    # a short order in the last word alone
    check(ctx, sets, lig_of, HALF, order=[T - 1, N - 2, T - 2, N - 3, T - 1, 0])
    ctx.close()


@pytest.mark.gpu
def test_reference_rows_do_not_change_the_result():
    ctx, lig_of, sets, (off, x, h) = pool()
    table = ctx.library_contacts(off, x, h, *PARAMS)
    refs = [lfp.reference_from_pose(table, t, level='atom') for t in (3, P(3), 0)]
    orders = (None, [3, 4, P(3), P(4), 3, 0, EMPTY], list(range(99, -1, -1)) + [P(i) for i in range(60)])
    results = []
    for Q in (0, 1, 3):
        f = ctx.library_fingerprints(lfp.references(refs[:Q]), ALL15, by_residue=False, bits=True)
        now, ref_sets = feature_sets(f)
        assert f['n_refs'] == Q and len(f['count']) == Q + len(sets) and now == sets
        assert all(q_of(r, sets[t]) == ONE for r, t in zip(ref_sets, (3, P(3), 0)))      # the references ARE similar to poses
        results.append([check(ctx, now, lig_of, thr, order=o, max_clusters=64)[0] for thr in (HALF, THIRD) for o in orders])
    assert _same_bytes(results[1], results[0]) and _same_bytes(results[2], results[0])
    ctx.close()


@pytest.mark.gpu
def test_sources():
    ctx, lig_of, sets, (off, x, h) = pool(n_refs=0)
    T = len(sets)
    rng = np.random.default_rng(3)
    check(ctx, sets, lig_of, HALF, max_clusters=4096)                                   # all
    perm = rng.permutation(T).tolist()
    for order in (perm, perm[:T // 3], [2, 0, 2, 1, 0]):                                  # list
        check(ctx, sets, lig_of, HALF, order=order, max_clusters=4096)
    # shortlist: the same clusters as the list over the shortlist's fetched poses
    table = ctx.library_contacts(off, x, h, *PARAMS)
    ctx.library_fingerprints(lfp.references([lfp.reference_from_pose(table, P(20), level='atom')]), ALL15, by_residue=False)
    w = lsl.weights(atom_atom={'records': 1})
    n_cand = {'poses': T, 'ligands': 40}
    for unit in lsl.UNITS:
        for kw in (dict(kind='summary', weights=w), dict(kind='tanimoto', ref=0)):
            for k in (1, 33, n_cand[unit]):
                short = ctx.library_shortlist(kw['kind'], unit=unit, k=k, **{a: b for a, b in kw.items() if a != 'kind'})
                assert len(short['pose']) == k
                got, want = check(ctx, sets, lig_of, HALF, order=short['pose'].tolist(), max_clusters=4096, source='shortlist')
                assert np.array_equal(got['ligand'], short['ligand'])
                # the positions were materialised: another shortlist leaves the clusters as they are
                before = _resident(ctx)
                ctx.library_shortlist('list', pose_ids=[5, 4])
                assert before[0] == _capi.ARP_OK and _same_resident(_resident(ctx), before) and _same_bytes(before[2], {a: got[a] for a in ARRAYS})
    assert len(set(short['score'].tolist())) > 1
    ctx.close()


@pytest.mark.gpu
def test_no_feature_empty_poses_and_a_ligand_without_poses():
    # U = 0: every pose far away — no column, no word, no bit matrix: one cluster of all
    ctx, lig_of, off, x, h = line_launch(4, [FAR] * 40, [13, 0, 27])
    f = ctx.library_fingerprints(None, ALL15, by_residue=False, bits=True)
    assert f['bits'].shape == (40, 15, 0) and not f['count'].any()
    sets, _ = feature_sets(f)
    for thr in (0, HALF, ONE):
        got, _ = check(ctx, sets, lig_of, thr)
        assert got['cluster'].tolist() == [0] * 40 and got['similarity'].tolist() == [ONE] * 40 and got['size'].tolist() == [40]
        assert got['ligand'].tolist() == [0] * 13 + [2] * 27 and ctx.library_clusters_info()['words'] == 0
    check(ctx, sets, lig_of, ONE, order=[39, 39, 1])
    ctx.close()
    # empty poses among full ones: similar to nothing but another empty pose, which joins at 0 / 0 = 1.0
    ctx, lig_of, sets, _ = pool()
    for thr in (1, HALF, ONE):
        got, _ = check(ctx, sets, lig_of, thr, order=[0, 1, EMPTY, 2, P(0), EMPTY + 1, 0])
        c = int(got['cluster'][2])
        assert got['leader'][c] == EMPTY and got['cluster'][5] == c and got['similarity'][5] == ONE and got['size'][c] == 2
    assert check(ctx, sets, lig_of, 0, order=[0, EMPTY, 1])[0]['size'].tolist() == [3]
    assert 7 not in check(ctx, sets, lig_of, HALF, max_clusters=4096)[0]['ligand'].tolist()      # the ligand without poses
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('by_residue', (True, False), ids=('residue', 'atom'))
def test_main_case(by_residue):
    rec, ligs, ps, lib, ctx, table = tls.main_launch()
    lo = table['ligand_pose_off']
    lig_of = lcl.ligands_of(lo).tolist()
    assert len(ligs) == 7 and np.diff(lo).tolist() == list(tl.MAIN_P) and 3 not in lig_of
    f = ctx.library_fingerprints(lfp.references([lfp.reference_from_pose(table, int(lo[2]), rec.res_id if by_residue else None,
                                                                         level='residue' if by_residue else 'atom')]),
                                 ALL15, by_residue=by_residue, bits=True)
    sets, _ = feature_sets(f)
    T = len(sets)
    thr, free = telling_threshold(sets, list(range(T)), lig_of)
    got, want = check(ctx, sets, lig_of, thr, max_clusters=4096)
    assert differences(got, free) == [] and differences(lcl.leader(f, thr, ligand_of=lig_of, max_clusters=4096), free) == []
    order = list(range(T - 1, -1, -1))
    got, _ = check(ctx, sets, lig_of, thr, order=order, max_clusters=5)
    assert differences(lcl.leader(f, thr, order=order, ligand_of=lig_of, max_clusters=5), got) == []
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: protocol
def _launch(ctx, source=ALL, thr=HALF, ids=None, max_clusters=256, n_order=None):
    info = np.zeros(8, np.int64)
    i = None if ids is None else np.ascontiguousarray(ids, np.int32)
    rc = ctx._L.arp_library_clusters_launch(ctx._h, source, _p(i), (0 if i is None else len(i)) if n_order is None else n_order, thr, max_clusters, _p(info))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), info


def _resident(ctx):
    """The resident library clusters, fetched without a launch: (rc, message, arrays)."""
    info = ctx.library_clusters_info()
    M, Cn = info['positions'], info['clusters']
    out = dict(pose=np.empty(M, np.int32), ligand=np.empty(M, np.int32), cluster=np.empty(M, np.int32), similarity=np.empty(M, np.int64),
               leader=np.empty(Cn, np.int32), leader_position=np.empty(Cn, np.int32), size=np.empty(Cn, np.uint32))
    n, m = C.c_int64(-1), C.c_int64(-1)
    rc = ctx._L.arp_library_clusters_fetch(ctx._h, M, Cn, *[_p(out[k]) for k in ARRAYS], C.byref(n), C.byref(m))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), out


def _same_resident(a, b):
    return a[0] == b[0] and _same_bytes(a[2], b[2])


NO_RESULT = dict(positions=0, clusters=0, unassigned=0, max_clusters=0, words=0, rounds=0, threshold_q32=0)


def _main_ctx():
    rec, ligs, ps = tp.case_main()
    rec_gpu = tp.device_planes(rec)
    ctx, lib = tp.library_ctx(rec_gpu, ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    return rec, rec_gpu, ligs, lib, ctx, off, x, h


@pytest.mark.gpu
def test_every_refusal_names_its_cause_in_order_and_touches_nothing():
    rec, rec_gpu, ligs, lib, ctx, off, x, h = _main_ctx()
    T = int(off[-1])
    w = lsl.weights(atom_atom={'records': 1})
    bad = dict(thr=ONE + 1, max_clusters=0, source=7, ids=[T], n_order=5)      # everything wrong at once: the FIRST cause is named
    rc, msg, _ = _launch(ctx, **bad)
    assert rc == _capi.ARP_E_ARG and 'no library result' in msg
    ctx.library_summary(off, x, h, *PARAMS)
    rc, msg, _ = _launch(ctx, **bad)
    assert rc == _capi.ARP_E_ARG and 'no library fingerprint' in msg
    ctx.library_fingerprints(lfp.references([{3: 0x7FFF}]), ALL15)
    good = ctx.library_clusters(HALF, source='list', order=[5, 1, 5, T - 1, 2])
    launches = ctx.library_clusters_info()['launches']
    before = _resident(ctx)
    assert before[0] == _capi.ARP_OK and np.array_equal(before[2]['pose'], good['pose']) and launches == 1

    def refused(word, **kw):
        rc, msg, info = _launch(ctx, **kw)
        assert rc == _capi.ARP_E_ARG and word in msg, (word, rc, msg)
        assert _same_resident(_resident(ctx), before) and ctx.library_clusters_info()['launches'] == launches, word
    # in the documented order: each call keeps the faults BEHIND the one that is named
    refused('threshold_q32', thr=ONE + 1, max_clusters=0, source=7, ids=[T], n_order=5)
    refused('max_clusters', max_clusters=0, source=7, ids=[T], n_order=5)
    refused('max_clusters', max_clusters=4097)
    refused('unknown source', source=7, ids=[T], n_order=5)
    refused('unknown source', source=-1)
    refused('order missing', source=LIST, ids=None, n_order=3)
    refused('n_order must be', source=LIST, ids=[T], n_order=0)
    refused('n_order must be', source=LIST, ids=[0], n_order=(1 << 20) + 1)
    refused('outside [0, T)', source=LIST, ids=[0, T])
    refused('outside [0, T)', source=LIST, ids=[-1])
    refused('ARP_LIBCL_LIST alone', source=ALL, ids=[0])
    refused('ARP_LIBCL_LIST alone', source=ALL, ids=None, n_order=1)
    refused('ARP_LIBCL_LIST alone', source=SHORTLIST, ids=[0])
    refused('no library shortlist', source=SHORTLIST)
    ctx.library_shortlist('summary', unit='poses', weights=w, k=5, min_score=1 << 40)      # a valid shortlist without an entry
    assert ctx.library_shortlist_info()['chosen'] == 0
    refused('shortlist is empty', source=SHORTLIST)
    # a pass that is pending
    sel = np.zeros(rec.n_atoms, np.uint8)
    sel[:30] = 1
    ctx.set_selection(sel)
    ctx.run_enqueue(5.0, 0.1, False)
    refused('has not been waited for', thr=ONE + 1)                   # before everything else
    ctx.run_wait()
    # NULL arguments
    assert ctx._L.arp_library_clusters_launch(None, ALL, None, 0, HALF, 256, _p(np.zeros(8, np.int64))) == _capi.ARP_E_ARG
    assert ctx._L.arp_library_clusters_launch(ctx._h, ALL, None, 0, HALF, 256, None) == _capi.ARP_E_ARG
    assert ctx._L.arp_library_clusters_info(ctx._h, None) == _capi.ARP_E_ARG
    assert _same_resident(_resident(ctx), before)
    assert _same_bytes(ctx.library_clusters(HALF, source='list', order=[5, 1, 5, T - 1, 2]), good)
    ctx.close()


@pytest.mark.gpu
def test_the_clusters_go_with_the_library_result_and_with_nothing_else():
    rec, rec_gpu, ligs, lib, ctx, off, x, h = _main_ctx()
    w = lsl.weights(atom_atom={'records': 1})
    none = dict(NO_RESULT, launches=0)
    rc, msg, _ = _resident(ctx)
    assert rc == _capi.ARP_E_ARG and 'no result' in msg and ctx.library_clusters_info() == none

    def made():
        ctx.library_summary(off, x, h, *PARAMS)
        ctx.library_fingerprints(lfp.references([{3: 0x7FFF}]), ALL15)
        ctx.library_clusters(HALF, max_clusters=8)
        return _resident(ctx)[0] == _capi.ARP_OK
    assert made()
    first = _resident(ctx)
    # not with set_selection, a later fingerprint (other arguments), a later shortlist, the planes entries or the best tables
    sel = np.zeros(rec.n_atoms, np.uint8)
    sel[:5] = 1
    ctx.set_selection(sel)
    ctx.library_fingerprints(lfp.references([{}, {}]), BIT['hbond'], by_residue=False)
    ctx.library_shortlist('summary', weights=w, k=3)
    ctx.library_planes_summary(off, x)
    ctx.set_ligand_library_planes(lib)
    ctx.library_best(np.ones(16, np.int32))
    ctx.library_fingerprints_best()
    assert _same_resident(_resident(ctx), first)
    launches = ctx.library_clusters_info()['launches']
    # a new library launch (the same poses again: still a new result), a new library, a new structure, models, a batch
    ctx.library_summary(off, x, h, *PARAMS)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and ctx.library_clusters_info() == dict(none, launches=launches)
    assert made() and _same_resident(_resident(ctx), first)
    ctx.set_ligand_library(lib)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and made()
    ctx.set_complex(rec_gpu)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and made()
    ctx.set_topology(rec_gpu)
    assert _resident(ctx)[0] == _capi.ARP_OK                          # (the kept topology is not the resident structure)
    ctx.set_models(np.stack([rec_gpu.xyz, rec_gpu.xyz]), np.stack([rec_gpu.h_xyz, rec_gpu.h_xyz]))
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.set_complex(rec_gpu)
    assert made()
    ctx.set_batch([rec_gpu, rec_gpu], [sel, sel])
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.close()


@pytest.mark.gpu
def test_a_launch_voids_nothing():
    from test_pose_clusters import _resident as pose_clusters_resident
    rec, rec_gpu, ligs, lib, ctx, off, x, h = _main_ctx()
    hem = np.nonzero(rec.res_id == int(np.nonzero(np.array(rec.res_name) == 'HEM')[0][0]))[0]
    sel = np.zeros(rec.n_atoms, np.uint8)
    sel[hem] = 1
    ctx.set_selection(sel)
    counts = ctx.run_launch(5.0, 0.1, False)
    px, ph = synth.poses_of(rec, hem, 6, seed=11, shift=2.0)
    ctx.poses_contacts(px, ph, 5.0, 0.1, False)
    ctx.poses_fingerprints(ALL15, n_refs=0)
    ctx.poses_clusters(HALF)
    T, L = int(off[-1]), len(ligs)
    ctx.library_contacts(off, x, h, *PARAMS)
    ctx.library_planes(off, x)
    ctx.library_best(np.ones(16, np.int32))
    ctx.library_fingerprints(lfp.references([{3: 0x7FFF}, {}]), ALL15)
    ctx.library_fingerprints_best()
    ctx.library_shortlist('summary', weights=lsl.weights(atom_atom={'records': 1}), k=4)

    def everything():
        return (tls._fetch_everything(ctx), tls._library_fetch(ctx, T), tls._library_best_fetch(ctx, L), tls._library_planes_fetch(ctx, T),
                tls._library_fp_fetch(ctx, L), tls._resident(ctx)[2], pose_clusters_resident(ctx)[2])
    before = everything()
    assert counts['atom_atom'] > 0 and len(before[1]['i']) > 0 and len(before[5]['pose']) == 4 and len(before[6]['pose']) == 6
    assert tls._resident(ctx)[0] == _capi.ARP_OK and pose_clusters_resident(ctx)[0] == _capi.ARP_OK
    fp_launches, sl_launches = ctx.library_fingerprints_info()['launches'], ctx.library_shortlist_info()['launches']
    for kw in (dict(source='all'), dict(source='list', order=[3, 3, 0, T - 1]), dict(source='shortlist', max_clusters=2)):
        got = ctx.library_clusters(HALF, **kw)
        assert len(got['pose']) in (T, 4)
        assert _same_bytes(everything(), before)
        assert ctx.library_fingerprints_info()['launches'] == fp_launches and ctx.library_shortlist_info()['launches'] == sl_launches
        assert ctx.library_info()['best'] and ctx.poses_clusters_info()['positions'] == 6
    st = ctx.stats()
    assert (st['libcl_positions'], st['libcl_clusters'], st['libcl_launches']) == (4, len(got['leader']), 3) and st['posecl_positions'] == 6
    ctx.close()


@pytest.mark.gpu
def test_null_pointers_capacity_and_a_caller_owned_stream():
    from test_gpu_paths import _hip_runtime
    rec, rec_gpu, ligs, lib, ctx, off, x, h = _main_ctx()
    ctx.library_summary(off, x, h, *PARAMS)
    ctx.library_fingerprints(lfp.references([{3: 0x7FFF}]), ALL15)
    want = ctx.library_clusters(HALF, max_clusters=6)
    M, Cn = len(want['pose']), len(want['leader'])
    assert M == int(off[-1]) and Cn >= 2
    L, hd = ctx._L, ctx._h
    n, m = C.c_int64(0), C.c_int64(0)
    none = [None] * 7
    assert L.arp_library_clusters_fetch(hd, 0, 0, *none, C.byref(n), C.byref(m)) == _capi.ARP_OK and (n.value, m.value) == (M, Cn)
    assert L.arp_library_clusters_fetch(hd, 0, 0, *none, None, C.byref(m)) == _capi.ARP_E_ARG
    assert L.arp_library_clusters_fetch(hd, 0, 0, *none, C.byref(n), None) == _capi.ARP_E_ARG
    assert L.arp_library_clusters_fetch(None, 0, 0, *none, C.byref(n), C.byref(m)) == _capi.ARP_E_ARG
    for slot, key in enumerate(ARRAYS):
        buf = np.full(want[key].shape, 7, want[key].dtype)
        args = list(none)
        args[slot] = _p(buf)
        per_position = key in lcl.PER_POSITION
        short, other = ((M - 1, Cn), (M, 0)) if per_position else ((M, Cn - 1), (0, Cn))
        n.value = m.value = 0
        assert L.arp_library_clusters_fetch(hd, *short, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_CAPACITY, key
        assert (n.value, m.value) == (M, Cn) and (buf == 7).all() and ('cap_positions' if per_position else 'cap_clusters') in L.arp_last_error(hd).decode()
        assert L.arp_library_clusters_fetch(hd, *other, *args, C.byref(n), C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, want[key]), key
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    ctx.library_summary(off, x, h, *PARAMS)
    ctx.library_fingerprints(lfp.references([{3: 0x7FFF}]), ALL15)
    assert _same_bytes(ctx.library_clusters(HALF, max_clusters=6), want)
    ctx.use_stream(0)                                                 # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------------------------------------------------- GPU: end to end
@pytest.mark.gpu
def test_run_library_clusters_end_to_end(tmp_path):
    rec, ligs, ps = tl.case_main()
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    ic = InteractionComplex(copy.copy(rec))
    full = ic.run_ligand_library(ligs, ps, *PARAMS)
    lo = full['ligand_pose_off']
    lig_of = lcl.ligands_of(lo).tolist()
    # the yardstick's sources, from a context of its own: the fingerprint's sets and the ranking
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    ctx.library_summary(off, x, h, *PARAMS)
    ref = lfp.reference_from_pose(full, int(lo[2]) + 1, rec.res_id)
    sets, _ = feature_sets(ctx.library_fingerprints(lfp.references([ref]), lfp.planes(None), bits=True))
    fpr = ctx.library_fingerprints(lfp.references([ref]), lfp.planes(None))
    ctx.close()
    w = lsl.weights(atom_atom={'records': 1})
    thr = lcl.threshold_q32(0.4)
    cases = (('summary', 'poses', 40, tls.pose_scores('summary', full, w)), ('summary', 'ligands', 6, tls.pose_scores('summary', full, w)),
             ('tanimoto', 'poses', 30, tls.pose_scores('tanimoto', fpr=fpr, ref=0)))
    for by, unit, k, score in cases:
        chosen = tls.ranked(score, lo, unit, k)
        want = walk(sets, thr, chosen, lig_of, 16)
        assert len(chosen) == k and (unit == 'ligands' or 2 <= len(want['leader']) < k)
        got = ic.run_library_clusters(lib, off, x, h, k, threshold=0.4, by=by, unit=unit, weights=w if by == 'summary' else None, refs=[ref],
                                      max_clusters=16, records=True)
        assert differences(got, want) == [] and (got['by'], got['unit']) == (by, unit) and ic.library_clusters is got
        # only the representatives' records, and exactly those the full route has for them
        reps = got['representatives']
        took = lsl.take(full, got['leader'].tolist())
        assert np.array_equal(reps['pose'], got['leader']) and np.array_equal(reps['ligand'], lcl.leader_ligands(got))
        assert all(_same_bytes(reps[c], took[c]) for c in ll.COLUMNS + ('pose_off', 'summary', 'ligand'))
    # refs may be empty by summary
    got = ic.run_library_clusters(ligs, off, x, h, 40, threshold=0.4, unit='poses', max_clusters=16)
    by_records = walk(feature_sets_without_refs(rec, lib, off, x, h), thr, tls.ranked(cases[0][3], lo, 'poses', 40), lig_of, 16)
    assert differences(got, by_records) == [] and 'representatives' not in got
    path = ic.write_library_clusters(str(tmp_path))
    lines = open(path).read().splitlines()
    assert path.endswith('.libraryclusters') and len(lines) == 1 + 40 and lines[0] == ','.join(lcl.CSV_HEADER)
    assert lines[1].split(',')[:4] == ['0', str(got['pose'][0]), str(got['ligand'][0]), '0']


def feature_sets_without_refs(rec, lib, off, x, h):
    ctx = _ctx(rec)
    ctx.set_ligand_library(lib)
    ctx.library_summary(off, x, h, *PARAMS)
    sets, refs = feature_sets(ctx.library_fingerprints(None, lfp.planes(None), bits=True))
    ctx.close()
    assert refs == []
    return sets
