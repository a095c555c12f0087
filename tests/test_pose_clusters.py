"""Pose clusters (arp_poses_clusters_launch / _fetch / _info, Context.poses_clusters, arpeggio_amd.pose_clusters,
InteractionComplex.run_pose_clusters).

The yardstick is written here and shares no code with ``pose_clusters.py``: ``pose_fingerprints.unpack`` of a ``bits=True`` fetch
gives a Python ``set`` of (node, plane) per pose; t = ``len(a & b)``, q in Python integers; the sequential walk — join the FIRST
similar leader, else lead while fewer than ``max_clusters`` leaders exist, else stay unassigned.  Every comparison is exact,
dtypes and shapes included: no tolerance, no time."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, pose_clusters as cl, pose_fingerprints as fp, pose_shortlist as sl, poses
from arpeggio_amd.core.interactions import InteractionComplex
from test_pose_fingerprints import ALL15, BIT, PARAMS, SCATTERED, _ctx, _mask, _p, _same_bytes, chain_case, hem_case, water_case

ONE = 1 << 32
HALF = 1 << 31
THIRD = 1431655765            # floor(2^32 / 3)
ARRAYS = ('pose', 'cluster', 'similarity', 'leader', 'leader_position', 'size')


# ------------------------------------------------------------------------------------------------------------- yardstick
def feature_sets(result):
    """A set of (node column, plane) per pose of a fingerprint result fetched with ``bits=True``."""
    on = fp.unpack(result)
    sets = [set(zip(*(a.tolist() for a in np.nonzero(on[p])))) for p in range(len(on))]
    assert [len(s) for s in sets] == np.asarray(result['count']).tolist()
    return sets


def q_of(a, b):
    t = len(a & b)
    u = len(a) + len(b) - t
    return ONE if u == 0 else (t << 32) // u


def positions_of(P, order=None, skip=0):
    return list(range(skip, P)) if order is None else [int(p) for p in order]


def walk(sets, thr, pos, max_clusters=256, q=None):
    """The sequential definition over the positions ``pos`` (pose ids).  Also ``not_latest``: the positions that joined a leader
    other than the latest one made."""
    q = q or (lambda a, b: q_of(sets[a], sets[b]))
    cluster, sim, lead, lead_pos, size, not_latest = [], [], [], [], [], []
    for m, p in enumerate(pos):
        for c, lp in enumerate(lead):
            v = q(p, lp)
            if v >= thr:
                cluster.append(c); sim.append(v); size[c] += 1
                if c != len(lead) - 1:
                    not_latest.append(m)
                break
        else:
            if len(lead) < max_clusters:
                cluster.append(len(lead)); sim.append(ONE); lead.append(p); lead_pos.append(m); size.append(1)
            else:
                cluster.append(-1); sim.append(-1)
    return dict(pose=np.array(pos, np.int32).reshape(-1), cluster=np.array(cluster, np.int32).reshape(-1), similarity=np.array(sim, np.int64).reshape(-1),
                leader=np.array(lead, np.int32).reshape(-1), leader_position=np.array(lead_pos, np.int32).reshape(-1),
                size=np.array(size, np.uint32).reshape(-1), threshold_q32=int(thr), max_clusters=int(max_clusters), unassigned=cluster.count(-1),
                not_latest=not_latest)


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


def pair_values(sets, pos):
    """The off-diagonal pair values of the distinct poses in ``pos``, ascending."""
    ids = sorted(set(pos))
    return sorted(q_of(sets[a], sets[b]) for k, a in enumerate(ids) for b in ids[k + 1:])


def quantile(values, frac):
    return values[int(frac * (len(values) - 1))]


def telling(w, M):
    """What a case needs to tell 'first similar' from 'last' or 'most similar'."""
    return 2 <= len(w['leader']) <= M - 1 and int(w['size'].max()) >= 2 and len(w['not_latest']) > 0


def telling_threshold(sets, pos, fracs=(0.5, 0.75, 0.625, 0.875, 0.375, 0.25, 0.9, 0.95)):
    """The first quantile in ``fracs`` of the yardstick's pair values at which the yardstick's own clustering is ``telling``:
    the median where that does, the later entries for the cases where it does not.  Nothing of the code under test is asked."""
    values = pair_values(sets, pos)
    for frac in fracs:
        thr = quantile(values, frac)
        w = walk(sets, thr, pos, 4096)
        if telling(w, len(pos)):
            return thr, w
    raise AssertionError('no quantile makes this case telling')


def check(ctx, sets, thr, order=None, skip=0, max_clusters=256, P=None):
    got = ctx.poses_clusters(thr, order=order, skip=skip, max_clusters=max_clusters)
    want = walk(sets, thr, positions_of(len(sets) if P is None else P, order, skip), max_clusters)
    assert differences(got, want) == [], (thr, order, skip, max_clusters)
    assert int(got['size'].sum()) + got['unassigned'] == len(got['pose'])
    assert (np.diff(got['leader_position']) > 0).all() and got['leader_position'][0] == 0
    return got, want


# ------------------------------------------------------------------------------------------------------------- CPU
def test_threshold_q32():
    assert cl.threshold_q32(0.0) == 0 and cl.threshold_q32(1.0) == ONE and cl.threshold_q32(0.5) == HALF and cl.threshold_q32(1) == ONE
    # 1/3 as a float is 6004799503160661 / 2^54, a little BELOW 1/3: times 2^32 is 1431655765.33..., the ceiling 1431655766
    assert (1.0 / 3.0).as_integer_ratio() == (6004799503160661, 1 << 54)
    assert cl.threshold_q32(1.0 / 3.0) == -((-6004799503160661 * ONE) // (1 << 54)) == THIRD + 1
    assert cl.threshold_q32(np.float32(0.25)) == 1 << 30 and cl.threshold_q32(2.0 ** -40) == 1      # the smallest q with q / 2^32 >= t
    for bad in (-0.1, 1.0000001, float('nan'), float('inf'), '0.5', None, True, [0.5]):
        with pytest.raises(ValueError):
            cl.threshold_q32(bad)


def test_pair_q32():
    z = np.zeros(2, np.uint64)
    assert cl.pair_q32(z, z, 0, 0) == ONE                                    # 0 / 0 is 1.0
    a = np.array([0b1011, 1 << 63], np.uint64)
    assert cl.pair_q32(a, a, 4, 4) == ONE                                    # t = u
    b = np.array([0b0110, 0], np.uint64)                                     # shares one bit; u = 4 + 2 - 1 = 5
    assert cl.pair_q32(a, b, 4, 2) == ONE // 5
    assert cl.pair_q32(np.array([0b01], np.uint64), np.array([0b11], np.uint64), 1, 2) == HALF
    assert cl.pair_q32(np.array([0b011], np.uint64), np.array([0b110], np.uint64), 2, 2) == THIRD == 1431655765      # 1 / 3
    assert cl.pair_q32(z, a, 0, 4) == 0
    with pytest.raises(ValueError):
        cl.pair_q32(z, np.zeros(3, np.uint64), 0, 0)


def hand_result():
    """Five poses over four features (one node word, one plane), every number by hand.
        pose 0   1 1 0 0      pose 1   0 1 1 0      pose 2   1 1 1 0      pose 3   . . . .      pose 4   0 0 1 1
        q(0,1) = 1/3   q(0,2) = 2/3   q(1,2) = 2/3   q(0,4) = 0   q(1,4) = 1/3   q(2,4) = 1/4   q(3, x) = 0, q(3,3) = 1"""
    bits = np.array([0b0011, 0b0110, 0b0111, 0, 0b1100], np.uint64).reshape(5, 1, 1)
    return dict(ids=np.arange(4, dtype=np.int32), count=np.array([2, 2, 3, 0, 2], np.uint32), bits=bits, planes=1, n_refs=0, level='atom')


def test_leader_on_the_hand_made_result():
    r = hand_result()
    two_thirds = (2 << 32) // 3
    # threshold 1/2: 0 leads; 1 (1/3 to 0) leads; 2 is similar to BOTH leaders (2/3, 2/3) and joins the first; 3 (no feature) is
    # similar to nothing and leads; 4 (0, 1/3, 0) leads
    got = cl.leader(r, HALF)
    want = dict(pose=np.arange(5, dtype=np.int32), cluster=np.array([0, 1, 0, 2, 3], np.int32), similarity=np.array([ONE, ONE, two_thirds, ONE, ONE], np.int64),
                leader=np.array([0, 1, 3, 4], np.int32), leader_position=np.array([0, 1, 3, 4], np.int32), size=np.array([2, 1, 1, 1], np.uint32),
                threshold_q32=HALF, max_clusters=256, unassigned=0)
    assert differences(got, want) == [] and sorted(got) == sorted(want)
    # max_clusters = 2: 3 and 4 find no leader and no room
    got = cl.leader(r, HALF, max_clusters=2)
    want = dict(pose=np.arange(5, dtype=np.int32), cluster=np.array([0, 1, 0, -1, -1], np.int32), similarity=np.array([ONE, ONE, two_thirds, -1, -1], np.int64),
                leader=np.array([0, 1], np.int32), leader_position=np.array([0, 1], np.int32), size=np.array([2, 1], np.uint32),
                threshold_q32=HALF, max_clusters=2, unassigned=2)
    assert differences(got, want) == []
    # an order with a repeated id, the empty pose first and again: 3 leads, 3 joins itself (0 / 0), 2 leads, 0 joins 2, 2 joins 2
    got = cl.leader(r, HALF, order=[3, 3, 2, 0, 2])
    want = dict(pose=np.array([3, 3, 2, 0, 2], np.int32), cluster=np.array([0, 0, 1, 1, 1], np.int32), similarity=np.array([ONE, ONE, ONE, two_thirds, ONE], np.int64),
                leader=np.array([3, 2], np.int32), leader_position=np.array([0, 2], np.int32), size=np.array([2, 3], np.uint32),
                threshold_q32=HALF, max_clusters=256, unassigned=0)
    assert differences(got, want) == []
    # the >= seam at floor(2^32 / 3): 1 joins 0 at the value itself, not one above; skip leaves pose 0 out
    assert cl.leader(r, THIRD)['cluster'].tolist() == [0, 0, 0, 1, 2] and cl.leader(r, THIRD + 1)['cluster'].tolist() == [0, 1, 0, 2, 3]
    got = cl.leader(r, THIRD, skip=1)
    assert got['pose'].tolist() == [1, 2, 3, 4] and got['cluster'].tolist() == [0, 0, 1, 0] and got['similarity'].tolist() == [ONE, two_thirds, ONE, THIRD]
    assert cl.leader(r, 0)['size'].tolist() == [5] and cl.leader(r, ONE)['cluster'].tolist() == [0, 1, 2, 3, 4]
    # the yardstick of this file says the same
    sets = feature_sets(r)
    for thr in (0, THIRD, THIRD + 1, HALF, ONE):
        for kw in (dict(), dict(max_clusters=2), dict(order=[3, 3, 2, 0, 2]), dict(skip=2)):
            w = walk(sets, thr, positions_of(5, kw.get('order'), kw.get('skip', 0)), kw.get('max_clusters', 256))
            assert differences(cl.leader(r, thr, **kw), w) == [], (thr, kw)
    for bad in (dict(threshold_q32=ONE + 1), dict(threshold_q32=-1), dict(max_clusters=0), dict(max_clusters=4097), dict(skip=5), dict(skip=-1),
                dict(order=[0, 5]), dict(order=[-1]), dict(order=[]), dict(order=[0], skip=1)):
        kw = dict(threshold_q32=HALF)
        kw.update(bad)
        with pytest.raises(ValueError):
            cl.leader(r, **kw)
    with pytest.raises(ValueError):
        cl.leader({k: v for k, v in r.items() if k != 'bits'}, HALF)


def test_shift_members_representatives_and_the_csv_text(tmp_path):
    c = cl.leader(hand_result(), HALF, max_clusters=3)
    assert c['cluster'].tolist() == [0, 1, 0, 2, -1] and c['unassigned'] == 1
    assert cl.members(c, 0).tolist() == [0, 2] and cl.members(c, 2).tolist() == [3] and cl.members(c, 0).dtype == np.int64
    with pytest.raises(ValueError):
        cl.members(c, 3)
    rep, n = cl.representatives(c)
    assert rep.tolist() == [0, 1, 3] and n.tolist() == [2, 1, 1]
    s = cl.shift(c, 100)
    assert s['pose'].tolist() == [100, 101, 102, 103, 104] and s['leader'].tolist() == [100, 101, 103] and s['pose'].dtype == np.int64
    assert s['cluster'] is c['cluster'] and c['pose'].tolist() == [0, 1, 2, 3, 4] and cl.members(s, 0).tolist() == [100, 102]
    recs = cl.to_records(s)
    assert recs[2] == {'type': 'pose-cluster', 'position': 2, 'pose': 102, 'cluster': 0, 'leader': 100, 'similarity': ((2 << 32) // 3) / ONE, 'size': 2}
    assert recs[4] == {'type': 'pose-cluster', 'position': 4, 'pose': 104, 'cluster': -1, 'leader': None, 'similarity': None, 'size': 0}
    path = cl.write_pose_clusters(str(tmp_path), 'x', s)
    assert os.path.basename(path) == 'x.poseclusters'
    assert open(path).read().splitlines() == ['position,pose,cluster,leader,similarity,size', '0,100,0,100,1.0,2', '1,101,1,101,1.0,1',
                                              '2,102,0,100,%r,2' % (((2 << 32) // 3) / ONE), '3,103,2,103,1.0,1', '4,104,-1,,,0']


def test_the_header_and_the_binding_name_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    for s in ('arp_poses_clusters_launch', 'arp_poses_clusters_fetch', 'arp_poses_clusters_info'):
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    assert '#define ARP_POSECL_MAX_CLUSTERS %d' % _capi.POSECL_MAX_CLUSTERS in hdr and cl.MAX_CLUSTERS == _capi.POSECL_MAX_CLUSTERS == 4096
    assert cl.MAX_POSES == _capi.POSES_MAX_POSES and cl.ONE_Q32 == sl.ONE_Q32


# ------------------------------------------------------------------------------------------------------------- GPU: seams
def _chain(K, planes, params=(5.0, 0.1, True)):
    pc, idx, x, h = chain_case(K)
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, *params)
    f = ctx.poses_fingerprints(planes, by_residue=False, n_refs=0, bits=True)
    return ctx, table, f, feature_sets(f)


@pytest.mark.gpu
def test_the_threshold_seam_by_hand():
    K = 10
    ctx, table, f, sets = _chain(K, BIT['proximal'])
    # No single SIFt bit is common to the 3.0 A and the 4.24 A records of the chain: the ladder is exclusive (3.0 A is below the
    # radii's sum, vdw_clash; 4.24 A is beyond it, proximal).  So the plane is `proximal`, which the 4.24 A records carry: pose k
    # has the features {k - 1, k + 1}, and the seam values come from those sets, by hand: q(0, 2) = q(7, 9) = 1/2 = 2^31 exactly,
    # q(k, k + 2) = 1/3 -> 1431655765 inside the chain, everything else 0.
    common = int(np.bitwise_and.reduce(table['sift'].astype(np.int64)))
    assert common == 0 and len(table['sift']) > 0
    assert sets == [{(u, 0) for u in (k - 1, k + 1) if 0 <= u < K} for k in range(K)] + [set()]
    assert q_of(sets[0], sets[2]) == HALF and q_of(sets[3], sets[5]) == THIRD and q_of(sets[4], sets[5]) == 0
    # threshold 1/3 (the floor itself): 2 joins 0 at 1/2, 3 joins 1 at exactly the threshold, 6 joins 4, 7 joins 5; 8, 9 and the
    # pose 50 A away, which has no feature and is similar to nothing, stand alone
    got, _ = check(ctx, sets, THIRD)
    assert got['cluster'].tolist() == [0, 1, 0, 1, 2, 3, 2, 3, 4, 5, 6] and got['leader'].tolist() == [0, 1, 4, 5, 8, 9, 10]
    assert got['size'].tolist() == [2, 2, 2, 2, 1, 1, 1] and got['similarity'].tolist() == [ONE, ONE, HALF, THIRD, ONE, ONE, THIRD, THIRD, ONE, ONE, ONE]
    # one above: only the end poses pair (1/2)
    got, _ = check(ctx, sets, THIRD + 1)
    assert got['cluster'].tolist() == [0, 1, 0, 2, 3, 4, 5, 6, 7, 6, 8] and got['size'].tolist() == [2, 1, 1, 1, 1, 1, 2, 1, 1]
    assert check(ctx, sets, HALF)[0]['cluster'].tolist() == [0, 1, 0, 2, 3, 4, 5, 6, 7, 6, 8]      # 2^31 itself still joins
    assert check(ctx, sets, HALF + 1)[0]['cluster'].tolist() == list(range(K + 1))                  # ... one above: nobody
    got, _ = check(ctx, sets, 0)
    assert got['size'].tolist() == [K + 1] and got['similarity'].tolist() == [ONE, 0, HALF] + [0] * (K - 2)      # one cluster
    # 1.0: every pose but an exact duplicate stands alone; the empty pose is similar to nothing but another empty pose
    order = list(range(K + 1)) + [3, K, 0]
    got, _ = check(ctx, sets, ONE, order=order)
    assert got['cluster'].tolist() == list(range(K + 1)) + [3, K, 0] and got['similarity'].tolist() == [ONE] * (K + 4)
    assert got['size'].tolist() == [2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2]
    info = ctx.poses_clusters_info()
    assert info == dict(positions=K + 4, clusters=K + 1, unassigned=0, max_clusters=256, words=1, lanes=4, launches=6, threshold_q32=ONE)
    ctx.close()


def _mask_of(n_planes):
    """A planes mask of ``n_planes`` bits that holds `proximal` and `vdw_clash` (the bits the chain's records carry)."""
    mask = BIT['proximal'] | (BIT['vdw_clash'] if n_planes > 1 else 0)
    for k in range(15):
        if bin(mask).count('1') < n_planes:
            mask |= 1 << k
    assert bin(mask).count('1') == n_planes
    return mask


# (K, planes of the mask): W = planes * ceil(K / 64) words, the lanes a pose the power of two in [4, 64] at or above min(W, 64).
# W = 270 is beyond the 256 words of the leader's row that are staged in LDS: that row comes from L2.
WORD_SEAMS = [(63, 1, 1, 4), (63, 2, 2, 4), (63, 3, 3, 4), (63, 4, 4, 4), (63, 5, 5, 8), (64, 15, 15, 16), (65, 1, 2, 4), (65, 15, 30, 32),
              (129, 1, 3, 4), (129, 15, 45, 64), (500, 8, 64, 64), (300, 13, 65, 64), (1100, 15, 270, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize('K,n_planes,W,lanes', WORD_SEAMS, ids=[f'K{k}-W{w}' for k, _, w, _ in WORD_SEAMS])
def test_word_and_lane_group_seams(K, n_planes, W, lanes):
    ctx, table, f, sets = _chain(K, _mask_of(n_planes))
    assert f['bits'].shape == (K + 1, n_planes, (K + 63) // 64) and len(f['ids']) == K
    few = 256 if K <= 129 else 8      # (the long chains: a handful of rounds, the rest unassigned — the yardstick stays quick)
    values = [v for v in set(pair_values(sets, range(min(K, 12)))) if v]
    assert values
    for thr in (min(values), max(values)):
        for order in (None, list(range(K, -1, -1))):
            got, want = check(ctx, sets, thr, order=order, max_clusters=few)
            assert len(want['leader']) >= 2 and int(want['size'].max()) >= 2
        info = ctx.poses_clusters_info()
        assert (info['words'], info['lanes'], info['positions']) == (W, lanes, K + 1)
    # a leader in the LAST word of the row, and members whose shared bits sit there alone
    tail = list(range(K - 1, max(K - 9, -1), -1))
    check(ctx, sets, min(values), order=tail)
    ctx.close()


def test_the_word_seams_meet_two_group_widths_and_a_row_beyond_the_stage():
    assert len({lanes for _, _, _, lanes in WORD_SEAMS}) >= 2 and {w for _, _, w, _ in WORD_SEAMS} >= {1, 2, 3, 4, 5, 64, 65}
    assert max(w for _, _, w, _ in WORD_SEAMS) > 256      # PCL_LDS_WORDS
    src = open(os.path.join(os.path.dirname(__file__), '..', 'arpeggio_amd', 'csrc', 'arp_poses_clusters.h')).read()
    assert '#define PCL_LDS_WORDS 256' in src


@pytest.mark.gpu
@pytest.mark.parametrize('M', [1, 2, 63, 64, 65, 130])
def test_position_seams(M):
    pc, idx, x, h = water_case(133)
    ctx = _ctx(pc, idx)
    for skip in (0, 3):
        P = M + skip
        ctx.poses_summary(x[:P], h[:P], 5.0, 0.1, False)
        f = ctx.poses_fingerprints(ALL15, n_refs=skip, bits=True)
        sets = feature_sets(f)
        values = pair_values(sets, range(skip, P)) or [HALF]
        for thr in sorted({quantile(values, 0.5), quantile(values, 0.75)}):
            got, want = check(ctx, sets, thr, skip=skip)
            assert len(got['pose']) == M and got['pose'].tolist() == list(range(skip, P))
            if skip:
                continue
            rng = np.random.default_rng(5)
            orders = [list(range(P)), list(range(P - 1, -1, -1)), rng.permutation(P).tolist(), rng.permutation(P)[:max(P // 2, 1)].tolist()]
            if P >= 3:
                orders.append([2, 0, 2, 1, 0])
            for order in orders:
                check(ctx, sets, thr, order=order)
    ctx.close()


@pytest.mark.gpu
def test_max_clusters():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    ctx.poses_summary(x, h, 5.0, 0.1, False)
    sets = feature_sets(ctx.poses_fingerprints(ALL15, n_refs=0, bits=True))
    pos = list(range(70))
    thr, free = telling_threshold(sets, pos)
    C0 = len(free['leader'])
    assert 2 <= C0 <= 69
    for mc in (1, C0 - 1, C0, C0 + 1, 4096):
        got, want = check(ctx, sets, thr, max_clusters=mc)
        assert len(got['leader']) == min(mc, C0) and (got['unassigned'] > 0) == (mc < C0)
        away = got['cluster'] < 0
        assert int(away.sum()) == got['unassigned'] and (got['similarity'][away] == -1).all() and (got['similarity'][~away] >= thr).all()
        assert int(got['size'].sum()) + got['unassigned'] == 70
        info = ctx.poses_clusters_info()
        assert (info['clusters'], info['unassigned'], info['max_clusters']) == (min(mc, C0), got['unassigned'], mc)
    ctx.close()


@pytest.mark.gpu
def test_empty_fingerprints():
    pc, idx, x, h = hem_case()
    x, h = x[:7].copy(), h[:7]
    ctx = _ctx(pc, idx)
    # every pose away: no column, no word, no bit matrix — one cluster of all
    ctx.poses_summary(x + np.float32(100.0), h, 5.0, 0.1, False)
    for by_residue in (True, False):
        f = ctx.poses_fingerprints(ALL15, by_residue=by_residue, n_refs=0, bits=True)
        assert f['bits'].shape == (7, 15, 0) and not f['count'].any()
        for thr in (0, HALF, ONE):
            got, _ = check(ctx, feature_sets(f), thr)
            assert got['cluster'].tolist() == [0] * 7 and got['similarity'].tolist() == [ONE] * 7 and got['size'].tolist() == [7] and got['leader'].tolist() == [0]
        assert differences(ctx.poses_clusters(ONE, order=[6, 6, 1]), walk(feature_sets(f), ONE, [6, 6, 1])) == []
        assert ctx.poses_clusters_info()['words'] == 0 and ctx.poses_clusters_info()['lanes'] == 4
    # one empty pose in the middle of full ones: similar to nothing; a second one joins it at 0 / 0 = 1.0
    x[3] += np.float32(100.0)
    x[5] += np.float32(100.0)
    ctx.poses_summary(x, h, 5.0, 0.1, False)
    f = ctx.poses_fingerprints(ALL15, n_refs=0, bits=True)
    sets = feature_sets(f)
    assert not sets[3] and not sets[5] and all(sets[p] for p in (0, 1, 2, 4, 6))
    for thr in (1, HALF, ONE):
        for order in (None, [0, 1, 2, 3, 4, 6]):
            got, _ = check(ctx, sets, thr, order=order)
            c3 = int(got['cluster'][3])
            assert got['leader'][c3] == 3 and got['size'][c3] == (2 if order is None else 1)
            if order is None:
                assert got['cluster'][5] == c3 and got['similarity'][5] == ONE
    got, _ = check(ctx, sets, 0)
    assert got['size'].tolist() == [7]                                       # 0 similar to everything, an empty pose included
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: contents
def _summary_rank(summary, skip=0):
    """Descending records per pose (slot 15), ties by ascending pose id."""
    score = np.asarray(summary)[:, 15].astype(np.int64)
    return (skip + np.argsort(-score[skip:], kind='stable')).tolist()


def _tanimoto_rank(sets, ref, skip=0):
    score = np.array([q_of(sets[p], sets[ref]) for p in range(len(sets))], np.int64)
    return (skip + np.argsort(-score[skip:], kind='stable')).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize('params', PARAMS, ids=[f'{c}-{v}-{int(s)}' for c, v, s in PARAMS])
def test_contents_on_the_haem(params):
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    summary = ctx.poses_summary(x, h, *params)
    widths = set()
    for level in ('residue', 'atom'):
        for planes in (ALL15, BIT['hydrophobic'], SCATTERED):
            sets = feature_sets(ctx.poses_fingerprints(planes, by_residue=level == 'residue', n_refs=0, bits=True))
            for pos in (_summary_rank(summary), _tanimoto_rank(sets, 0)):
                # the median of the yardstick's pair values, or the first later quantile of telling_threshold's list at which
                # the yardstick can tell 'first similar' from 'last' and 'most similar' (asserted inside)
                thr, want = telling_threshold(sets, pos)
                got = ctx.poses_clusters(thr, order=pos, max_clusters=4096)
                assert differences(got, want) == [], (level, planes)
                widths.add(ctx.poses_clusters_info()['lanes'])
            if level == 'residue' and planes == ALL15:      # ... and once from the upper quartile on
                thr, want = telling_threshold(sets, pos, (0.75, 0.875, 0.625, 0.5))
                assert differences(ctx.poses_clusters(thr, order=pos, max_clusters=4096), want) == []
    assert len(widths) >= 2
    ctx.close()


@pytest.mark.gpu
def test_contents_with_class_planes():
    from test_pose_shortlist import _ring_ctx
    ctx, pc, idx, x, h = _ring_ctx()
    summary = ctx.poses_summary(x, h, 5.0, 0.1, False)
    ctx.poses_planes_summary(x)
    mask = fp.planes(classes='all')
    n_sift = bin(mask & ALL15).count('1')
    f = ctx.poses_fingerprints(mask, n_refs=0, bits=True)
    assert f['bits'].shape[1] == bin(mask).count('1') > n_sift
    sets = feature_sets(f)
    assert any(k >= n_sift for s in sets for _, k in s)                      # a class plane has features (the SIFt planes stand in front)
    for pos in (_summary_rank(summary), _tanimoto_rank(sets, 0)):
        thr, want = telling_threshold(sets, pos)
        assert differences(ctx.poses_clusters(thr, order=pos, max_clusters=4096), want) == []
    ctx.close()


@pytest.mark.gpu
def test_against_the_all_pairs_matrix():
    pc, idx, x, h = water_case(133)
    ctx = _ctx(pc, idx)
    ctx.poses_summary(x[:65], h[:65], 5.0, 0.1, False)
    for level in ('residue', 'atom'):
        f = ctx.poses_fingerprints(ALL15, by_residue=level == 'residue', n_refs=0, all_pairs=True, bits=True)
        inter, count = f['inter'].astype(np.int64).tolist(), f['count'].astype(np.int64).tolist()

        def q(a, b):
            t = inter[a][b]
            u = count[a] + count[b] - t
            return ONE if u == 0 else (t << 32) // u
        sets = feature_sets(f)
        values = pair_values(sets, range(65))
        for thr in sorted({quantile(values, 0.5), quantile(values, 0.75), quantile(values, 0.9)}):
            by_inter = walk(None, thr, list(range(65)), 4096, q=q)
            assert differences(by_inter, walk(sets, thr, list(range(65)), 4096)) == []
            assert differences(ctx.poses_clusters(thr, max_clusters=4096), by_inter) == [], (level, thr)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
def _launch(ctx, thr=HALF, order=None, skip=0, max_clusters=256, n_order=None):
    info = np.zeros(8, np.int64)
    ids = None if order is None else np.ascontiguousarray(order, np.int32)
    rc = ctx._L.arp_poses_clusters_launch(ctx._h, _p(ids), (0 if ids is None else len(ids)) if n_order is None else n_order, skip, thr, max_clusters, _p(info))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), info


def _resident(ctx):
    """The resident clusters, fetched without a launch: (rc, message, arrays)."""
    info = ctx.poses_clusters_info()
    M, Cn = info['positions'], info['clusters']
    out = dict(pose=np.empty(M, np.int32), cluster=np.empty(M, np.int32), similarity=np.empty(M, np.int64), leader=np.empty(Cn, np.int32),
               leader_position=np.empty(Cn, np.int32), size=np.empty(Cn, np.uint32))
    n, m = C.c_int64(-1), C.c_int64(-1)
    rc = ctx._L.arp_poses_clusters_fetch(ctx._h, M, Cn, *[_p(out[k]) for k in ARRAYS], C.byref(n), C.byref(m))
    return rc, ctx._L.arp_last_error(ctx._h).decode(), out


def _same_resident(a, b):
    return a[0] == b[0] and _same_bytes(a[2], b[2])


NO_RESULT = dict(positions=0, clusters=0, unassigned=0, max_clusters=0, words=0, lanes=0, threshold_q32=0)


@pytest.mark.gpu
def test_every_refusal_names_its_cause_and_touches_nothing():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)

    def refused(word, code=_capi.ARP_E_ARG, **kw):
        rc, msg, _ = _launch(ctx, **kw)
        assert rc == code and word in msg, (word, rc, msg)
    refused('no poses result')
    ctx.poses_summary(x[:9], h[:9], 5.0, 0.1, False)
    refused('no fingerprint result')
    ctx.poses_fingerprints(ALL15, n_refs=2)
    good = ctx.poses_clusters(HALF, skip=2)
    launches = ctx.poses_clusters_info()['launches']
    before = _resident(ctx)
    assert before[0] == _capi.ARP_OK and _same_bytes(before[2], {k: good[k] for k in ARRAYS}) and launches == 1
    refused('threshold_q32 must be', thr=ONE + 1)
    refused('threshold_q32 must be', thr=(1 << 64) - 1)
    refused('max_clusters must be', max_clusters=0)
    refused('max_clusters must be', max_clusters=4097)
    refused('skip must be in', skip=-1)
    refused('skip must be in', skip=9)
    refused('an order takes skip = 0', order=[0, 1], skip=1)
    refused('n_order must be 1', order=[0], n_order=0)
    refused('n_order must be 1', order=[0], n_order=(1 << 20) + 1)
    refused('order has an id outside', order=[0, 9])
    refused('order has an id outside', order=[-1])
    refused('n_order must be 0 without an order', n_order=3)
    ctx.run_enqueue(5.0, 0.1, False)
    refused('not been waited for')
    ctx.run_wait()
    assert ctx._L.arp_poses_clusters_launch(None, None, 0, 0, HALF, 256, _p(np.zeros(8, np.int64))) == _capi.ARP_E_ARG
    assert ctx._L.arp_poses_clusters_launch(ctx._h, None, 0, 0, HALF, 256, None) == _capi.ARP_E_ARG
    # none of them touched the resident clusters
    assert ctx.poses_clusters_info()['launches'] == launches and _same_resident(_resident(ctx), before)
    with pytest.raises(ValueError, match='max_clusters must be'):
        ctx.poses_clusters(HALF, max_clusters=0)
    ctx.close()


@pytest.mark.gpu
def test_the_clusters_go_with_the_poses_result_and_not_with_the_fingerprint():
    from test_pose_shortlist import _ring_ctx
    ctx, pc, idx, x, h = _ring_ctx()
    m = _mask(pc, idx)
    params = (5.0, 0.1, False)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and 'no result' in _resident(ctx)[1]
    assert ctx.poses_clusters_info() == dict(NO_RESULT, launches=0)
    ctx.poses_contacts(x[:9], h[:9], *params)
    sets = feature_sets(ctx.poses_fingerprints(ALL15, n_refs=2, bits=True))
    first, _ = check(ctx, sets, HALF, skip=2)
    # every successful launch remakes the result
    second, _ = check(ctx, sets, THIRD, order=[8, 1, 8])
    assert ctx.poses_clusters_info()['launches'] == 2 and len(second['pose']) == 3
    assert _same_bytes(ctx.poses_clusters(HALF, skip=2), first)
    # a fingerprint launch with other arguments does NOT void the clusters (they read it only while their launch ran) ...
    before = _resident(ctx)
    launches = ctx.poses_fingerprints_info()['launches']
    ctx.poses_fingerprints(SCATTERED, by_residue=False, n_refs=0)
    assert ctx.poses_fingerprints_info()['launches'] == launches + 1 and _same_resident(_resident(ctx), before) and before[0] == _capi.ARP_OK
    # ... and clusters made from a fingerprint WITHOUT class planes are untouched by the planes entries
    ctx.poses_planes(x[:9])
    ctx.set_plane_atoms(pc)
    assert _same_resident(_resident(ctx), before)
    # made from class planes, they go with the poses-planes result
    ctx.poses_planes(x[:9])
    for void in (lambda: ctx.poses_planes(x[:9]), lambda: ctx.set_plane_atoms(pc)):
        sets = feature_sets(ctx.poses_fingerprints(fp.planes(classes='all'), n_refs=0, bits=True))
        check(ctx, sets, HALF)
        assert _resident(ctx)[0] == _capi.ARP_OK
        void()
        rc, msg, _ = _resident(ctx)
        assert rc == _capi.ARP_E_ARG and 'no result' in msg and ctx.poses_clusters_info()['positions'] == 0
        ctx.poses_planes(x[:9])
    # a new poses result, a new selection, a new structure, models
    launches = ctx.poses_clusters_info()['launches']
    ctx.poses_fingerprints(ALL15, n_refs=2)
    ctx.poses_clusters(HALF, skip=2)
    ctx.poses_contacts(x[:9], h[:9], *params)                          # the same poses again: still a new result
    assert _resident(ctx)[0] == _capi.ARP_E_ARG and ctx.poses_clusters_info() == dict(NO_RESULT, launches=launches + 1)
    ctx.poses_fingerprints(ALL15, n_refs=2)
    assert _same_bytes(ctx.poses_clusters(HALF, skip=2), first)
    ctx.set_selection(m)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.poses_contacts(x[:9], h[:9], *params)
    ctx.poses_fingerprints(ALL15, n_refs=2)
    ctx.poses_clusters(HALF, skip=2)
    assert _resident(ctx)[0] == _capi.ARP_OK
    ctx.set_complex(pc)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.set_selection(m)
    ctx.poses_contacts(x[:9], h[:9], *params)
    ctx.poses_fingerprints(ALL15, n_refs=2)
    ctx.poses_clusters(HALF, skip=2)
    ctx.set_topology(pc)
    X, H = poses.as_models(pc, idx, x[:2], h[:2])
    ctx.set_models(X, H)
    assert _resident(ctx)[0] == _capi.ARP_E_ARG
    ctx.close()


@pytest.mark.gpu
def test_a_launch_reads_no_bag_and_voids_nothing():
    from test_pose_fingerprints import _fetch_everything
    from test_pose_shortlist import _resident as _resident_shortlist, _ring_ctx
    ctx, pc, idx, x, h = _ring_ctx()
    counts = ctx.run_launch(5.0, 0.1, False)
    assert counts['atom_atom'] > 0 and len(ctx.residue_pairs()['res_a']) > 0
    label, net = ctx.networks(ALL15, 0x7F, True)
    ctx.poses_planes(x[:9])
    ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    f = ctx.poses_fingerprints(fp.planes(classes='all'), n_refs=2, bits=True)
    ctx.poses_shortlist('tanimoto', ref=-1, skip=2, k=4, tables=sl.TABLES)
    before, short = _fetch_everything(ctx), _resident_shortlist(ctx, planes=True)
    assert short[0] == _capi.ARP_OK
    sets = feature_sets(f)
    for kw in (dict(thr=HALF, skip=2), dict(thr=THIRD, order=[3, 3, 0]), dict(thr=ONE, max_clusters=2)):
        got, _ = check(ctx, sets, kw.pop('thr'), **kw)
        assert _same_bytes(_fetch_everything(ctx), before)
        assert _same_bytes(ctx.poses_fingerprints(fp.planes(classes='all'), n_refs=2, bits=True), f) and ctx.poses_fingerprints_info()['launches'] == 1
        again = _resident_shortlist(ctx, planes=True)
        assert again[0] == _capi.ARP_OK and _same_bytes(again[2], short[2])
        again = ctx.networks(ALL15, 0x7F, True)
        assert _same_bytes(again[0], label) and _same_bytes(again[1], net)
    st = ctx.stats()
    assert (st['posecl_positions'], st['posecl_clusters'], st['posecl_launches']) == (9, len(got['leader']), 3) and got['unassigned'] > 0
    ctx.close()


@pytest.mark.gpu
def test_null_pointers_capacity_and_a_caller_owned_stream():
    from test_gpu_paths import _hip_runtime
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    ctx.poses_summary(x[:9], h[:9], 5.0, 0.1, False)
    sets = feature_sets(ctx.poses_fingerprints(ALL15, n_refs=0, bits=True))
    values = pair_values(sets, range(9))      # (the first quantile at which the yardstick makes some, but not nine, clusters)
    thr = next(quantile(values, f) for f in (0.5, 0.75, 0.25, 0.9) if 2 <= len(walk(sets, quantile(values, f), list(range(9)))['leader']) < 9)
    want, _ = check(ctx, sets, thr)
    M, Cn = 9, len(want['leader'])
    L, hd = ctx._L, ctx._h
    n, m = C.c_int64(0), C.c_int64(0)
    none = [None] * 6
    assert L.arp_poses_clusters_fetch(hd, 0, 0, *none, C.byref(n), C.byref(m)) == _capi.ARP_OK and (n.value, m.value) == (M, Cn)
    assert L.arp_poses_clusters_fetch(hd, 0, 0, *none, None, C.byref(m)) == _capi.ARP_E_ARG
    assert L.arp_poses_clusters_fetch(hd, 0, 0, *none, C.byref(n), None) == _capi.ARP_E_ARG
    for slot, key in enumerate(ARRAYS):
        buf = np.full(want[key].shape, 7, want[key].dtype)
        args = list(none)
        args[slot] = _p(buf)
        n.value = m.value = 0
        short = (M - 1, Cn) if slot < 3 else (M, Cn - 1)
        assert L.arp_poses_clusters_fetch(hd, *short, *args, C.byref(n), C.byref(m)) == _capi.ARP_E_CAPACITY, key
        assert (n.value, m.value) == (M, Cn) and (buf == 7).all() and 'too small' in L.arp_last_error(hd).decode()
        other = (M, 0) if slot < 3 else (0, Cn)                       # (the capacity of the arrays not asked for is not looked at)
        assert L.arp_poses_clusters_fetch(hd, *other, *args, C.byref(n), C.byref(m)) == _capi.ARP_OK and _same_bytes(buf, want[key]), key
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    ctx.poses_summary(x[:9], h[:9], 5.0, 0.1, False)
    ctx.poses_fingerprints(ALL15, n_refs=0)
    got = ctx.poses_clusters(thr)
    assert _same_bytes(got, {k: want[k] for k in got})
    ctx.use_stream(0)                                                 # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------------------------------------------------- GPU: end to end
@pytest.mark.gpu
def test_run_pose_clusters_end_to_end(tmp_path):
    pc, idx, x, h = hem_case()
    params = (5.0, 0.1, False)
    ic = InteractionComplex(copy.copy(pc))
    # the yardstick: the home pose in front of the poses, as the default reference
    atoms, rows = poses.movable(pc, idx)
    both_x, both_h = np.concatenate([pc.xyz[atoms][None].astype(np.float32), x]), np.concatenate([pc.h_xyz[rows][None], h])
    ic.initialize()
    ctx = ic._ctx
    ctx.set_selection(_mask(pc, idx))
    summary = ctx.poses_summary(both_x, both_h, *params)
    sets = feature_sets(ctx.poses_fingerprints(fp.planes(), n_refs=1, bits=True))
    ranks = dict(summary=_summary_rank(summary, 1), tanimoto=_tanimoto_rank(sets, 0, 1), input=list(range(1, 71)))
    results = {}
    for by, pos in ranks.items():
        want = walk(sets, HALF, pos, 256)
        want['pose'], want['leader'] = want['pose'].astype(np.int64) - 1, want['leader'].astype(np.int64) - 1
        got = ic.run_pose_clusters(['RESNAME:HEM'], x, h, *params, threshold=0.5, by=by)
        assert differences(got, want) == [], by
        assert (got['by'], got['n_refs'], got['level']) == (by, 1, 'residue') and ic.pose_clusters is got and 'records' not in got
        results[by] = got
    assert len(results['summary']['leader']) >= 2
    # pose 0 of synth.poses_of is the home pose: by Tanimoto to the default reference it ranks first and leads cluster 0
    assert results['tanimoto']['pose'][0] == 0 and results['tanimoto']['leader'][0] == 0 and results['input']['pose'].tolist() == list(range(70))
    # two references of the caller's, atom level, named contacts, few clusters, the leaders' records
    got = ic.run_pose_clusters(np.asarray(idx), x[2:], h[2:], *params, threshold=0.25, by='tanimoto', refs_xyz=x[:2], refs_h_xyz=h[:2],
                               contacts=['hbond', 'hydrophobic'], level='atom', max_clusters=3, records=True)
    ctx.poses_summary(x, h, *params)
    sets = feature_sets(ctx.poses_fingerprints(BIT['hbond'] | BIT['hydrophobic'], by_residue=False, n_refs=2, bits=True))
    best = np.array([max(q_of(sets[p], sets[0]), q_of(sets[p], sets[1])) for p in range(70)], np.int64)
    want = walk(sets, 1 << 30, (2 + np.argsort(-best[2:], kind='stable')).tolist(), 3)
    want['pose'], want['leader'] = want['pose'].astype(np.int64) - 2, want['leader'].astype(np.int64) - 2
    assert differences(got, want) == [] and got['n_refs'] == 2 and 1 <= len(got['leader']) <= 3
    full = copy.copy(ic.run_poses(['RESNAME:HEM'], x[2:], h[2:], *params))
    part = sl.take(full, got['leader'])
    rec = got['records']
    assert np.array_equal(rec['pose'], got['leader']) and rec['pose'].dtype == np.int64
    for k in poses.COLUMNS + ('pose_off', 'summary'):
        assert _same_bytes(rec[k], part[k]), k
    assert len(rec['i']) > 0
    for bad in (dict(by='distance'), dict(level='chain'), dict(threshold=1.5), dict(max_clusters=0), dict(classes='all', level='atom')):
        with pytest.raises(ValueError):
            ic.run_pose_clusters(['RESNAME:HEM'], x, h, *params, **bad)
    # the CSV
    ic.pose_clusters = results['tanimoto']
    path = ic.write_pose_clusters(str(tmp_path))
    lines = open(path).read().splitlines()
    r = results['tanimoto']
    assert os.path.basename(path) == ic.id + '.poseclusters' and len(lines) == 71 and lines[0] == 'position,pose,cluster,leader,similarity,size'
    assert lines[1] == '0,0,0,0,1.0,%d' % r['size'][0]
    c1 = int(r['cluster'][1])
    assert lines[2] == '1,%d,%d,%d,%r,%d' % (r['pose'][1], c1, r['leader'][c1], int(r['similarity'][1]) / ONE, r['size'][c1])
