"""Host side of the pose clusters (``Context.poses_clusters`` / ``InteractionComplex.run_pose_clusters``): leader clustering of
the poses of a launch by the Tanimoto similarity of their interaction fingerprints (csrc/arp_poses_clusters.h).

A ``clusters`` dict:

    pose             int32 [M]    the pose of each position (the positions are the caller's rank order)
    cluster          int32 [M]    the cluster of each position, an index in leader order; -1 when unassigned
    similarity       int64 [M]    the similarity to its own leader's pose in 32 fractional bits; 2^32 for a leader; -1 when unassigned
    leader           int32 [C]    the leaders' poses
    leader_position  int32 [C]    the leaders' positions, strictly ascending
    size             uint32 [C]   members per cluster, the leader included
    threshold_q32, max_clusters, unassigned

The method is sphere exclusion in rank order: walk the positions; a pose similar to an earlier leader joins the FIRST such
leader, otherwise it becomes a leader (while fewer than ``max_clusters`` exist; it stays unassigned after that).  ``leader`` is
the host route over a fingerprint result fetched with ``bits=True`` — what the device result must equal.  Everything here is
NumPy and Python integers: no GPU, no native library.
"""
import csv
import fractions
import os

import numpy as np

ONE_Q32 = 1 << 32            # the similarity 1.0
MAX_CLUSTERS = 4096          # ARP_POSECL_MAX_CLUSTERS
MAX_POSES = 1 << 20          # ARP_POSES_MAX_POSES
PER_POSITION = ('pose', 'cluster', 'similarity')
PER_CLUSTER = ('leader', 'leader_position', 'size')
DTYPES = dict(pose=np.int32, cluster=np.int32, similarity=np.int64, leader=np.int32, leader_position=np.int32, size=np.uint32)


def threshold_q32(t):
    """The smallest integer q with q / 2^32 >= t, for a float ``t`` in [0, 1]: poses are similar when their Tanimoto similarity is
    at least ``t``.  Exact (through ``fractions.Fraction``: a float is a fraction); anything else raises ``ValueError``."""
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)):
        raise ValueError('threshold_q32: a number in [0, 1]')
    t = float(t)
    if not 0.0 <= t <= 1.0:      # (a NaN fails both comparisons)
        raise ValueError('threshold_q32: a number in [0, 1]')
    scaled = fractions.Fraction(t) * ONE_Q32
    return -((-scaled.numerator) // scaled.denominator)


def _popcount(words):
    return sum(bin(int(w)).count('1') for w in np.asarray(words, np.uint64).reshape(-1).tolist())


_BYTE_BITS = np.array([bin(v).count('1') for v in range(256)], np.uint8)


def _row_popcount(words):
    """uint64 [n, W] -> the set bits of every row, uint64 [n]."""
    w = np.ascontiguousarray(words, np.uint64)
    return _BYTE_BITS[w.view(np.uint8).reshape(w.shape[0], w.shape[1] * 8)].sum(axis=1, dtype=np.uint64)


def pair_q32(bits_a, bits_b, count_a, count_b):
    """The similarity of two poses as the device computes it, a Python integer: t = the bits both rows have, u = count_a +
    count_b - t, floor(t 2^32 / u), and 2^32 where u = 0 (0 / 0 is 1.0)."""
    a, b = np.asarray(bits_a, np.uint64).reshape(-1), np.asarray(bits_b, np.uint64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError('pair_q32: the rows differ in length')
    t = _popcount(a & b)
    u = int(count_a) + int(count_b) - t
    return ONE_Q32 if u == 0 else (t << 32) // u


def positions(n_poses, order=None, skip=0):
    """The pose of every position (int32 [M]) as ``Context.poses_clusters`` reads its arguments; ``ValueError`` where it refuses."""
    P = int(n_poses)
    if order is None:
        if not 0 <= int(skip) < P:
            raise ValueError('positions: skip must be in [0, P)')
        return np.arange(int(skip), P, dtype=np.int32)
    ids = np.asarray(order, np.int64).reshape(-1)
    if int(skip) != 0:
        raise ValueError('positions: an order takes skip = 0')
    if not 1 <= len(ids) <= MAX_POSES:
        raise ValueError('positions: 1 ... 2^20 positions')
    if ids.min() < 0 or ids.max() >= P:
        raise ValueError('positions: order has an id outside [0, P)')
    return ids.astype(np.int32)


def leader(result, threshold_q32, order=None, skip=0, max_clusters=256):
    """The host route: the clusters of a fingerprint result fetched with ``bits=True`` (``Context.poses_fingerprints``), the same
    dict with the same dtypes as ``Context.poses_clusters`` returns."""
    thr, mc = int(threshold_q32), int(max_clusters)
    if not 0 <= thr <= ONE_Q32:
        raise ValueError('leader: threshold_q32 must be 0 ... 2^32')
    if not 1 <= mc <= MAX_CLUSTERS:
        raise ValueError(f'leader: max_clusters must be 1 ... {MAX_CLUSTERS}')
    if 'bits' not in result:
        raise ValueError('leader: the fingerprint result has no bits (fetch it with bits=True)')
    count = np.asarray(result['count']).reshape(-1).astype(np.int64)
    P = len(count)
    rows = np.ascontiguousarray(result['bits'], np.uint64)
    rows = rows.reshape(P, rows.size // max(P, 1))      # (no feature at all: no word)
    pose = positions(P, order, skip)
    M = len(pose)
    cluster, similarity = np.full(M, -1, np.int32), np.full(M, -1, np.int64)
    lead, lead_pos, size = [], [], []
    # round by round, as the device does it: the first position left leads, every later one left that is similar to it joins —
    # a position reaches round c only when it was similar to none of the leaders before, so it joins the first similar one
    left = np.arange(M, dtype=np.int64)
    while len(left) and len(lead) < mc:
        m0, rest = int(left[0]), left[1:]
        lp, c = int(pose[m0]), len(lead)
        t = _row_popcount(rows[pose[rest]] & rows[lp][None, :])
        u = (count[pose[rest]] + count[lp]).astype(np.uint64) - t      # (t <= both counts: no wrap; t < 2^32: t << 32 fits 64 bits)
        q = np.where(u == 0, np.uint64(ONE_Q32), (t << np.uint64(32)) // np.maximum(u, np.uint64(1)))
        similar = q >= np.uint64(thr)
        cluster[m0], similarity[m0] = c, ONE_Q32
        cluster[rest[similar]], similarity[rest[similar]] = c, q[similar].astype(np.int64)
        lead.append(lp)
        lead_pos.append(m0)
        size.append(1 + int(similar.sum()))
        left = rest[~similar]
    return dict(pose=pose, cluster=cluster, similarity=similarity, leader=np.asarray(lead, np.int32), leader_position=np.asarray(lead_pos, np.int32),
                size=np.asarray(size, np.uint32), threshold_q32=thr, max_clusters=mc, unassigned=int((cluster < 0).sum()))


def members(clusters, c):
    """The poses of cluster ``c`` in position order, the leader first (int64)."""
    if not 0 <= int(c) < len(clusters['leader']):
        raise ValueError(f'members: no cluster {c}')
    return np.asarray(clusters['pose']).astype(np.int64)[np.asarray(clusters['cluster']) == int(c)]


def representatives(clusters):
    """One pose per cluster — its leader, the best-ranked member — with the members behind it: (pose int64 [C], size int64 [C])."""
    return np.asarray(clusters['leader']).astype(np.int64), np.asarray(clusters['size']).astype(np.int64)


def shift(clusters, by):
    """The clusters with ``by`` added to every pose id (``pose`` and ``leader``, int64): a launch's ids in the caller's numbering."""
    out = dict(clusters)
    out['pose'] = np.asarray(clusters['pose']).astype(np.int64) + int(by)
    out['leader'] = np.asarray(clusters['leader']).astype(np.int64) + int(by)
    return out


def _rows(clusters):
    lead, size = np.asarray(clusters['leader']).tolist(), np.asarray(clusters['size']).tolist()
    for m, (p, c, q) in enumerate(zip(np.asarray(clusters['pose']).tolist(), np.asarray(clusters['cluster']).tolist(),
                                      np.asarray(clusters['similarity']).tolist())):
        if c < 0:
            yield m, int(p), -1, None, None, 0
        else:
            yield m, int(p), int(c), int(lead[c]), int(q) / ONE_Q32, int(size[c])


def to_records(clusters):
    """For JSON: one dict per position ('type': 'pose-cluster'): position, pose, cluster, the leader's pose, the similarity to it
    as a float and the cluster's size (cluster -1, leader and similarity ``None``, size 0 when unassigned); plain ints and floats."""
    return [{'type': 'pose-cluster', 'position': m, 'pose': p, 'cluster': c, 'leader': lp, 'similarity': q, 'size': n}
            for m, p, c, lp, q, n in _rows(clusters)]


CSV_HEADER = ['position', 'pose', 'cluster', 'leader', 'similarity', 'size']


def write_csv(path, clusters):
    """One row per position: position, pose, cluster, the leader's pose, the similarity q / 2^32 (the shortest text that gives
    the float64 back) and the cluster's size; an unassigned position has cluster -1, empty leader and similarity, size 0."""
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for m, p, c, lp, q, n in _rows(clusters):
            w.writerow([m, p, c, '' if lp is None else lp, '' if q is None else repr(q), n])


def write_pose_clusters(wd, sid, clusters):
    """'<id>.poseclusters' in ``wd``."""
    path = os.path.join(wd, sid + '.poseclusters')
    write_csv(path, clusters)
    return path
