"""Host side of the library clusters (``Context.library_clusters`` / ``InteractionComplex.run_library_clusters``): leader clustering
of poses of a ligand library by the Tanimoto similarity of their library fingerprints (csrc/arp_library_clusters.h).

A ``clusters`` dict is what ``pose_clusters`` describes, with the ligand beside the pose:

    pose             int32 [M]    the GLOBAL pose of each position (the positions are the caller's rank order)
    ligand           int32 [M]    the ligand of that pose
    cluster          int32 [M]    the cluster of each position, an index in leader order; -1 when unassigned
    similarity       int64 [M]    the similarity to its own leader's pose in 32 fractional bits; 2^32 for a leader; -1 when unassigned
    leader           int32 [C]    the leaders' global poses
    leader_position  int32 [C]    the leaders' positions, strictly ascending
    size             uint32 [C]   members per cluster, the leader included
    threshold_q32, max_clusters, unassigned

A library fingerprint has Q + T rows, the Q references first: global pose t is ROW Q + t, and a reference is never a position.
``leader`` is the host route over a library fingerprint fetched with ``bits=True`` — what the device result must equal.
Everything here is NumPy and Python integers: no GPU, no native library.
"""
import csv
import os

import numpy as np

from . import pose_clusters as _pcl
from .pose_clusters import MAX_CLUSTERS, MAX_POSES, ONE_Q32, members, pair_q32, representatives, shift, threshold_q32      # noqa: F401

WINDOW = 32                  # ARP_LIBCL_WINDOW: the positions a round of the device route resolves together
LDS_WORDS = 2048             # ARP_LIBCL_LDS_WORDS: 32 rows are staged in LDS when 32 W <= this
SOURCES = ('all', 'list', 'shortlist')      # ARP_LIBCL_ALL, ARP_LIBCL_LIST, ARP_LIBCL_SHORTLIST
PER_POSITION = ('pose', 'ligand', 'cluster', 'similarity')
PER_CLUSTER = _pcl.PER_CLUSTER
DTYPES = dict(_pcl.DTYPES, ligand=np.int32)


def ligands_of(ligand_pose_off):
    """The ligand of every global pose (int32 [T]) from ``ligand_pose_off`` [L + 1]; a ligand without poses owns none."""
    off = np.asarray(ligand_pose_off, np.int64).reshape(-1)
    return np.repeat(np.arange(len(off) - 1, dtype=np.int32), np.diff(off))


def leader(result, threshold_q32, order=None, ligand_of=None, max_clusters=256):
    """The host route: the clusters of a library fingerprint fetched with ``bits=True`` (``Context.library_fingerprints``), the
    same dict with the same dtypes as ``Context.library_clusters`` returns.  ``order``: global poses in [0, T) (None: all of
    them).  ``ligand_of``: the ligand of every global pose (``ligands_of``); without it the result has no ``ligand``."""
    Q = int(result['n_refs'])
    T = len(np.asarray(result['count']).reshape(-1)) - Q
    if T < 1:
        raise ValueError('leader: the fingerprint has no pose rows')
    if order is None:
        rows = np.arange(Q, Q + T, dtype=np.int64)
    else:
        ids = np.asarray(order, np.int64).reshape(-1)
        if not 1 <= len(ids) <= MAX_POSES:
            raise ValueError('leader: 1 ... 2^20 positions')
        if ids.min() < 0 or ids.max() >= T:
            raise ValueError('leader: order has an id outside [0, T)')
        rows = ids + Q
    out = _pcl.leader(result, threshold_q32, order=rows, max_clusters=max_clusters)
    out['pose'] = (out['pose'].astype(np.int64) - Q).astype(np.int32)
    out['leader'] = (out['leader'].astype(np.int64) - Q).astype(np.int32)
    if ligand_of is not None:
        lig = np.asarray(ligand_of, np.int32).reshape(-1)
        if len(lig) != T:
            raise ValueError('leader: ligand_of must name the ligand of each of the T poses')
        out['ligand'] = lig[out['pose']]
    return out


def leader_ligands(clusters):
    """The ligand of every cluster's leader (int32 [C])."""
    return np.asarray(clusters['ligand'], np.int32)[np.asarray(clusters['leader_position'], np.int64)]


def _rows(clusters):
    lead, size = np.asarray(clusters['leader']).tolist(), np.asarray(clusters['size']).tolist()
    lead_lig = leader_ligands(clusters).tolist()
    for m, (p, l, c, q) in enumerate(zip(np.asarray(clusters['pose']).tolist(), np.asarray(clusters['ligand']).tolist(),
                                         np.asarray(clusters['cluster']).tolist(), np.asarray(clusters['similarity']).tolist())):
        if c < 0:
            yield m, int(p), int(l), -1, None, None, None, 0
        else:
            yield m, int(p), int(l), int(c), int(lead[c]), int(lead_lig[c]), int(q) / ONE_Q32, int(size[c])


def to_records(clusters):
    """For JSON: one dict per position ('type': 'library-cluster'): position, pose, ligand, cluster, the leader's pose and ligand,
    the similarity to it as a float and the cluster's size (cluster -1, leader, leader_ligand and similarity ``None``, size 0
    when unassigned); plain ints and floats."""
    return [{'type': 'library-cluster', 'position': m, 'pose': p, 'ligand': l, 'cluster': c, 'leader': lp, 'leader_ligand': ll, 'similarity': q,
             'size': n} for m, p, l, c, lp, ll, q, n in _rows(clusters)]


CSV_HEADER = ['position', 'pose', 'ligand', 'cluster', 'leader', 'leader_ligand', 'similarity', 'size']


def write_csv(path, clusters):
    """One row per position: position, pose, ligand, cluster, the leader's pose and ligand, the similarity q / 2^32 (the shortest
    text that gives the float64 back) and the cluster's size; an unassigned position has cluster -1, empty leader, leader_ligand
    and similarity, size 0."""
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for m, p, l, c, lp, ll, q, n in _rows(clusters):
            w.writerow([m, p, l, c, '' if lp is None else lp, '' if ll is None else ll, '' if q is None else repr(q), n])


def write_library_clusters(wd, sid, clusters):
    """'<id>.libraryclusters' in ``wd``."""
    path = os.path.join(wd, sid + '.libraryclusters')
    write_csv(path, clusters)
    return path
