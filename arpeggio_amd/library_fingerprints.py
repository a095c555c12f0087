"""Host side of the library fingerprints (``Context.library_fingerprints`` / ``InteractionComplex.run_library_fingerprints``):
which molecules of a ligand library reproduce the interactions of a known binder, and each ligand's best pose for that.

The device delivers a ``result`` made from the resident library result (csrc/arp_library_fingerprints.h), shaped as
``pose_fingerprints`` describes it, over Q + T rows: the Q references first, then the global poses of the library result.  A
feature is (node, plane): a receptor residue (``level='residue'``) or receptor atom (``'atom'``) and one of the 15 SIFt bits.
The ligand atom of a record never names a node; there is no all-pairs matrix.  With a mask beyond bit 14
(``planes(classes=...)``) the ring and amide records of the resident library-planes result of the same poses enter as the 14 class
planes of ``pose_fingerprints.CLASS_PLANE_NAMES``, residue level only (``ligand_library.plane_fingerprints`` is the host route and
says how a record's node is found); reference masks may then carry those bits too (``reference_from_plane_records``).

The references need not be poses of the launch.  They are feature lists (``references``):

    ref_off     int64  [Q + 1]   reference q holds the features ref_off[q] ... ref_off[q + 1] - 1
    ref_node    int32  [F]       nodes of the launch's level, strictly ascending within a reference
    ref_planes  uint32 [F]       the planes the reference has at that node, BEFORE the launch's selection

The device ANDs every mask with the launch's ``planes``; a feature whose mask becomes 0 is dropped, and a node that keeps a plane
is a column even if no pose touches it: a reference's ``count`` is complete.

The best pose per ligand (``best``, ``Context.library_fingerprints_best``) is a dict:

    n_poses       int64  [L]
    best_pose     int32  [L, Q]   the global pose of the highest Tanimoto to reference q, ties to the lower pose; -1: no pose
    tanimoto_q32  int64  [L, Q]   that score in 32 fractional bits (``pose_shortlist.tanimoto_q32``); -1: no pose
    shared        uint32 [L, Q]   features that pose shares with the reference
    count         uint32 [L, Q]   that pose's own feature count (recovery = shared / the reference's count)

Because the first Q rows of a result are the references, ``tanimoto``, ``recovery``, ``rank``, ``strip_references``, ``merge`` and
``unpack`` of ``pose_fingerprints`` apply unchanged and are re-exported here.  Everything here is NumPy on the host.
"""
import csv
import os

import numpy as np

from .pose_fingerprints import (CLASS_PLANE_NAMES, LEVELS, MAX_REFS, N_ALL_PLANES, N_PLANES, merge, plane_names, planes, rank,      # noqa: F401
                                recovery, reference_counts, strip_references, tanimoto, unpack)

MAX_FEATURES = 1 << 22      # ARP_LIBFP_MAX_FEATURES
ONE_Q32 = 1 << 32
ALL_PLANES = (1 << N_PLANES) - 1
ALL_CLASS_PLANES = (1 << N_ALL_PLANES) - 1      # the 15 SIFt bits and the 14 ring / amide class planes
BEST_KEYS = ('best_pose', 'tanimoto_q32', 'shared', 'count')
BEST_DTYPES = dict(best_pose=np.int32, tanimoto_q32=np.int64, shared=np.uint32, count=np.uint32)


def validate(refs, n_nodes=None, classes=False):
    """What arp_library_fingerprints_launch refuses of its reference arrays, in its order and with its causes, checked on the
    host (ValueError).  ``n_nodes``: the nodes of the level (atoms, or residues) when known.  Two things the launch cannot see
    are checked here as well: a ``ref_off`` that is not one-dimensional shares the message of the Q range, and the lengths of
    ``ref_node`` / ``ref_planes`` against ``ref_off[-1]`` come between the feature limit and the node range.  ``classes``: the
    masks are those of arp_library_fingerprints_planes_launch, 29 bits (the class planes 15 ... 28 as well)."""
    off = np.asarray(refs['ref_off'])
    node, mask = np.asarray(refs['ref_node']), np.asarray(refs['ref_planes'])
    if off.ndim != 1 or not 0 <= len(off) - 1 <= MAX_REFS:
        raise ValueError('library fingerprints: 0 ... MAX_REFS references')
    off = off.astype(np.int64)
    if off[0] != 0:
        raise ValueError('library fingerprints: ref_off must start at 0')
    if (np.diff(off) < 0).any():
        raise ValueError('library fingerprints: ref_off must not decrease')
    F = int(off[-1])
    if F > MAX_FEATURES:
        raise ValueError('library fingerprints: more than MAX_FEATURES reference features')
    if node.shape != (F,) or mask.shape != (F,):
        raise ValueError('library fingerprints: ref_node and ref_planes must hold ref_off[-1] entries each')
    node, mask = node.astype(np.int64), mask.astype(np.int64)
    if (node < 0).any() or (n_nodes is not None and (node >= int(n_nodes)).any()):
        raise ValueError('library fingerprints: a reference node outside [0, nodes of the level)')
    inner = np.ones(F, bool)
    inner[off[:-1][off[:-1] < F]] = False                  # (the first feature of a reference has no predecessor in it)
    if F and (np.diff(node, prepend=node[0])[inner] <= 0).any():
        raise ValueError('library fingerprints: the nodes of a reference must be strictly ascending')
    if not classes and ((mask < 0) | (mask > ALL_PLANES)).any():
        raise ValueError('library fingerprints: a reference mask has bits beyond the 15 SIFt bits')
    if ((mask < 0) | (mask > ALL_CLASS_PLANES)).any():
        raise ValueError('library fingerprints: a reference mask has bits beyond the 29 planes')
    return refs


def references(lists, n_nodes=None, classes=False):
    """The reference arrays of ``lists``: per reference a ``(nodes, masks)`` pair of equally long integer sequences, or a dict
    ``{node: mask}`` (sorted by node here).  ``validate`` names what is refused; ``classes`` admits 29-bit masks."""
    lists = list(lists)
    if len(lists) > MAX_REFS:
        raise ValueError('library fingerprints: 0 ... MAX_REFS references')
    nodes, masks = [], []
    for item in lists:
        if isinstance(item, dict):
            keys = sorted(item)
            n, m = np.array(keys, np.int64), np.array([item[k] for k in keys], np.int64)
        else:
            n, m = np.asarray(item[0], np.int64).reshape(-1), np.asarray(item[1], np.int64).reshape(-1)
        if len(n) != len(m):
            raise ValueError('library fingerprints: a reference needs one mask per node')
        nodes.append(n)
        masks.append(m)
    off = np.concatenate([[0], np.cumsum([len(n) for n in nodes])]).astype(np.int64)
    node = np.concatenate(nodes) if nodes else np.zeros(0, np.int64)
    mask = np.concatenate(masks) if masks else np.zeros(0, np.int64)
    validate(dict(ref_off=off, ref_node=node, ref_planes=mask), n_nodes, classes)
    return dict(ref_off=off, ref_node=node.astype(np.int32), ref_planes=mask.astype(np.uint32))


def n_references(refs):
    return len(refs['ref_off']) - 1


def reference_from_records(i, sift, ctype, res_id=None, planes=ALL_PLANES, ctype_mask=0x7F, level='residue'):
    """One reference as a ``(nodes, masks)`` pair from atom-atom records whose receptor atoms are ``i``: the records whose ``ctype``
    bit is in ``ctype_mask`` and that have a plane of ``planes`` give their node (``res_id[i]`` at ``level='residue'``, else
    ``i``) the planes they have among ``planes``.  A node whose mask the selection empties is dropped."""
    if level not in LEVELS:
        raise ValueError("reference_from_records: level must be 'residue' or 'atom'")
    i, s, c = np.asarray(i, np.int64).reshape(-1), np.asarray(sift, np.int64).reshape(-1), np.asarray(ctype, np.int64).reshape(-1)
    if not len(i) == len(s) == len(c):
        raise ValueError('reference_from_records: i, sift and ctype must be equally long')
    if level == 'residue':
        if res_id is None:
            raise ValueError("reference_from_records: level='residue' needs res_id")
        node = np.asarray(res_id, np.int64)[i]
    else:
        node = i
    m = s & int(planes) & ALL_PLANES
    keep = (((int(ctype_mask) >> np.minimum(c, 31)) & 1) != 0) & (c < 7) & (m != 0)
    node, m = node[keep], m[keep]
    nodes = np.unique(node)
    masks = np.zeros(len(nodes), np.int64)
    np.bitwise_or.at(masks, np.searchsorted(nodes, node), m)
    return nodes.astype(np.int32), masks.astype(np.uint32)


def reference_from_plane_records(planes_table, receptor, t=None, planes=ALL_CLASS_PLANES, ctype_mask=0x7F):
    """One reference as a ``(nodes, masks)`` pair from the ring / amide records of a known binder: global pose ``t`` of a
    ``Context.library_planes`` table on ``receptor`` (``None``: every pose of the table joined).  The features are those of
    ``ligand_library.plane_fingerprints`` — residue nodes, class planes 15 ... 28 — that ``planes`` selects."""
    from . import ligand_library as _ll
    per = _ll.plane_fingerprints(planes_table, receptor, ctype_mask)
    if t is not None and not 0 <= int(t) < len(per):
        raise ValueError(f'reference_from_plane_records: no global pose {t}')
    feats = set().union(*per) if t is None else per[int(t)]
    masks = {}
    for node, plane in feats:
        if (int(planes) >> plane) & 1:
            masks[node] = masks.get(node, 0) | (1 << plane)
    nodes = sorted(masks)
    return np.array(nodes, np.int32), np.array([masks[u] for u in nodes], np.uint32)


def reference_from_pose(library_result, t, res_id=None, planes=None, ctype_mask=0x7F, level='residue', planes_result=None, receptor=None):
    """``reference_from_records`` over the records of global pose ``t`` of a library result (``Context.library_contacts``).
    ``planes_result``: the ``Context.library_planes`` table of the same poses on ``receptor`` (its pack, required then); the
    pose's ring / amide features (``reference_from_plane_records``) are merged in per node, residue level only.  ``planes``
    defaults to the 15 SIFt bits, with ``planes_result`` to all 29 planes."""
    off = np.asarray(library_result['pose_off']).astype(np.int64)
    if not 0 <= int(t) < len(off) - 1:
        raise ValueError(f'reference_from_pose: no global pose {t}')
    if planes is None:
        planes = ALL_PLANES if planes_result is None else ALL_CLASS_PLANES
    if planes_result is not None:
        if receptor is None or level != 'residue':
            raise ValueError("reference_from_pose: planes_result needs the receptor's pack and level='residue'")
        if res_id is None:
            res_id = receptor.res_id
    a, b = off[int(t)], off[int(t) + 1]
    nodes, masks = reference_from_records(np.asarray(library_result['i'])[a:b], np.asarray(library_result['sift'])[a:b],
                                          np.asarray(library_result['ctype'])[a:b], res_id, planes, ctype_mask, level)
    if planes_result is None:
        return nodes, masks
    both = dict(zip(nodes.tolist(), masks.tolist()))
    for u, m in zip(*(v.tolist() for v in reference_from_plane_records(planes_result, receptor, t, planes, ctype_mask))):
        both[u] = both.get(u, 0) | m
    keys = sorted(both)
    return np.array(keys, np.int32), np.array([both[u] for u in keys], np.uint32)


def _q32(result):
    """int64 [T, Q] and the [T] / [T, Q] integer arrays it was made from: the poses' rows of a result in either form."""
    Q = len(reference_counts(result))
    skip = 0 if 'reference_count' in result else Q
    n = np.asarray(result['count']).astype(np.uint64)[skip:]
    x = np.asarray(result['cross']).astype(np.uint64).reshape(-1, Q)[skip:]
    u = n[:, None] + reference_counts(result).astype(np.uint64)[None, :] - x      # (x <= both counts: no wrap)
    # uint64 as on the device: x < 2^32, so x << 32 fits, and the quotient is at most 2^32
    s = np.where(u == 0, np.uint64(ONE_Q32), (x << np.uint64(32)) // np.maximum(u, np.uint64(1)))
    return s.astype(np.int64), n.astype(np.int64), x.astype(np.int64)


def best(result, ligand_pose_off):
    """Host mirror of arp_library_fingerprints_best: per ligand and reference the global pose of the highest ``tanimoto_q32``,
    ties to the lower pose.  ``result`` with or without its reference rows stripped; ``ligand_pose_off`` int64 [L + 1] over its
    poses.  ``first_pose`` 0 is recorded so that ``merge_best`` can place a chunk."""
    lo = np.asarray(ligand_pose_off, np.int64)
    Q = len(reference_counts(result))
    if Q < 1:
        raise ValueError('best: the result has no reference')
    s, n, x = _q32(result)
    if lo[0] != 0 or (np.diff(lo) < 0).any() or lo[-1] != len(n):
        raise ValueError('best: ligand_pose_off must run from 0 to the poses of the result without decreasing')
    L = len(lo) - 1
    out = dict(n_poses=np.diff(lo).astype(np.int64), best_pose=np.full((L, Q), -1, np.int32), tanimoto_q32=np.full((L, Q), -1, np.int64),
               shared=np.zeros((L, Q), np.uint32), count=np.zeros((L, Q), np.uint32))
    for l in range(L):
        if lo[l + 1] > lo[l]:
            k = lo[l] + np.argmax(s[lo[l]:lo[l + 1]], axis=0)      # (the first of equal scores), [Q]
            q = np.arange(Q)
            out['best_pose'][l], out['tanimoto_q32'][l], out['shared'][l], out['count'][l] = k, s[k, q], x[k, q], n[k]
    return out


def merge_best(chunks):
    """The best tables of launches over consecutive ranges of the global poses (``ligand_library.chunk_plan``; a ligand's poses
    may be cut between two of them) as one launch over all of them gives it.  ``chunks``: ``(best, first global pose)`` pairs in
    the order of the ranges; a chunk's ``best_pose`` counts from its own first pose.  The higher score wins, then the lower
    pose."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError('merge_best: no chunk')
    shape = np.asarray(chunks[0][0]['best_pose']).shape
    out = dict(n_poses=np.zeros(shape[0], np.int64), best_pose=np.full(shape, -1, np.int32), tanimoto_q32=np.full(shape, -1, np.int64),
               shared=np.zeros(shape, np.uint32), count=np.zeros(shape, np.uint32))
    for b, first in chunks:
        pose = np.asarray(b['best_pose'], np.int64)
        if pose.shape != shape:
            raise ValueError('merge_best: the chunks differ in ligands or references')
        there = pose >= 0
        pose = np.where(there, pose + int(first), -1)
        score = np.asarray(b['tanimoto_q32'], np.int64)
        have = out['best_pose'] >= 0
        take = there & (~have | (score > out['tanimoto_q32']) | ((score == out['tanimoto_q32']) & (pose < out['best_pose'])))
        out['best_pose'][take] = pose[take]
        for k in ('tanimoto_q32', 'shared', 'count'):
            out[k][take] = np.asarray(b[k])[take]
        out['n_poses'] += np.asarray(b['n_poses'], np.int64)
    return out


def _ligand_label(ligands, l):
    pc = ligands[l]
    pc.ensure_labels()
    return f'{pc.res_chain[0]}/{int(pc.res_seq[0])}/{pc.res_name[0]}'


def to_records(best_table, reference_count, ligand_pose_off=None, ligands=None):
    """For JSON: one dict per (ligand, reference) ('type': 'library-fingerprint') with the best pose as the global id and,
    given ``ligand_pose_off``, within its ligand; the score as a float and as its 32-bit fraction; shared count, the pose's
    count and the recovery of the reference.  Plain ints, floats and strings."""
    nref = np.asarray(reference_count, np.int64).reshape(-1)
    pose = np.asarray(best_table['best_pose'], np.int64)
    lo = None if ligand_pose_off is None else np.asarray(ligand_pose_off, np.int64)
    out = []
    for l in range(pose.shape[0]):
        for q in range(pose.shape[1]):
            t, s, x = int(pose[l, q]), int(best_table['tanimoto_q32'][l, q]), int(best_table['shared'][l, q])
            r = dict(ligand=l, reference=q, type='library-fingerprint', n_poses=int(best_table['n_poses'][l]), best_pose=t,
                     tanimoto_q32=s, tanimoto=(s / ONE_Q32 if t >= 0 else None), shared=x, count=int(best_table['count'][l, q]),
                     recovery=(None if t < 0 else (x / int(nref[q]) if nref[q] > 0 else 1.0)))
            if lo is not None:
                r['pose'] = t - int(lo[l]) if t >= 0 else -1
            if ligands is not None:
                r['name'] = _ligand_label(ligands, l)
            out.append(r)
    return out


CSV_HEADER = ['ligand', 'reference', 'n_poses', 'best_pose', 'tanimoto_q32', 'tanimoto', 'shared', 'count', 'recovery']


def write_csv(path, best_table, reference_count, ligand_pose_off=None, ligands=None):
    """One row per (ligand, reference), the columns of ``CSV_HEADER`` (floats as the shortest text that gives the float64 back,
    empty where the ligand has no pose); 'pose' (within the ligand) and 'name' follow when ``to_records`` has them."""
    recs = to_records(best_table, reference_count, ligand_pose_off, ligands)
    extra = [k for k in ('pose', 'name') if recs and k in recs[0]]
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER + extra)
        for r in recs:
            w.writerow([('' if r[k] is None else repr(r[k]) if isinstance(r[k], float) else r[k]) for k in CSV_HEADER + extra])


def write_library_fingerprints(wd, sid, best_table, reference_count, ligand_pose_off=None, ligands=None):
    """'<id>.libraryfp' in ``wd``."""
    path = os.path.join(wd, sid + '.libraryfp')
    write_csv(path, best_table, reference_count, ligand_pose_off, ligands)
    return path
