"""Host side of the pose fingerprints (``Context.poses_fingerprints`` / ``InteractionComplex.run_pose_fingerprints``): which
poses of a ligand reproduce the interactions of reference poses, which receptor nodes the poses touch and how often.

The device delivers a ``result``, a dict of small integer arrays made from the resident poses result
(csrc/arp_poses_fingerprints.h).  A feature is (node, plane): a receptor residue (``level='residue'``) or receptor atom
(``'atom'``) and one of the SIFt bits of ``planes`` (``config.SIFT_NAMES``) — "the pose has a participating record with that
bit to that node".  The first ``n_refs`` poses of a launch are its references.

    ids        int32  [U]           the nodes that occur in any pose of the launch, ascending
    count      uint32 [P]           features of pose p
    cross      uint32 [P, Q]        features pose p shares with reference q
    occupancy  uint32 [U, NP]       poses behind the references that have feature (ids[u], k-th selected plane)
    planes, n_refs, level           what it was made with
    bits       uint64 [P, NP, ceil(U / 64)]   (on request) the bit matrix: feature (u, k) is bit u & 63 of word u >> 6 of plane k
    inter      uint32 [P, P]        (on request) features two poses share

In a result as the device gives it the reference rows are the first ``n_refs`` rows of ``count`` / ``cross``.
``strip_references`` moves them to ``reference_count`` / ``reference_cross`` (what ``run_pose_fingerprints`` returns); every function here
takes either form.  Everything here is NumPy on the host: no GPU, no native library.
"""
import csv
import os

import numpy as np

from . import similarity
from .core import config

N_PLANES = 15          # ARP_POSEFP_PLANES
N_ALL_PLANES = 29      # ARP_POSEFP_ALL_PLANES
MAX_REFS = 64          # ARP_POSEFP_MAX_REFS
LEVELS = ('residue', 'atom')
# The ring and amide classes as planes 15 ... 28 (residue level only).  A record takes part when exactly one of its two entities
# is the ligand's; the name says which side the ligand supplies where the table has two kinds of entity, the node is the
# residue of the other.
CLASS_PLANE_NAMES = tuple([f'{n}_LIGAND_ATOM' for n in config.ATOM_PLANE_NAMES] + [f'{n}_LIGAND_RING' for n in config.ATOM_PLANE_NAMES] +
                          ['PLANE_PLANE', 'GROUP_GROUP', 'GROUP_PLANE_LIGAND_AMIDE', 'GROUP_PLANE_LIGAND_RING'])
CLASS_SHORTHANDS = {'atom_plane': CLASS_PLANE_NAMES[:10], 'plane_plane': CLASS_PLANE_NAMES[10:11], 'group_group': CLASS_PLANE_NAMES[11:12],
                    'group_plane': CLASS_PLANE_NAMES[12:], 'all': CLASS_PLANE_NAMES}
assert len(CLASS_PLANE_NAMES) == N_ALL_PLANES - N_PLANES


def planes(contacts=None, classes=()):
    """The ``planes`` mask of the contacts named in ``contacts`` (``similarity.planes`` without class planes: ``None`` means
    every contact but bare proximity) and of the ring / amide classes named in ``classes``: names of ``CLASS_PLANE_NAMES``, the
    shorthands 'atom_plane', 'plane_plane', 'group_group', 'group_plane' (every plane of that table) or 'all' (all 14); a
    single name may be given as a string.  ``contacts=[]`` with classes gives the class planes alone; a mask without any plane
    raises ``ValueError``."""
    chosen = tuple((classes,) if isinstance(classes, str) else classes)
    mask = 0 if (chosen and contacts is not None and len(contacts) == 0) else similarity.planes(contacts)
    for name in chosen:
        if name in CLASS_SHORTHANDS:
            members = CLASS_SHORTHANDS[name]
        elif name in CLASS_PLANE_NAMES:
            members = (name,)
        else:
            raise ValueError(f'planes: no class plane {name!r} (CLASS_PLANE_NAMES, or a table, or all)')
        for m in members:
            mask |= 1 << (N_PLANES + CLASS_PLANE_NAMES.index(m))
    return mask


def plane_names(mask):
    """The names of the selected planes, in the order of the plane axis."""
    return [config.SIFT_NAMES[k] for k in range(N_PLANES) if (int(mask) >> k) & 1] + \
           [CLASS_PLANE_NAMES[k - N_PLANES] for k in range(N_PLANES, N_ALL_PLANES) if (int(mask) >> k) & 1]


def reference_counts(result):
    """int64 [Q]: the feature counts of the references."""
    if 'reference_count' in result:
        return np.asarray(result['reference_count']).astype(np.int64)
    return np.asarray(result['count']).astype(np.int64)[:int(result['n_refs'])]


def _cross(result):
    a = np.asarray(result['cross']).astype(np.int64)
    if a.ndim != 2 or a.shape[0] != len(result['count']) or a.shape[1] != len(reference_counts(result)):
        raise ValueError('pose_fingerprints: cross must be [P, n_refs]')
    return a


def tanimoto(result):
    """float64 [P, Q]: cross / (count[p] + count[ref q] - cross); 1.0 where pose and reference both have no feature, as
    ``similarity.tanimoto`` decides it."""
    a = _cross(result)
    union = np.asarray(result['count']).astype(np.int64)[:, None] + reference_counts(result)[None, :] - a
    t = np.ones(a.shape, np.float64)
    np.divide(a, union, out=t, where=union > 0)
    return t


def recovery(result):
    """float64 [P, Q]: cross / count[ref q], the share of the reference's features the pose reproduces; 1.0 for a reference
    without features."""
    a = _cross(result)
    n = np.broadcast_to(reference_counts(result)[None, :], a.shape)
    t = np.ones(a.shape, np.float64)
    np.divide(a, n, out=t, where=n > 0)
    return t


def rank(result, q=0, by='tanimoto'):
    """The poses ordered by their score against reference ``q``, best first (int64 [P]); the lower index wins a tie.  ``by``:
    'tanimoto', 'recovery' or 'shared' (the shared count itself)."""
    if by not in ('tanimoto', 'recovery', 'shared'):
        raise ValueError("rank: by must be 'tanimoto', 'recovery' or 'shared'")
    a = _cross(result)
    if not 0 <= q < a.shape[1]:
        raise ValueError(f'rank: no reference {q}')
    score = (tanimoto(result) if by == 'tanimoto' else recovery(result) if by == 'recovery' else a.astype(np.float64))[:, q]
    return np.argsort(-score, kind='stable').astype(np.int64)


def unpack(result):
    """bool [P, U, NP] from ``bits``."""
    b = np.ascontiguousarray(result['bits'], np.uint64)
    U = len(result['ids'])
    if b.ndim != 3 or b.shape[2] != (U + 63) // 64:
        raise ValueError('unpack: bits must be [P, NP, ceil(U / 64)]')
    P, NP, wpp = b.shape
    on = np.unpackbits(b.astype('<u8').view(np.uint8).reshape(P, NP, wpp * 8), axis=2, bitorder='little')[:, :, :U]
    return np.ascontiguousarray(on.astype(bool).transpose(0, 2, 1))


def strip_references(result):
    """The result with its reference rows moved out of ``count`` / ``cross`` into ``reference_count`` / ``reference_cross``."""
    if 'reference_count' in result:
        return dict(result)
    Q = int(result['n_refs'])
    out = {k: v for k, v in result.items() if k not in ('bits', 'inter')}
    out['reference_count'], out['reference_cross'] = np.asarray(result['count'])[:Q].copy(), np.asarray(result['cross'])[:Q].copy()
    out['count'], out['cross'] = np.asarray(result['count'])[Q:].copy(), np.asarray(result['cross'])[Q:].copy()
    return out


def merge(chunks):
    """The results of launches that each carried the same references in front of their own poses, as one launch over all the
    poses would give it: ``ids`` is the union, ``occupancy`` is added by id, ``count`` / ``cross`` rows are concatenated with
    every chunk's reference rows dropped after the first.  ``ValueError`` when planes, level or the references' ``count`` /
    ``cross`` block differ between chunks.  ``bits`` and ``inter`` are not carried over."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError('merge: no chunk')
    if any('reference_count' in c for c in chunks):
        raise ValueError('merge: a chunk has its references stripped (merge first, strip then)')
    first = chunks[0]
    Q = int(first['n_refs'])
    for c in chunks[1:]:
        if int(c['planes']) != int(first['planes']) or c['level'] != first['level'] or int(c['n_refs']) != Q:
            raise ValueError('merge: the chunks were made with different planes, level or n_refs')
        if not (np.array_equal(np.asarray(c['count'])[:Q], np.asarray(first['count'])[:Q]) and
                np.array_equal(np.asarray(c['cross'])[:Q], np.asarray(first['cross'])[:Q])):
            raise ValueError('merge: the chunks carry different references')
    NP = bin(int(first['planes'])).count('1')
    ids = np.unique(np.concatenate([np.asarray(c['ids'], np.int32) for c in chunks]))
    occ = np.zeros((len(ids), NP), np.uint32)
    for c in chunks:
        occ[np.searchsorted(ids, np.asarray(c['ids'], np.int32))] += np.asarray(c['occupancy'], np.uint32).reshape(-1, NP)
    out = dict(ids=ids, occupancy=occ, planes=int(first['planes']), n_refs=Q, level=first['level'])
    out['count'] = np.concatenate([np.asarray(c['count'], np.uint32)[Q if k else 0:] for k, c in enumerate(chunks)])
    out['cross'] = np.concatenate([np.asarray(c['cross'], np.uint32).reshape(-1, Q)[Q if k else 0:] for k, c in enumerate(chunks)])
    return out


def _labels(pc, level, component_types):
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    return lab.atom_macro if level == 'atom' else (lambda r: lab.res_macro[r])


def to_records(result, pc, component_types=None):
    """For JSON: one dict per pose ('type': 'pose-fingerprint') with its count and per reference the shared count, Tanimoto and
    recovery; then one per node ('pose-occupancy') with the number of poses per selected plane; plain ints, floats, strings."""
    a, t, r = _cross(result), tanimoto(result), recovery(result)
    names = plane_names(result['planes'])
    label = _labels(pc, result['level'], component_types)
    out = [{'pose': p, 'type': 'pose-fingerprint', 'count': int(n),
            'references': [{'reference': q, 'shared': int(a[p, q]), 'tanimoto': float(t[p, q]), 'recovery': float(r[p, q])}
                           for q in range(a.shape[1])]}
           for p, n in enumerate(np.asarray(result['count']).tolist())]
    occ = np.asarray(result['occupancy']).reshape(len(result['ids']), len(names))
    out += [{'node': label(int(u)), 'type': 'pose-occupancy', 'level': result['level'],
             'poses': {nm: int(v) for nm, v in zip(names, row)}} for u, row in zip(np.asarray(result['ids']).tolist(), occ.tolist())]
    return out


def csv_header(result):
    Q = len(reference_counts(result))
    return ['pose', 'count'] + [f'{what}_{q}' for q in range(Q) for what in ('shared', 'tanimoto', 'recovery')]


def write_csv(path, result, pc, component_types=None):
    """One row per pose: pose, count and per reference the shared count, the Tanimoto similarity and the recovery (floats as the
    shortest text that gives the float64 back); then a second header ('node' and the names of the selected planes) and the
    occupancy rows, the node in the form the other CSV tables use ('A/508/' for a residue, 'A/508/O' for an atom)."""
    a, t, r = _cross(result), tanimoto(result), recovery(result)
    names = plane_names(result['planes'])
    label = _labels(pc, result['level'], component_types)
    occ = np.asarray(result['occupancy']).reshape(len(result['ids']), len(names))
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(csv_header(result))
        for p, n in enumerate(np.asarray(result['count']).tolist()):
            row = [p, int(n)]
            for q in range(a.shape[1]):
                row += [int(a[p, q]), repr(float(t[p, q])), repr(float(r[p, q]))]
            w.writerow(row)
        w.writerow(['node'] + names)
        for u, row in zip(np.asarray(result['ids']).tolist(), occ.tolist()):
            w.writerow([label(int(u))] + [int(v) for v in row])


def write_pose_fingerprints(wd, sid, result, pc, component_types=None):
    """'<id>.posefp' in ``wd``."""
    path = os.path.join(wd, sid + '.posefp')
    write_csv(path, result, pc, component_types)
    return path
