"""Host side of the pose shortlist (``Context.poses_shortlist`` / ``InteractionComplex.run_pose_shortlist``): the poses of a
launch ranked on the device, and only the chosen poses' records copied (csrc/arp_poses_shortlist.h).

A ``shortlist`` is a dict:

    pose       int32 [K]        the chosen poses in rank order (descending score, ties by ascending pose id)
    score      int64 [K]        their scores (0 for a list)
    summary    uint32 [K, 16]   the poses result's summary rows of the chosen poses, unfiltered
    planes_summary              the poses-planes result's rows (when that result was read)
    i, j, dist, sift, ctype, pose_off    the kept atom-atom records of the chosen poses, compacted: a ``poses`` table of K poses
                                (``poses.split``, ``poses.partners``, ``poses.fingerprints``, ``poses.to_records`` work on it)
    atom_plane, plane_plane, group_group, group_plane    (when requested) one dict per table, shaped as ``poses_planes`` gives them
    movable    int32 [S]

The score is an integer: a weighted sum of summary slots (``weights``), or the Tanimoto similarity to a reference pose in 32
fractional bits (``tanimoto_q32``).  ``scores``, ``order``, ``take`` and ``take_planes`` are the host route over fully fetched
tables — what the device result must equal.  Everything here is NumPy and Python integers: no GPU, no native library.
"""
import csv
import os

import numpy as np

from . import poses
from .core import config

KINDS = ('list', 'summary', 'tanimoto')      # ARP_SHORTLIST_LIST, ARP_SHORTLIST_SUMMARY, ARP_SHORTLIST_TANIMOTO
TABLES = ('atom_atom',) + poses.PLANE_TABLES  # bit t of the `tables` mask
MAX_WEIGHT = 1 << 24                         # ARP_SHORTLIST_MAX_WEIGHT
ONE_Q32 = 1 << 32                            # the Tanimoto similarity 1.0
NO_THRESHOLD = -(1 << 63)                    # INT64_MIN
SIFT_ALL, CTYPE_ALL = 0x7FFF, 0x7F
ATOM_ATOM_SLOTS = tuple(config.SIFT_NAMES[:poses.N_BITS]) + ('records',)


def tables_mask(tables):
    """The ``tables`` mask of the names in ``tables`` (``TABLES``; a single name may be given as a string)."""
    chosen = (tables,) if isinstance(tables, str) else tuple(tables)
    mask = 0
    for name in chosen:
        if name not in TABLES:
            raise ValueError(f'tables_mask: no table {name!r} ({", ".join(TABLES)})')
        mask |= 1 << TABLES.index(name)
    if not mask:
        raise ValueError('tables_mask: no table named')
    return mask


def weights(atom_atom=None, planes=None):
    """int32 [32] for a ranking by summary: ``atom_atom`` maps SIFt names (``config.SIFT_NAMES``, or 'records' for slot 15) to
    the weight of that slot of the poses result's summary, ``planes`` maps ``poses.PLANE_SUMMARY_SLOTS`` names to the weight of
    that slot of the poses-planes result's.  Integers of magnitude at most 2^24."""
    w = np.zeros(32, np.int32)
    for base, names, given, what in ((0, ATOM_ATOM_SLOTS, atom_atom, 'atom_atom'), (16, poses.PLANE_SUMMARY_SLOTS, planes, 'planes')):
        for name, v in (given or {}).items():
            if name not in names:
                raise ValueError(f'weights: no {what} summary slot {name!r}')
            if int(v) != v or abs(int(v)) > MAX_WEIGHT:
                raise ValueError(f'weights: {name!r} must be an integer of magnitude at most 2^24')
            w[base + names.index(name)] = int(v)
    return w


def tanimoto_q32(count, cross, n_refs, ref):
    """The Tanimoto score of every pose of a fingerprint launch as the device computes it, a list of P Python integers: for
    reference q, t = cross[p][q], u = count[p] + count[q] - t, floor(t 2^32 / u), and 2^32 where u = 0 (0 / 0 is 1.0, as
    ``pose_fingerprints.tanimoto``).  ``ref`` names the reference; -1 takes the largest over all ``n_refs``."""
    n = np.asarray(count).reshape(-1).astype(np.uint64)
    Q = int(n_refs)
    if Q < 1 or not -1 <= int(ref) < Q:
        raise ValueError('tanimoto_q32: ref must be -1 or in [0, n_refs), n_refs >= 1')
    t = np.asarray(cross).reshape(len(n), -1).astype(np.uint64)[:, :Q]
    u = n[:, None] + n[None, :Q] - t                       # (t <= both counts: no wrap; t < 2^32: t << 32 fits 64 bits)
    q32 = np.where(u == 0, np.uint64(ONE_Q32), (t << np.uint64(32)) // np.maximum(u, np.uint64(1)))
    best = q32.max(axis=1) if int(ref) < 0 else q32[:, int(ref)]
    return [int(v) for v in best.tolist()]


def scores(kind, summary=None, planes_summary=None, w=None, count=None, cross=None, n_refs=0, ref=0, n_poses=None):
    """The score of every pose of a launch, a list of P Python integers: 'summary' — the weighted sum of the slots of
    ``summary`` [P, 16] and, where ``planes_summary`` is given, of its slots with ``w[16:]``; 'tanimoto' — ``tanimoto_q32``;
    'list' — zeros (``n_poses`` of them)."""
    if kind not in KINDS:
        raise ValueError(f'scores: kind must be one of {KINDS}')
    if kind == 'list':
        return [0] * int(n_poses)
    if kind == 'tanimoto':
        return tanimoto_q32(count, cross, n_refs, ref)
    w64 = np.asarray(w).reshape(-1).astype(np.int64)
    if len(w64) != 32 or int(np.abs(w64).max()) > MAX_WEIGHT:
        raise ValueError('scores: 32 weights of magnitude at most 2^24')
    if planes_summary is None and w64[16:].any():
        raise ValueError('scores: a weight on a planes slot needs planes_summary')
    # (32 terms below 2^24 * 2^32: the sum fits int64 with room to spare, so the int64 product is exact)
    sc = np.asarray(summary, np.uint32).reshape(-1, 16).astype(np.int64) @ w64[:16]
    if planes_summary is not None:
        sc = sc + np.asarray(planes_summary, np.uint32).reshape(-1, 16).astype(np.int64) @ w64[16:]
    return [int(v) for v in sc.tolist()]


def order(score, skip=0, k=None, min_score=None):
    """The ranked poses ``skip <= p < P`` in descending score, ties by ascending pose id (a stable argsort of the negated
    score); the first ``k`` of them (``None``: all) whose score is at least ``min_score`` (``None``: no threshold).  int64."""
    sc = np.asarray([int(v) for v in score], np.int64).reshape(-1)      # (|score| < 2^61: the negation cannot wrap)
    ranked = int(skip) + np.argsort(-sc[int(skip):], kind='stable').astype(np.int64)
    if k is not None:
        ranked = ranked[:max(int(k), 0)]
    if min_score is not None:
        ranked = ranked[sc[ranked] >= max(int(min_score), NO_THRESHOLD)]
    return ranked


def _kept_rows(off, ids, keep):
    """Per pose of ``ids`` the row numbers of its segment [off[p], off[p + 1]) that ``keep(s, e)`` (a bool array, or None for
    all) keeps — only the chosen poses' rows are looked at."""
    off = np.asarray(off).astype(np.int64)
    out = []
    for p in np.asarray(ids, np.int64).tolist():
        s, e = int(off[p]), int(off[p + 1])
        rows = np.arange(s, e)
        k = keep(s, e)
        out.append(rows if k is None else rows[k])
    return out


def take(table, pose_ids, sift_mask=0, ctype_mask=CTYPE_ALL):
    """The host route to the atom-atom part of a shortlist, over a fully fetched ``Context.poses_contacts`` table: the records
    of the poses ``pose_ids`` (in that order, repeats allowed) with bit ``ctype`` in ``ctype_mask`` and, where ``sift_mask`` is
    not 0, a SIFt bit in ``sift_mask`` — in the order the table holds them — with ``pose_off`` [K + 1], the unfiltered
    ``summary`` rows, ``pose`` and ``movable``."""
    ids = np.asarray(pose_ids, np.int64).reshape(-1)
    cols = {c: np.asarray(table[c]) for c in poses.COLUMNS}

    def keep(s, e):
        if not int(sift_mask) and int(ctype_mask) & CTYPE_ALL == CTYPE_ALL:
            return None
        k = ((int(ctype_mask) >> cols['ctype'][s:e].astype(np.int64)) & 1) != 0
        return k & ((cols['sift'][s:e].astype(np.int64) & int(sift_mask)) != 0) if int(sift_mask) else k
    idx = _kept_rows(table['pose_off'], ids, keep)
    rows = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    out = {c: cols[c][rows.astype(np.int64)].astype(poses.DTYPES[c]) for c in poses.COLUMNS}
    out['pose_off'] = np.concatenate([[0], np.cumsum([len(x) for x in idx])]).astype(np.uint64)
    out['summary'] = np.asarray(table['summary'], np.uint32).reshape(-1, poses.SUMMARY)[ids]
    out['pose'] = ids.astype(np.int32)
    if 'movable' in table:
        out['movable'] = np.asarray(table['movable'])
    return out


def take_planes(planes_table, pose_ids, ctype_mask=CTYPE_ALL, tables=poses.PLANE_TABLES):
    """``take`` for the ring and amide tables of a fully fetched ``Context.poses_planes`` result: per table of ``tables`` the
    records of the poses ``pose_ids`` with bit ``ctype`` in ``ctype_mask``, in the table's order, with ``pose_off``; and the
    unfiltered ``summary`` rows."""
    ids = np.asarray(pose_ids, np.int64).reshape(-1)
    out = {}
    for name in tables:
        src = planes_table[name]
        ct = np.asarray(src['ctype'])
        idx = _kept_rows(src['pose_off'], ids, lambda s, e: ((int(ctype_mask) >> ct[s:e].astype(np.int64)) & 1) != 0)
        rows = (np.concatenate(idx) if idx else np.zeros(0, np.int64)).astype(np.int64)
        tab = {c: np.asarray(src[c])[rows].astype(dt) for c, dt in poses.plane_columns(name)}
        tab['pose_off'] = np.concatenate([[0], np.cumsum([len(x) for x in idx])]).astype(np.uint64)
        out[name] = tab
    out['summary'] = np.asarray(planes_table['summary'], np.uint32).reshape(-1, poses.SUMMARY)[ids]
    return out


def _select(short, rows):
    """The shortlist made of the entries ``rows`` of ``short`` (in that order)."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    out = {k: v for k, v in short.items() if k not in poses.COLUMNS and k not in TABLES and k not in ('pose', 'score', 'summary', 'planes_summary', 'pose_off')}
    out['pose'] = np.asarray(short['pose'])[rows]
    out['score'] = np.asarray(short['score'], np.int64)[rows]
    for name in ('summary', 'planes_summary'):
        if name in short:
            out[name] = np.asarray(short[name], np.uint32).reshape(-1, poses.SUMMARY)[rows]
    if 'pose_off' in short:
        part = take(dict(short, summary=np.zeros((len(short['pose']), poses.SUMMARY), np.uint32)), rows)
        out.update({c: part[c] for c in poses.COLUMNS})
        out['pose_off'] = part['pose_off']
    have = [name for name in poses.PLANE_TABLES if name in short]
    if have:
        part = take_planes(dict(short, summary=np.zeros((len(short['pose']), poses.SUMMARY), np.uint32)), rows, tables=have)
        out.update({name: part[name] for name in have})
    return out


def concat(chunks):
    """Shortlists one after the other as one (no re-ranking): entries, records and offsets joined in the order given."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError('concat: no chunk')
    first = chunks[0]
    out = {k: v for k, v in first.items() if k not in poses.COLUMNS and k not in TABLES and k not in ('pose', 'score', 'summary', 'planes_summary', 'pose_off')}
    out['pose'] = np.concatenate([np.asarray(c['pose']).astype(np.int64) for c in chunks])
    out['score'] = np.concatenate([np.asarray(c['score'], np.int64) for c in chunks])
    for name in ('summary', 'planes_summary'):
        if name in first:
            out[name] = np.concatenate([np.asarray(c[name], np.uint32).reshape(-1, poses.SUMMARY) for c in chunks])

    def joined_off(tabs):
        base, offs = 0, [np.zeros(1, np.uint64)]
        for t in tabs:
            o = np.asarray(t['pose_off']).astype(np.uint64)
            offs.append(o[1:] + np.uint64(base))
            base += int(o[-1])
        return np.concatenate(offs)

    if 'pose_off' in first:
        for c in poses.COLUMNS:
            out[c] = np.concatenate([np.asarray(ch[c]) for ch in chunks]).astype(poses.DTYPES[c])
        out['pose_off'] = joined_off(chunks)
    for name in poses.PLANE_TABLES:
        if name in first:
            out[name] = {c: np.concatenate([np.asarray(ch[name][c]) for ch in chunks]).astype(dt) for c, dt in poses.plane_columns(name)}
            out[name]['pose_off'] = joined_off([ch[name] for ch in chunks])
    return out


def merge(chunks, k):
    """The global best ``k`` of per-chunk shortlists whose ``pose`` has been shifted to global ids: the entries of all chunks
    in descending score, a tie going to the lower global id, the first ``k`` of them (fewer when there are fewer) with their
    records."""
    joined = concat(chunks)
    pose, score = np.asarray(joined['pose']).astype(np.int64).tolist(), np.asarray(joined['score'], np.int64).tolist()
    rows = sorted(range(len(pose)), key=lambda r: (-score[r], pose[r]))[:max(int(k), 0)]
    return _select(joined, rows)


def shift(short, base):
    """The shortlist with ``base`` added to its pose ids (int64): a chunk's ids in the caller's numbering."""
    out = dict(short)
    out['pose'] = np.asarray(short['pose']).astype(np.int64) + int(base)
    return out


def to_records(short, pc, component_types=None):
    """The kept atom-atom records as the dicts ``poses.to_records`` gives, each with 'rank' (its place in the shortlist), 'pose'
    (the pose id) and 'score' (a plain int)."""
    pose, score = np.asarray(short['pose']).tolist(), np.asarray(short['score'], np.int64).tolist()
    out = poses.to_records(short, pc, component_types)
    for rec in out:
        r = rec['pose']
        rec['rank'], rec['pose'], rec['score'] = r, int(pose[r]), int(score[r])
    return out


CSV_HEADER = ['rank', 'pose', 'score'] + poses.CSV_HEADER[1:]


def write_csv(path, short, pc, component_types=None):
    """One row per kept atom-atom record: rank, pose and score, then the columns of ``poses.write_csv``."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    ct = config.CONTACT_TYPE_NAMES
    pose, score = np.asarray(short['pose']).tolist(), np.asarray(short['score'], np.int64).tolist()
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r, i, j, d, s, c in zip(poses.pose_of(short).tolist(), np.asarray(short['i']).tolist(), np.asarray(short['j']).tolist(),
                                    export.rounded(short['dist']), np.asarray(short['sift']).tolist(), np.asarray(short['ctype']).tolist()):
            w.writerow([r, int(pose[r]), int(score[r]), lab.atom_macro(i), lab.atom_macro(j), d,
                        '|'.join(n for k, n in enumerate(config.SIFT_NAMES) if (s >> k) & 1), ct[c]])


def write_pose_shortlist(wd, sid, short, pc, component_types=None):
    """'<id>.shortlist' in ``wd``."""
    path = os.path.join(wd, sid + '.shortlist')
    write_csv(path, short, pc, component_types)
    return path
