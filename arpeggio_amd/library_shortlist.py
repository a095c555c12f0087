"""Host side of the library shortlist (``Context.library_shortlist`` / ``InteractionComplex.run_library_shortlist``): the global
poses of a library launch — or its ligands, each by its best pose — ranked on the device, and only the chosen poses' records
copied (csrc/arp_library_shortlist.h).

A ``shortlist`` is a library table (``ligand_library``) of K one-pose entries, in rank order (descending score, ties by
ascending global pose):

    ligand     int32 [K]        the ligand of every entry
    pose       int32 [K]        its global pose (int64 once shifted to a caller's numbering)
    score      int64 [K]        (0 for a list)
    summary    uint32 [K, 16]   the library result's summary rows of the chosen poses, unfiltered
    planes_summary              the library-planes result's rows (when that result was read)
    i, a, dist, sift, ctype, pose_off    the kept atom-atom records of the chosen poses, compacted
    ligand_pose_off  int64 [K + 1] = 0 ... K: entry r stands where a ligand with one pose does, so ``ligand_library.split`` works
                                on it; ``to_records`` / ``write_csv`` here name the real ligand
    atom_plane, plane_plane, group_group, group_plane    (when requested) one dict per table, shaped as ``library_planes`` gives them

The pose score is that of ``pose_shortlist`` (``weights``, ``tanimoto_q32``).  ``scores``, ``ligand_best``, ``order``, ``take``
and ``take_planes`` are the host route over fully fetched tables — what the device result must equal.  Everything here is NumPy
and Python integers: no GPU, no native library.
"""
import csv
import os

import numpy as np

from . import ligand_library as _ll
from . import pose_shortlist as _sl
from .pose_shortlist import (CTYPE_ALL, KINDS, MAX_WEIGHT, NO_THRESHOLD, ONE_Q32, SIFT_ALL, TABLES, shift, tables_mask,      # noqa: F401
                             take_planes, tanimoto_q32, weights)

UNITS = ('poses', 'ligands')                 # ARP_LIBRARY_SHORTLIST_POSES, ARP_LIBRARY_SHORTLIST_LIGANDS


def scores(kind, summary=None, planes_summary=None, w=None, count=None, cross=None, n_refs=0, ref=0, n_poses=None):
    """The score of every global pose of a launch, a list of T Python integers, as ``pose_shortlist.scores`` — with 'tanimoto'
    over the library fingerprint's ``count`` [Q + T] and ``cross`` [Q + T, Q]: pose t is row Q + t, the reference rows are no
    poses."""
    sc = _sl.scores(kind, summary, planes_summary, w, count, cross, n_refs, ref, n_poses)
    return sc[int(n_refs):] if kind == 'tanimoto' else sc


def ligand_best(score, ligand_pose_off):
    """Per ligand its best global pose — the highest score, ties to the lower pose; -1 for a ligand without poses — and that
    score (None there): ``(int64 [L], list of L)``."""
    sc = [int(v) for v in score]
    lo = np.asarray(ligand_pose_off, np.int64).reshape(-1)
    best = np.full(len(lo) - 1, -1, np.int64)
    best_score = [None] * (len(lo) - 1)
    for l in range(len(lo) - 1):
        for t in range(int(lo[l]), int(lo[l + 1])):
            if best[l] < 0 or sc[t] > best_score[l]:
                best[l], best_score[l] = t, sc[t]
    return best, best_score


def order(score, ligand_pose_off, unit='ligands', k=None, min_score=None):
    """The chosen global poses in rank order (int64): the candidates — every global pose, or per ligand with a pose its best
    (``ligand_best``) — in descending score, ties by ascending global pose; the first ``k`` of them (``None``: all) whose score
    is at least ``min_score`` (``None``: no threshold)."""
    if unit not in UNITS:
        raise ValueError(f'order: unit must be one of {UNITS}')
    sc = [int(v) for v in score]
    if unit == 'ligands':
        cand = [int(t) for t in ligand_best(sc, ligand_pose_off)[0].tolist() if t >= 0]
    else:
        cand = list(range(len(sc)))
    ranked = sorted(cand, key=lambda t: (-sc[t], t))
    if k is not None:
        ranked = ranked[:max(int(k), 0)]
    if min_score is not None:
        ranked = [t for t in ranked if sc[t] >= int(min_score)]
    return np.asarray(ranked, np.int64).reshape(-1)


def _as_poses(table):
    """A library table read as a ``poses`` table: column ``a`` under the name ``j`` (the helpers of ``pose_shortlist`` serve)."""
    t = {k: v for k, v in table.items() if k not in ('a', 'ligand', 'ligand_pose_off')}
    if 'a' in table:
        t['j'] = table['a']
    return t


def _as_library(short, ligand):
    out = dict(short)
    if 'j' in out:
        out['a'] = out.pop('j')
    out.pop('movable', None)
    out['ligand'] = np.asarray(ligand, np.int32).reshape(-1)
    out['ligand_pose_off'] = np.arange(len(out['ligand']) + 1, dtype=np.int64)
    return out


def take(table, pose_ids, sift_mask=0, ctype_mask=CTYPE_ALL):
    """The host route to the atom-atom part of a shortlist, over a fully fetched ``Context.library_contacts`` table: the records
    of the global poses ``pose_ids`` (in that order, repeats allowed), filtered as ``pose_shortlist.take`` filters, with
    ``pose_off`` [K + 1], the unfiltered ``summary`` rows, ``pose``, ``ligand`` and ``ligand_pose_off``."""
    ids = np.asarray(pose_ids, np.int64).reshape(-1)
    return _as_library(_sl.take(_as_poses(table), ids, sift_mask, ctype_mask), _ll.ligand_of(table)[ids])


def merge(chunks, k, unit='ligands'):
    """The global best ``k`` of per-chunk shortlists whose ``pose`` has been shifted to the caller's global poses (``shift``).
    Unit 'ligands': a ligand whose poses were cut between two chunks appears in both — of a ligand's entries the one with the
    higher score, then the lower global pose, is kept BEFORE the best ``k`` are taken.  Then descending score, a tie to the
    lower global pose, the first ``k`` (fewer when there are fewer) with their records."""
    if unit not in UNITS:
        raise ValueError(f'merge: unit must be one of {UNITS}')
    chunks = list(chunks)
    joined = _sl.concat([_as_poses(c) for c in chunks])
    ligand = np.concatenate([np.asarray(c['ligand'], np.int64).reshape(-1) for c in chunks])
    pose, score = np.asarray(joined['pose']).astype(np.int64).tolist(), np.asarray(joined['score'], np.int64).tolist()
    rows = sorted(range(len(pose)), key=lambda r: (-score[r], pose[r]))
    if unit == 'ligands':
        seen, first = set(), []
        for r in rows:      # (in rank order the first entry of a ligand is its best)
            if int(ligand[r]) not in seen:
                seen.add(int(ligand[r]))
                first.append(r)
        rows = first
    rows = rows[:max(int(k), 0)]
    return _as_library(_sl._select(joined, rows), ligand[np.asarray(rows, np.int64)])


def _rows(short, receptor, ligands, component_types):
    """``ligand_library._rows`` over the entries, each row with its rank (the entry stands where a ligand does)."""
    lig = np.asarray(short['ligand']).astype(np.int64).tolist()
    return _ll._rows(short, receptor, [ligands[l] for l in lig], component_types)


def to_records(short, receptor, ligands, component_types=None):
    """The kept atom-atom records as the dicts ``ligand_library.to_records`` gives, each with 'rank' (its place in the
    shortlist), 'ligand', 'pose' (the global pose) and 'score' (a plain int)."""
    lig, pose, score = (np.asarray(short[c]).astype(np.int64).tolist() for c in ('ligand', 'pose', 'score'))
    return [{'rank': r, 'ligand': lig[r], 'pose': pose[r], 'score': score[r], 'bgn': rec.atom_dict(i), 'end': lab.atom_dict(a), 'type': 'atom-atom',
             'distance': d, 'contact': names, 'interacting_entities': ct}
            for r, _, rec, i, lab, a, d, names, ct in _rows(short, receptor, ligands, component_types)]


CSV_HEADER = ['rank', 'ligand', 'pose', 'score'] + _ll.CSV_HEADER[2:]


def write_csv(path, short, receptor, ligands, component_types=None):
    """One row per kept atom-atom record: rank, ligand, global pose and score, then the columns of ``ligand_library.write_csv``."""
    lig, pose, score = (np.asarray(short[c]).astype(np.int64).tolist() for c in ('ligand', 'pose', 'score'))
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r, _, rec, i, lab, a, d, names, ct in _rows(short, receptor, ligands, component_types):
            w.writerow([r, lig[r], pose[r], score[r], rec.atom_macro(i), lab.atom_macro(a), d, '|'.join(names), ct])


def write_library_shortlist(wd, sid, short, receptor, ligands, component_types=None):
    """'<id>.libraryshortlist' in ``wd``."""
    path = os.path.join(wd, sid + '.libraryshortlist')
    write_csv(path, short, receptor, ligands, component_types)
    return path
