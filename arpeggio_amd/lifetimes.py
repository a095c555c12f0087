"""Host side of the contact-lifetimes table (``Context.models_lifetimes`` / ``EnsembleComplex.run_lifetimes``): how long a
contact lasts along the ordered axis of an ensemble's models and how often it forms and breaks, where the persistence table
(``arpeggio_amd.persistence``) gives the fraction of models that have it.

Inputs: F resident models, the atom-atom bag of a pass over them, and three launch arguments — ``gap`` (0 ... 65534: models
of absence tolerated inside an interval), ``sift_any`` (15 bits, not 0) and ``ctype_mask`` (contact types, not 0, in the bit
order of ``contact_filter.masks``).

Which records take part.  A record takes part when ``(sift & sift_any) != 0`` and bit ``ctype`` of ``ctype_mask`` is set.
With ``0x7FFF`` and every contact type set, every record takes part.

Rows.  One row per topology pair (a, b), a < b, that has at least one participating record, in ascending (a, b).

Intervals.  Let a pair's participating models be f1 < f2 < ... < fm.  An *interval* is a maximal stretch in which consecutive
present models differ by at most ``gap + 1``.  Its *span* is ``f_end - f_start + 1``, so bridged holes count.

A table is a dict of eleven NumPy columns (``tables.LIFETIMES``, the order of the C fetch's arguments):

    a, b            int32    topology atom ids
    n_models        uint16   m
    first, last     int32    f1, fm
    n_intervals     uint16   number of intervals
    longest         uint16   the largest span
    longest_start   int32    first model of the interval with the largest span; on a tie, the earliest
    head, tail      uint16   span of the first and of the last interval (equal when n_intervals == 1)
    span_sum        uint32   sum of all spans (mean lifetime = span_sum / n_intervals)

With the all-records masks, a, b, n_models, first and last are byte-equal to the same columns of ``models_persistence()`` on
the same pass.  ``head`` and ``tail`` exist so that two chunk tables of one trajectory merge exactly (``merge``).

Everything here is NumPy on the host: no GPU is needed to merge, normalise or export tables.
"""
import csv
import os

import numpy as np

from . import tables

COLUMNS = tables.LIFETIMES.columns
MAX_GAP = 65534
_TOP = {'n_models': 65535, 'n_intervals': 65535, 'longest': 65535, 'head': 65535, 'tail': 65535, 'span_sum': 0xFFFFFFFF}


def empty():
    """A table without rows."""
    return tables.empty(tables.LIFETIMES)


def check_gap(gap):
    gap = int(gap)
    if not 0 <= gap <= MAX_GAP:
        raise ValueError(f'lifetimes: gap must lie in 0 ... {MAX_GAP}')
    return gap


def merge(t1, t2, model_offset, gap):
    """The table of two chunks of one trajectory, EXACTLY that of the whole: ``t1`` over models [0, model_offset), ``t2`` over
    the models that follow (its 0-based model indices are shifted by ``model_offset``), both made with ``gap`` and the same
    masks.  Rows are joined on (a, b) and come back in that order.  For a pair in both tables, with
    ``delta = t2.first + model_offset - t1.last``:

    - ``delta <= gap + 1``: t1's tail and t2's head are one interval of span ``j = t1.tail + t2.head + delta - 1``;
      ``n_intervals = n1 + n2 - 1``, ``span_sum = s1 + s2 + delta - 1``, ``head = j if n1 == 1 else t1.head``,
      ``tail = j if n2 == 1 else t2.tail``;
    - otherwise the counts and ``span_sum`` add, ``head = t1.head`` and ``tail = t2.tail``;
    - ``longest`` / ``longest_start`` are decided among three candidates taken in time order and replaced only by a strictly
      larger span: ``(t1.longest, t1.longest_start)``, the joined interval ``(j, t1.last - t1.tail + 1)`` if any, and
      ``(t2.longest, t2.longest_start + model_offset)``.

    A pair that one side lacks is copied (t2's model indices shifted).  ``OverflowError`` when a merged value leaves its
    column's type, as ``tables.merge``; ``ValueError`` when a model of ``t2`` would not follow every model of ``t1``."""
    model_offset, gap = int(model_offset), check_gap(gap)
    if model_offset < 0:
        raise ValueError('merge: model_offset must not be negative')
    a = np.concatenate([t1['a'], t2['a']]).astype(np.int64)
    b = np.concatenate([t1['b'], t2['b']]).astype(np.int64)
    n1 = len(t1['a'])
    stride = int(b.max()) + 1 if len(b) else 1
    key, inv = np.unique(a * stride + b, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(key)
    r1, r2 = inv[:n1], inv[n1:]      # (a table's pairs are distinct: each of r1, r2 hits a row at most once)
    has1, has2 = np.zeros(U, bool), np.zeros(U, bool)
    has1[r1] = True
    has2[r2] = True
    # both sides as int64 columns over the U rows (0 where a side lacks the pair), t2's model indices shifted
    x, y = ({k: np.zeros(U, np.int64) for k, _ in COLUMNS[2:]} for _ in range(2))
    for k, _ in COLUMNS[2:]:
        x[k][r1] = t1[k]
        y[k][r2] = t2[k]
    for k in ('first', 'last', 'longest_start'):
        y[k][r2] += model_offset
    both = has1 & has2
    delta = y['first'] - x['last']
    if both.any() and delta[both].min() < 1:
        raise ValueError('merge: a model of t2 does not follow the models of t1 (model_offset too small)')
    joined = both & (delta <= gap + 1)
    j = x['tail'] + y['head'] + delta - 1
    m = {}
    m['n_models'] = x['n_models'] + y['n_models']
    m['first'] = np.where(has1, x['first'], y['first'])
    m['last'] = np.where(has2, y['last'], x['last'])
    m['n_intervals'] = x['n_intervals'] + y['n_intervals'] - joined
    m['span_sum'] = x['span_sum'] + y['span_sum'] + np.where(joined, delta - 1, 0)
    m['head'] = np.where(has1, np.where(joined & (x['n_intervals'] == 1), j, x['head']), y['head'])
    m['tail'] = np.where(has2, np.where(joined & (y['n_intervals'] == 1), j, y['tail']), x['tail'])
    # the three candidates in time order (a side that lacks the pair brings span 0, which replaces nothing)
    longest, start = x['longest'].copy(), x['longest_start'].copy()
    for span, at, live in ((j, x['last'] - x['tail'] + 1, joined), (y['longest'], y['longest_start'], has2)):
        better = live & (span > longest)
        longest, start = np.where(better, span, longest), np.where(better, at, start)
    m['longest'], m['longest_start'] = longest, start
    out = tables.alloc(tables.LIFETIMES, U, np.zeros)
    out['a'], out['b'] = (key // stride).astype(np.int32), (key % stride).astype(np.int32)
    for k, top in _TOP.items():
        if U and m[k].max() > top:
            raise OverflowError(f'merge: {k} leaves its type (more than 65535 models, or a span_sum of 2^32)')
    for k, dt in COLUMNS[2:]:
        out[k] = m[k].astype(dt)
    return out


def mean_span(t):
    """Mean lifetime of every pair in models: ``span_sum / n_intervals`` as float64 [U]."""
    return t['span_sum'].astype(np.float64) / t['n_intervals'].astype(np.float64)


def occupancy(t, n_models_total):
    """Fraction of the ``n_models_total`` models in which every pair has a participating record: float64 [U]."""
    F = int(n_models_total)
    if F < 1:
        raise ValueError('occupancy: n_models_total must be at least 1')
    return t['n_models'].astype(np.float64) / F


def to_records(pc, t, n_models_total, component_types=None):
    """The table as a list of dicts for JSON: 'bgn' / 'end' label the two atoms as ``persistence.to_records`` does, the
    counts are plain ints, 'mean_span' and 'occupancy' are floats."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    mean, occ = mean_span(t), occupancy(t, n_models_total)
    out = []
    for r in range(len(t['a'])):
        out.append({'bgn': lab.atom_dict(int(t['a'][r])), 'end': lab.atom_dict(int(t['b'][r])), 'type': 'atom-atom',
                    'n_models': int(t['n_models'][r]), 'first_model': int(t['first'][r]), 'last_model': int(t['last'][r]),
                    'n_intervals': int(t['n_intervals'][r]), 'longest': int(t['longest'][r]),
                    'longest_start': int(t['longest_start'][r]), 'head': int(t['head'][r]), 'tail': int(t['tail'][r]),
                    'span_sum': int(t['span_sum'][r]), 'mean_span': float(mean[r]), 'occupancy': float(occ[r])})
    return out


CSV_HEADER = ['atom_bgn', 'atom_end', 'n_models', 'first_model', 'last_model', 'n_intervals', 'longest', 'longest_start', 'head',
              'tail', 'span_sum', 'mean_span', 'occupancy']


def write_csv(path, t, pc, n_models_total, component_types=None):
    """One row per pair: the atoms in the form the other CSV tables use ('A/508/O'), the nine integer columns, the mean span
    and the occupancy (the shortest text that gives the float64 back)."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    mean, occ = mean_span(t), occupancy(t, n_models_total)
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r in range(len(t['a'])):
            w.writerow([lab.atom_macro(int(t['a'][r])), lab.atom_macro(int(t['b'][r]))] + [int(t[k][r]) for k, _ in COLUMNS[2:]] +
                       [repr(float(mean[r])), repr(float(occ[r]))])


def write_lifetimes(wd, sid, t, pc, n_models_total, component_types=None):
    """'<id>.lifetimes' in ``wd``."""
    path = os.path.join(wd, sid + '.lifetimes')
    write_csv(path, t, pc, n_models_total, component_types)
    return path
