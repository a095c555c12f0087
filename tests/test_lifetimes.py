"""Contact lifetimes over the models of an ensemble, reduced on the device (arp_models_lifetimes_launch / _fetch,
Context.models_lifetimes, EnsembleComplex.run_lifetimes, arpeggio_amd.lifetimes).

The yardstick is never the device reduction: it is ``reference_lifetimes`` below — one plain loop over per-model bags that did
not come through the new code (the oracle's, or the bags ``run_models`` fetches and cuts), itself held against hand-written
rows and against ``_direct``, the definition applied to one pair's list of models.  Every comparison is exact: integers only."""
import copy
import csv
import ctypes as C
import functools
import json

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, contact_filter, lifetimes, persistence, similarity, synth, tables
from arpeggio_amd.core import config
from test_models import CASES, _same, _selectors
from test_persistence import _aa, _bag, _ctx_with_models, _hub, _mask, _oracle_bags, _random_bags, reference_table

ALL = (contact_filter.SIFT_ALL, contact_filter.CTYPE_ALL)
BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
HBOND = BIT['hbond']
INTER = 1 << config.CONTACT_TYPE_NAMES.index('INTER')
PARAMS = ((5.0, 0.1, False), (4.0, 0.25, True))
# the derived columns in the order of a hand-written row
DERIVED = ('n_models', 'first', 'last', 'n_intervals', 'longest', 'longest_start', 'head', 'tail', 'span_sum')


def reference_lifetimes(per_model_bags, n, gap, sift_any, ctype_mask):
    """The lifetimes table of per-model atom-atom bags (model-local ids, i < j, a pair at most once per model): one loop over
    the models in ascending order with, per row, the interval that is open — its first model and the last model seen.  A row
    met again beyond ``gap + 1`` models closes its interval and opens another; the end of the loop closes every row's last."""
    kept = []
    for b in per_model_bags:
        assert np.all(b['i'] < b['j'])
        take = ((b['sift'].astype(np.int64) & int(sift_any)) != 0) & (((int(ctype_mask) >> b['ctype'].astype(np.int64)) & 1) != 0)
        kept.append((b['i'].astype(np.int64) * n + b['j'].astype(np.int64))[take])
    uk = np.unique(np.concatenate(kept)) if kept else np.zeros(0, np.int64)
    U = len(uk)
    z = lambda: np.zeros(U, np.int64)
    nm, first, last, start, n_int, longest, lstart, head, ssum = z(), z(), z(), z(), z(), z(), z(), z(), z()

    def close(rows):
        span = last[rows] - start[rows] + 1
        head[rows] = np.where(n_int[rows] == 0, span, head[rows])
        n_int[rows] += 1
        ssum[rows] += span
        better = span > longest[rows]          # strictly: on a tie the earlier interval stays
        lstart[rows] = np.where(better, start[rows], lstart[rows])
        longest[rows] = np.where(better, span, longest[rows])
        return span

    for f, keys in enumerate(kept):
        idx = np.searchsorted(uk, keys)
        assert len(np.unique(idx)) == len(idx), 'a pair twice in one model'
        seen = nm[idx] > 0
        broken = seen & (f - last[idx] > gap + 1)
        close(idx[broken])
        start[idx[~seen | broken]] = f
        first[idx[~seen]] = f
        last[idx] = f
        nm[idx] += 1
    tail = close(np.arange(U))
    assert max(nm.max(initial=0), longest.max(initial=0)) <= 65535
    cols = dict(a=uk // n, b=uk % n, n_models=nm, first=first, last=last, n_intervals=n_int, longest=longest, longest_start=lstart,
                head=head, tail=tail, span_sum=ssum)
    return {k: cols[k].astype(dt) for k, dt in lifetimes.COLUMNS}


def _direct(models, gap):
    """The definition on one pair's ascending list of models: the nine derived columns as a tuple (``DERIVED``)."""
    iv = [[models[0], models[0]]]
    for f in models[1:]:
        if f - iv[-1][1] <= gap + 1:
            iv[-1][1] = f
        else:
            iv.append([f, f])
    spans = [e - s + 1 for s, e in iv]
    best = max(spans)
    return (len(models), models[0], models[-1], len(iv), best, iv[spans.index(best)][0], spans[0], spans[-1], sum(spans))


def _rows(t):
    return [tuple(int(t[k][r]) for k in DERIVED) for r in range(len(t['a']))]


def _pairs(t):
    return list(zip(t['a'].tolist(), t['b'].tolist()))


def _pattern_bags(patterns, F, n):
    """One pair per pattern (a set of models), the pairs in ascending (a, b) as the patterns come; all-records SIFt / type."""
    iu, ju = np.triu_indices(n, 1)
    assert len(patterns) <= len(iu)
    bags = []
    for f in range(F):
        rows = [p for p, models in enumerate(patterns) if f in models]
        bags.append(_bag(iu[rows], ju[rows], [3.0] * len(rows), [BIT['proximal']] * len(rows), [2] * len(rows)))
    return bags


# ------------------------------------------------------------------------------------------------------------- CPU
def test_reference_lifetimes_on_hand_made_bags():
    """Eleven models over 6 atoms.  (0, 1) in {0, 1, 3, 6, 10}: differences 1, 2, 3, 4, so gap g bridges the difference g + 1
    and splits at g + 2 for g = 0, 1, 2.  (0, 2) in {0, 1, 4, 5}: two longest intervals.  (1, 4) in model 7 only.  (2, 3) in
    every model, hbond in 0 ... 4 and vdw after, contact type 0 in even and 1 in odd models.  (3, 5) in {2, 3, 6, 7, 9}: a tie
    whose earliest start is not the first model of the table, and a longest interval that is the last one at gap 1."""
    H, V, P = BIT['hbond'], BIT['vdw'], BIT['proximal']
    present = {(0, 1): {0, 1, 3, 6, 10}, (0, 2): {0, 1, 4, 5}, (1, 4): {7}, (2, 3): set(range(11)), (3, 5): {2, 3, 6, 7, 9}}
    bags = []
    for f in range(11):
        rec = [(a, b) for (a, b), m in present.items() if f in m]
        sift = {(0, 1): P, (0, 2): H | P, (1, 4): V, (2, 3): H if f < 5 else V, (3, 5): P}
        ctype = {(0, 1): 2, (0, 2): 2, (1, 4): 2, (2, 3): f & 1, (3, 5): 2}
        bags.append(_bag([r[0] for r in rec], [r[1] for r in rec], [3.0] * len(rec), [sift[r] for r in rec], [ctype[r] for r in rec]))
    #        n_models, first, last, n_intervals, longest, longest_start, head, tail, span_sum
    want = {0: [(5, 0, 10, 4, 2, 0, 2, 1, 5), (4, 0, 5, 2, 2, 0, 2, 2, 4), (1, 7, 7, 1, 1, 7, 1, 1, 1), (11, 0, 10, 1, 11, 0, 11, 11, 11),
                (5, 2, 9, 3, 2, 2, 2, 1, 5)],
            1: [(5, 0, 10, 3, 4, 0, 4, 1, 6), (4, 0, 5, 2, 2, 0, 2, 2, 4), (1, 7, 7, 1, 1, 7, 1, 1, 1), (11, 0, 10, 1, 11, 0, 11, 11, 11),
                (5, 2, 9, 2, 4, 6, 2, 4, 6)],
            2: [(5, 0, 10, 2, 7, 0, 7, 1, 8), (4, 0, 5, 1, 6, 0, 6, 6, 6), (1, 7, 7, 1, 1, 7, 1, 1, 1), (11, 0, 10, 1, 11, 0, 11, 11, 11),
                (5, 2, 9, 1, 8, 2, 8, 8, 8)]}
    for gap in (0, 1, 2):
        t = reference_lifetimes(bags, 6, gap, *ALL)
        assert list(t) == [k for k, _ in lifetimes.COLUMNS] and all(t[k].dtype == dt for k, dt in lifetimes.COLUMNS)
        assert _pairs(t) == [(0, 1), (0, 2), (1, 4), (2, 3), (3, 5)]
        assert _rows(t) == want[gap], gap
        assert _rows(t) == [_direct(sorted(present[p]), gap) for p in _pairs(t)]
    # records removed by the SIFt mask: hbond only — (0, 2) as it was, (2, 3) in models 0 ... 4
    t = reference_lifetimes(bags, 6, 0, H, contact_filter.CTYPE_ALL)
    assert _pairs(t) == [(0, 2), (2, 3)] and _rows(t) == [(4, 0, 5, 2, 2, 0, 2, 2, 4), (5, 0, 4, 1, 5, 0, 5, 5, 5)]
    # ... and by the contact-type mask: type 1 only — (2, 3) in the odd models
    t = reference_lifetimes(bags, 6, 0, contact_filter.SIFT_ALL, 1 << 1)
    assert _pairs(t) == [(2, 3)] and _rows(t) == [(5, 1, 9, 5, 1, 1, 1, 1, 5)]
    t = reference_lifetimes(bags, 6, 1, contact_filter.SIFT_ALL, 1 << 1)
    assert _rows(t) == [(5, 1, 9, 1, 9, 1, 9, 9, 9)]
    # both at once, and a mask that no record meets
    t = reference_lifetimes(bags, 6, 0, H, 1 << 1)
    assert _pairs(t) == [(2, 3)] and _rows(t) == [(2, 1, 3, 2, 1, 1, 1, 1, 2)]
    _same(reference_lifetimes(bags, 6, 0, contact_filter.SIFT_ALL, 1 << 3), lifetimes.empty(), 'no record')
    _same(reference_lifetimes([], 6, 0, *ALL), lifetimes.empty(), 'no model')


def test_merge_equals_the_whole_for_every_pattern_over_nine_models():
    """Every non-empty presence pattern over 9 models (511, one pair each) x every boundary x gap 0, 1, 2: 12 264 cases.  The
    whole is also held against the definition applied to each pattern on its own."""
    F, n = 9, 33
    patterns = [{f for f in range(F) if (p >> f) & 1} for p in range(1, 1 << F)]
    bags = _pattern_bags(patterns, F, n)
    cases = 0
    for gap in (0, 1, 2):
        whole = reference_lifetimes(bags, n, gap, *ALL)
        assert len(whole['a']) == 511 and _rows(whole) == [_direct(sorted(m), gap) for m in patterns]
        for c in range(1, F):
            t1, t2 = reference_lifetimes(bags[:c], n, gap, *ALL), reference_lifetimes(bags[c:], n, gap, *ALL)
            _same(lifetimes.merge(t1, t2, c, gap), whole, (gap, c))
            cases += len(whole['a'])
    assert cases == 12264


def test_merge_of_random_chunks_equals_the_whole_at_every_boundary():
    rs = np.random.RandomState(11)
    F, n = 7, 30
    bags = _random_bags(rs, F, n, 60, empty=(3,))
    for gap in (0, 1, 2):
        whole = reference_lifetimes(bags, n, gap, *ALL)
        assert len(whole['a']) > 50 and whole['n_intervals'].max() > 1
        for c in range(1, F):
            m = lifetimes.merge(reference_lifetimes(bags[:c], n, gap, *ALL), reference_lifetimes(bags[c:], n, gap, *ALL), c, gap)
            assert list(m) == [k for k, _ in lifetimes.COLUMNS]
            _same(m, whole, (gap, c))
        # three chunks, left to right
        ref = lambda lo, hi: reference_lifetimes(bags[lo:hi], n, gap, *ALL)
        _same(lifetimes.merge(lifetimes.merge(ref(0, 2), ref(2, 5), 2, gap), ref(5, F), 5, gap), whole, (gap, 'three'))
        # an empty table on either side
        for m in (lifetimes.merge(lifetimes.empty(), whole, 0, gap), lifetimes.merge(whole, lifetimes.empty(), F, gap)):
            _same(m, whole, 'empty side')
    # with masks: the chunks and the whole filtered alike
    whole = reference_lifetimes(bags, n, 1, 0x00F0, 0x0F)
    assert 0 < len(whole['a']) < len(reference_lifetimes(bags, n, 1, *ALL)['a'])
    _same(lifetimes.merge(reference_lifetimes(bags[:4], n, 1, 0x00F0, 0x0F), reference_lifetimes(bags[4:], n, 1, 0x00F0, 0x0F), 4, 1), whole, 'masks')
    # a value beyond its column's type, the order of the chunks, the arguments
    t = reference_lifetimes(bags[:1], n, 0, *ALL)
    U = len(t['a'])
    hi = dict(t, n_models=np.full(U, 40000, np.uint16))
    with pytest.raises(OverflowError):
        lifetimes.merge(hi, hi, 40000, 0)
    hs = dict(t, n_intervals=np.full(U, 40000, np.uint16))
    with pytest.raises(OverflowError):
        lifetimes.merge(hs, hs, 40000, 0)
    long1 = dict(t, last=np.full(U, 39999, np.int32), tail=np.full(U, 40000, np.uint16))
    with pytest.raises(OverflowError):      # the joined interval of 80 000 models
        lifetimes.merge(long1, dict(t, head=np.full(U, 40000, np.uint16)), 40000, 0)
    with pytest.raises(ValueError):         # t2 would begin inside t1
        lifetimes.merge(reference_lifetimes(bags[:3], n, 0, *ALL), reference_lifetimes(bags[:3], n, 0, *ALL), 1, 0)
    for bad in (-1, 65535):
        with pytest.raises(ValueError):
            lifetimes.merge(t, t, 1, bad)
    with pytest.raises(ValueError):
        lifetimes.merge(t, t, -1, 0)


def test_records_and_csv_on_a_small_case(tmp_path):
    pc = _hub()
    pc.ensure_labels()
    P = BIT['proximal']
    m0 = _bag([0, 2], [1, 5], [3.0, 4.0], [P, P], [2, 0])
    m1 = _bag([0], [1], [3.5], [P], [1])
    e = _bag([], [], [], [], [])
    t = reference_lifetimes([m0, m1, e, m1, m1], pc.n_atoms, 0, *ALL)      # (0, 1) in {0, 1, 3, 4}, (2, 5) in {0}
    assert _rows(t) == [(4, 0, 4, 2, 2, 0, 2, 2, 4), (1, 0, 0, 1, 1, 0, 1, 1, 1)]
    assert lifetimes.mean_span(t).tolist() == [2.0, 1.0] and lifetimes.mean_span(t).dtype == np.float64
    assert lifetimes.occupancy(t, 5).tolist() == [0.8, 0.2]
    with pytest.raises(ValueError):
        lifetimes.occupancy(t, 0)
    from arpeggio_amd.core import export
    lab = export.Labels(pc, pc.component_types)
    rec = lifetimes.to_records(pc, t, 5)
    assert len(rec) == 2 and rec[0]['bgn'] == lab.atom_dict(0) and rec[0]['end'] == lab.atom_dict(1) and rec[1]['end'] == lab.atom_dict(5)
    as_persistence = persistence.to_records(reference_table([m0, m1], pc.n_atoms), pc)      # the same atom labels
    assert [(r['bgn'], r['end']) for r in rec] == [(r['bgn'], r['end']) for r in as_persistence]
    assert [rec[0][k] for k in ('n_models', 'first_model', 'last_model', 'n_intervals', 'longest', 'longest_start', 'head', 'tail',
                                'span_sum', 'mean_span', 'occupancy')] == [4, 0, 4, 2, 2, 0, 2, 2, 4, 2.0, 0.8]
    assert rec[0]['type'] == 'atom-atom' and json.loads(json.dumps(rec)) == rec
    path = lifetimes.write_lifetimes(str(tmp_path), 'x1', t, pc, 5)
    assert path.endswith('x1.lifetimes')
    rows = list(csv.reader(open(path, newline='')))
    assert rows[0] == lifetimes.CSV_HEADER and len(rows) == 3
    assert rows[1] == [lab.atom_macro(0), lab.atom_macro(1), '4', '0', '4', '2', '2', '0', '2', '2', '4', '2.0', '0.8']
    assert rows[2][:2] == [lab.atom_macro(2), lab.atom_macro(5)] and rows[2][2:11] == ['1', '0', '0', '1', '1', '0', '1', '1', '1']


def test_columns_and_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert int(re.search(r'#define\s+ARP_LIFETIMES_MAX_GAP\s+(\d+)u', hdr).group(1)) == _capi.LIFETIMES_MAX_GAP == lifetimes.MAX_GAP == 65534
    args = re.search(r'int arp_models_lifetimes_fetch\(arp_ctx\* ctx, int64_t cap,(.*?), int64_t\* count\);', hdr, re.S).group(1)
    ctype = {np.int32: 'int32_t', np.uint16: 'uint16_t', np.uint32: 'uint32_t'}
    assert [' '.join(a.split()) for a in args.split(',')] == [f'{ctype[dt]}* {k}' for k, dt in tables.LIFETIMES.columns]
    assert lifetimes.COLUMNS is tables.LIFETIMES.columns and tables.LIFETIMES.width == {}
    assert all(s in _capi.SYMBOLS for s in ('arp_models_lifetimes_launch', 'arp_models_lifetimes_fetch', 'arp_models_lifetimes_info'))


# ------------------------------------------------------------------------------------------------------------- GPU
# the presence patterns of the eight switch atoms over F = 130 models (a run of 130 records is three wave steps of 64) and the
# rows they must give, written out by hand for gap 0, 1 and 2:
#    n_models, first, last, n_intervals, longest, longest_start, head, tail, span_sum
SEAM_F = 130
SEAMS = [
    # all models but 64: the hole falls between records 63 and 64 — the first lane of the second step is a head
    (set(range(130)) - {64}, {0: (129, 0, 129, 2, 65, 65, 64, 65, 129), 1: (129, 0, 129, 1, 130, 0, 130, 130, 130), 2: (129, 0, 129, 1, 130, 0, 130, 130, 130)}),
    # models 0 ... 63: exactly one full step
    (set(range(64)), {g: (64, 0, 63, 1, 64, 0, 64, 64, 64) for g in (0, 1, 2)}),
    # models 0 ... 64: one lane in the second step
    (set(range(65)), {g: (65, 0, 64, 1, 65, 0, 65, 65, 65) for g in (0, 1, 2)}),
    # the even models: 65 records — 65 intervals at gap 0 (64 of them end inside the first step), one of span 129 at gap 1
    (set(range(0, 130, 2)), {0: (65, 0, 128, 65, 1, 0, 1, 1, 65), 1: (65, 0, 128, 1, 129, 0, 129, 129, 129), 2: (65, 0, 128, 1, 129, 0, 129, 129, 129)}),
    # 3 ... 12 and 100 ... 109: two longest intervals, the earliest start
    (set(range(3, 13)) | set(range(100, 110)), {g: (20, 3, 109, 2, 10, 3, 10, 10, 20) for g in (0, 1, 2)}),
    # 0 ... 9, 20 ... 29, 40 ... 127, 129: records 20 ... 107 are the longest interval, across the step boundary at record 64
    (set(range(10)) | set(range(20, 30)) | set(range(40, 128)) | {129},
     {0: (109, 0, 129, 4, 88, 40, 10, 1, 109), 1: (109, 0, 129, 3, 90, 40, 10, 90, 110), 2: (109, 0, 129, 3, 90, 40, 10, 90, 110)}),
    # model 129 alone
    ({129}, {g: (1, 129, 129, 1, 1, 129, 1, 1, 1) for g in (0, 1, 2)}),
    # differences 2, 3, 4 after a difference of 1
    ({0, 1, 3, 6, 10}, {0: (5, 0, 10, 4, 2, 0, 2, 1, 5), 1: (5, 0, 10, 3, 4, 0, 4, 1, 6), 2: (5, 0, 10, 2, 7, 0, 7, 1, 8)}),
]


def test_the_hand_written_seam_rows_are_the_definitions():
    for models, rows in SEAMS:
        for gap, row in rows.items():
            assert _direct(sorted(models), gap) == row, (sorted(models)[:12], gap)


@functools.lru_cache(maxsize=None)
def _seam_input():
    """proteinlike40 with every model equal to model 0, and eight heavy switch atoms — pairwise farther apart than the cutoff,
    each with a contact — moved far away (x_max + 20 + 20 p A) in the models outside their pattern."""
    pc = _hub()
    pc.ensure_labels()
    F, cutoff = SEAM_F, 5.0
    oc = oracle.OracleComplex(pc)
    oc.make_selection(None)
    bag0 = oc.atom_contacts(cutoff, 0.1, False)
    deg = np.bincount(np.concatenate([bag0['i'], bag0['j']]), minlength=pc.n_atoms)
    x64 = pc.xyz.astype(np.float64)
    heavy = [a for a in range(pc.n_atoms) if pc.element[a] not in ('H', 'D') and deg[a] > 0]
    switch = []
    for a in heavy:
        if all(np.linalg.norm(x64[a] - x64[s]) > cutoff + 1.0 for s in switch):
            switch.append(a)
        if len(switch) == len(SEAMS):
            break
    assert len(switch) == len(SEAMS)
    xyz = np.repeat(pc.xyz[None].astype(np.float32), F, axis=0)
    h_xyz = np.repeat(pc.h_xyz[None].astype(np.float64), F, axis=0)
    x_max = float(x64[:, 0].max())
    for p, (a, (models, _)) in enumerate(zip(switch, SEAMS)):
        away = np.array([f not in models for f in range(F)])
        to = np.array([x_max + 20.0 + 20.0 * p, x64[a, 1], x64[a, 2]])
        xyz[away, a] = to.astype(np.float32)
        h_xyz[away, pc.h_off[a]:pc.h_off[a + 1]] += to - x64[a]
    return pc, xyz, h_xyz, switch, bag0


@pytest.mark.gpu
def test_seams_between_wave_steps_against_hand_computed_rows():
    pc, xyz, h_xyz, switch, bag0 = _seam_input()
    n, F = pc.n_atoms, SEAM_F
    x64 = pc.xyz.astype(np.float64)
    for p, a in enumerate(switch):
        assert pc.element[a] not in ('H', 'D')
        assert int((bag0['i'] == a).sum() + (bag0['j'] == a).sum()) >= 1
        assert all(np.linalg.norm(x64[a] - x64[b]) > 5.0 for b in switch[p + 1:])
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    per = _aa(ctx.run_models(5.0, 0.1, False))
    of_switch = {a: p for p, a in enumerate(switch)}
    for gap in (0, 1, 2):
        got = ctx.models_lifetimes(gap)
        _same(got, reference_lifetimes(per, n, gap, *ALL), ('reference', gap))
        rows = _rows(got)
        met = set()
        for r, (a, b) in enumerate(_pairs(got)):
            assert not (a in of_switch and b in of_switch)
            p = of_switch.get(a, of_switch.get(b))
            if p is None:
                assert rows[r] == (F, 0, F - 1, 1, F, 0, F, F, F), (gap, a, b)
            else:
                assert rows[r] == SEAMS[p][1][gap], (gap, p, a, b)
                met.add(p)
        assert met == set(range(len(SEAMS))) and len(rows) > 500
    ctx.close()


COMBOS = ((0, ALL[0], ALL[1], None, None), (2, ALL[0], ALL[1], None, None), (0, HBOND, ALL[1], ('hbond',), None),
          (2, ALL[0], INTER, None, ('INTER',)))


@pytest.mark.gpu
@pytest.mark.parametrize('name,make,F,jitter', CASES, ids=[c[0] for c in CASES])
def test_table_equals_the_reference_of_the_per_model_bags(name, make, F, jitter):
    """Through Context (the same pass as the fetched bags) and through EnsembleComplex (its own pass): the table equals
    ``reference_lifetimes`` of the bags ``run_models`` returns; whole structure at 5.0 A also of the ORACLE's per-model bags."""
    from arpeggio_amd.core import EnsembleComplex
    pc = make()
    pc.ensure_labels()
    n = pc.n_atoms
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=jitter)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    rows = split = 0
    for params in PARAMS:
        for sel in _selectors(pc):
            ctx.set_selection(np.tile(_mask(pc, sel), F))
            per = _aa(ctx.run_models(*params))
            for gap, sift_any, ctype_mask, contacts, entities in COMBOS:
                what = (name, params, tuple(sel), gap, sift_any, ctype_mask)
                want = reference_lifetimes(per, n, gap, sift_any, ctype_mask)
                got = ctx.models_lifetimes(gap, sift_any, ctype_mask)
                _same(got, want, what + ('context',))
                rows += len(want['a'])
                split += int((want['n_intervals'] > 1).sum())
                if (sift_any, ctype_mask) == ALL:
                    pt = ctx.models_persistence()
                    for k in ('a', 'b', 'n_models', 'first', 'last'):
                        assert got[k].tobytes() == pt[k].tobytes(), what + (k,)
                e = ens.run_lifetimes(sel, *params, gap=gap, contacts=contacts, interacting_entities=entities)
                _same(e, want, what + ('ensemble',))
                assert ens.lifetimes is e and ens.lifetimes_models == F and ens._results is None
                if F == 1:
                    for k in ('n_models', 'n_intervals', 'longest', 'head', 'tail', 'span_sum'):
                        assert np.all(got[k] == 1), what + (k,)
                    assert not got['first'].any() and not got['last'].any() and not got['longest_start'].any()
            if params == PARAMS[0] and not sel:
                obags = []
                for k in range(F):
                    oc = oracle.OracleComplex(ens.model_pack(k))
                    oc.make_selection(None)
                    obags.append(oc.atom_contacts(*params))
                for gap in (0, 2):
                    _same(ctx.models_lifetimes(gap), reference_lifetimes(obags, n, gap, *ALL), (name, 'oracle', gap))
    print(name, 'rows', rows, 'with more than one interval', split)
    assert rows > 0 and (F == 1 or split > 0)
    ctx.close()


@pytest.mark.gpu
def test_streamed_chunks_accumulate_exactly_to_the_table_of_the_whole(tmp_path):
    from arpeggio_amd.core import EnsembleComplex
    pc = _hub()
    n, gap = pc.n_atoms, 1
    xyz, h_xyz = synth.models_of(pc, 12, seed=9, jitter=0.3)
    one = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    one.run_arpeggio([], 5.0, 0.1, False)
    per = [one.model(k)._bags['atom_atom'] for k in range(12)]
    want = reference_lifetimes(per, n, gap, *ALL)
    assert want['n_intervals'].max() > 1 and int((want['span_sum'] > want['n_models']).sum()) > 0      # (bridged holes exist)
    _same(one.run_lifetimes([], 5.0, 0.1, False, gap=gap), want, 'whole')
    ens = EnsembleComplex((copy.copy(pc), xyz[:5], h_xyz[:5]))
    with pytest.raises(AttributeError):
        ens.write_lifetimes(str(tmp_path))
    for lo, hi in ((0, 5), (5, 9), (9, 12)):
        if lo:
            ens.set_coordinates(xyz[lo:hi], h_xyz[lo:hi])
        ens.run_lifetimes([], 5.0, 0.1, False, gap=gap, accumulate=True)
        assert ens.lifetimes_models == hi
    _same(ens.lifetimes, want, 'streamed')
    path = ens.write_lifetimes(str(tmp_path))
    assert path.endswith(pc.id + '.lifetimes') and len(open(path).read().splitlines()) == len(want['a']) + 1
    # another gap, other contacts or other entities between chunks are refused, and the accumulated table stays
    for kw in (dict(gap=2), dict(gap=gap, contacts=('hbond',)), dict(gap=gap, interacting_entities=('INTER',))):
        with pytest.raises(ValueError, match='accumulate'):
            ens.run_lifetimes([], 5.0, 0.1, False, accumulate=True, **kw)
    _same(ens.lifetimes, want, 'after the refusals')
    # accumulate=False starts over
    ens.run_lifetimes([], 5.0, 0.1, False, gap=2)
    assert ens.lifetimes_models == 3
    _same(ens.lifetimes, reference_lifetimes(per[9:], n, 2, *ALL), 'restart')


def _fetch(ctx, U):
    t = tables.alloc(tables.LIFETIMES, U, np.zeros)
    cnt = C.c_int64(-1)
    rc = ctx._L.arp_models_lifetimes_fetch(ctx._h, U, *(_capi._p(t[k]) for k, _ in tables.LIFETIMES.columns), C.byref(cnt))
    return rc, cnt.value, t


@pytest.mark.gpu
def test_refusals_and_empty_tables():
    pc = _hub()
    F = 6
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.run_launch(5.0, 0.1, False)
    with pytest.raises(ValueError, match='arp_models_lifetimes_launch: no models resident'):
        ctx.models_lifetimes()
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    with pytest.raises(ValueError, match='arp_models_lifetimes_launch: no results'):      # models resident, no pass yet
        ctx.models_lifetimes()
    assert _fetch(ctx, 0)[0] == _capi.ARP_E_ARG
    ctx.run_launch(5.0, 0.1, False)
    with pytest.raises(ValueError, match='arp_models_lifetimes_launch: gap'):
        ctx.models_lifetimes(65535)
    for bad in ((0, 0x7F), (0x7FFF, 0)):
        with pytest.raises(ValueError, match='arp_models_lifetimes_launch: a mask of 0'):
            ctx.models_lifetimes(0, *bad)
    for bad in ((0x8000, 0x7F), (0x7FFF, 0x80)):
        with pytest.raises(ValueError, match='arp_models_lifetimes_launch: a mask has bits beyond'):
            ctx.models_lifetimes(0, *bad)
    assert _fetch(ctx, 0)[0] == _capi.ARP_E_ARG      # nothing was made by the refused launches
    per = _aa(_capi.split_models(ctx.fetch_packed()[0], ctx._models))
    t = ctx.models_lifetimes(65534)                   # the largest gap: every pair one interval
    _same(t, reference_lifetimes(per, pc.n_atoms, 65534, *ALL), 'gap 65534')
    U = len(t['a'])
    assert U > 100 and np.all(t['n_intervals'] == 1)
    # cap too small: ARP_E_CAPACITY with the count; NULL columns are allowed
    cnt = C.c_int64(-1)
    a = np.full(U, -7, np.int32)
    L, h = ctx._L, ctx._h
    assert L.arp_models_lifetimes_fetch(h, U - 1, _capi._p(a), *([None] * 10), C.byref(cnt)) == _capi.ARP_E_CAPACITY
    assert cnt.value == U and np.all(a == -7)
    assert L.arp_models_lifetimes_fetch(h, U, _capi._p(a), *([None] * 10), C.byref(cnt)) == 0 and np.array_equal(a, t['a'])
    # a mask that no record meets: 0 rows and a fetch of 0
    met = np.zeros(15, bool)
    for b in per:
        met |= ((b['sift'][:, None] >> np.arange(15)) & 1).any(axis=0)
    unmet = [k for k in range(15) if not met[k]]
    assert unmet, 'every SIFt bit occurs: choose another case'
    t0 = ctx.models_lifetimes(0, 1 << unmet[0])
    _same(t0, lifetimes.empty(), 'no record takes part')
    assert ctx.stats()['lifetimes_rows'] == 0
    assert L.arp_models_lifetimes_fetch(h, 0, *([None] * 11), C.byref(cnt)) == 0 and cnt.value == 0
    ctx.close()
    # a shard
    c2 = _capi.Context(0)
    c2.set_complex(pc)
    c2.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    with pytest.raises(ValueError, match='arp_models_lifetimes_launch: not for a shard'):
        c2.models_lifetimes()
    c2.close()


@pytest.mark.gpu
def test_a_model_without_records_in_the_middle():
    """One water selected; in model 2 of 5 it is moved 50 A away from everything, so that model has no record at all: at gap 0
    a pair on both sides of it has two intervals, at gap 1 one that spans the hole."""
    from arpeggio_amd.core import EnsembleComplex
    pc = _hub()
    F = 5
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.1)
    waters = [r for r in range(pc.n_residues) if pc.res_name[r] == 'HOH']
    best, atoms = -1, None
    for w in waters:
        at = np.nonzero(pc.res_id == w)[0]
        sel = np.zeros(pc.n_atoms, np.uint8)
        sel[at] = 1
        k = min(len(b['i']) for b in _oracle_bags(pc, xyz, h_xyz, sel=sel))
        if k > best:
            best, atoms = k, at
    assert best > 0
    for a_ in atoms:
        xyz[2, a_] += np.float32(50.0)
        h_xyz[2, pc.h_off[a_]:pc.h_off[a_ + 1]] += 50.0
    sel = np.zeros(pc.n_atoms, np.uint8)
    sel[atoms] = 1
    obags = _oracle_bags(pc, xyz, h_xyz, sel=sel)
    assert len(obags[2]['i']) == 0 and all(len(obags[k]['i']) > 0 for k in (0, 1, 3, 4))
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    g0 = ens.run_lifetimes(atoms, 5.0, 0.1, False, gap=0)
    _same(g0, reference_lifetimes(obags, pc.n_atoms, 0, *ALL), 'gap 0')
    across = (g0['first'] < 2) & (g0['last'] > 2)
    assert across.any() and np.all(g0['n_intervals'][across] >= 2)
    g1 = ens.run_lifetimes(atoms, 5.0, 0.1, False, gap=1)
    _same(g1, reference_lifetimes(obags, pc.n_atoms, 1, *ALL), 'gap 1')
    both = (g0['n_models'] == 4)
    assert both.any() and np.all(g1['n_intervals'][both] == 1) and np.all(g1['longest'][both] == 5) and np.all(g1['span_sum'][both] == 5)


# what the derived results of test_derived_voiding read, with lifetimes beside them
def _others(ctx):
    planes = similarity.planes(None, ('atom_atom',))
    return dict(persist=lambda: ctx.models_persistence(), respair=lambda: ctx.residue_pairs(),
                respersist=lambda: ctx.models_residue_persistence(), filtered=lambda: ctx.contacts_filter(contact_filter.SPECIFIC[0], 0x7F),
                bridges=lambda: ctx.water_bridges(contact_filter.SPECIFIC[0]),
                bridgepersist=lambda: ctx.models_water_bridge_persistence(contact_filter.SPECIFIC[0]),
                similarity=lambda: ctx.models_similarity(planes))


@pytest.mark.gpu
def test_repeated_launches_and_what_voids_the_table():
    pc = _hub()
    pc.ensure_labels()
    F = 3
    xyz, h_xyz = synth.models_of(pc, F, seed=4)
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    ctx.run_launch(5.0, 0.1, False)
    launches = lambda: ctx.stats()['lifetimes_launches']
    assert launches() == 0 and ctx.stats()['lifetimes_rows'] == 0
    t = ctx.models_lifetimes(1, HBOND | BIT['polar'], 0x7F)
    U = len(t['a'])
    assert U > 0 and launches() == 1 and ctx.stats()['lifetimes_rows'] == U
    # equal arguments: the resident table; any other argument: another one
    _same(ctx.models_lifetimes(1, HBOND | BIT['polar'], 0x7F), t, 'again')
    assert launches() == 1
    for k, args in enumerate(((2, HBOND | BIT['polar'], 0x7F), (1, HBOND, 0x7F), (1, HBOND | BIT['polar'], 0x3F), (1, HBOND | BIT['polar'], 0x7F))):
        ctx.models_lifetimes(*args)
        assert launches() == 2 + k, args
    _same(ctx.models_lifetimes(1, HBOND | BIT['polar'], 0x7F), t, 'the first arguments once more')
    before = _fetch(ctx, U)
    assert before[0] == _capi.ARP_OK and before[1] == U
    _same(before[2], t, 'fetch')
    made = launches()

    def same(what):
        rc, cnt, got = _fetch(ctx, U)
        assert rc == _capi.ARP_OK and cnt == U and launches() == made, what
        _same(got, t, what)

    # events that leave it alone: the packed layout, a plane bag alone, the making of any other derived result
    ctx.set_packed_layout(True)
    same('packed layout')
    ctx.set_packed_layout(False)
    ctx.launch_bag('plane_plane')
    same('plane bag')
    ctx.run_launch(5.0, 0.1, False)
    t = ctx.models_lifetimes(1, HBOND | BIT['polar'], 0x7F)
    made = launches()
    for name, make in _others(ctx).items():
        make()
        same(name)
    # ... and it voids none of them: each is still the resident one (a fetch through ctypes returns ARP_OK)
    assert ctx._L.arp_models_persistence_fetch(ctx._h, 1 << 30, *([None] * 10), C.byref(C.c_int64())) == _capi.ARP_OK
    inter = np.zeros((F, F), np.uint32)
    assert ctx._L.arp_models_similarity_fetch(ctx._h, F, _capi._p(inter), C.byref(C.c_int64())) == _capi.ARP_OK

    # events that void it: the fetch returns ARP_E_ARG, and the next launch makes it anew
    def voided(what, event):
        assert _fetch(ctx, U)[0] == _capi.ARP_OK, what
        event()
        assert _fetch(ctx, U)[0] == _capi.ARP_E_ARG, what
        assert ctx.stats()['lifetimes_rows'] == 0, what

    def remade(what):
        nonlocal made
        _same(ctx.models_lifetimes(1, HBOND | BIT['polar'], 0x7F), t, what)
        made += 1
        assert launches() == made, what

    voided('a new pass', lambda: ctx.run_launch(5.0, 0.1, False))
    remade('a new pass')
    voided('a new selection', lambda: ctx.set_selection(np.ones(ctx.n, np.uint8)))
    with pytest.raises(ValueError, match='no results'):
        ctx.models_lifetimes(1, HBOND | BIT['polar'], 0x7F)
    ctx.run_launch(5.0, 0.1, False)
    remade('a new selection followed by a pass')
    voided('the atom-atom bag alone', lambda: ctx.atom_contacts_launch(5.0, 0.1, False))
    remade('the atom-atom bag alone')
    voided('a models upload', lambda: ctx.set_models(xyz, h_xyz))
    ctx.run_launch(5.0, 0.1, False)
    remade('a models upload followed by a pass')
    ctx.close()
