"""The seven results reduced over the resident models of an ensemble, run at the top of their model ranges: F = 65535 for
the tables that count models in uint16 (contact, residue and water-bridge persistence, lifetimes) and F = 2048, 2049, 4095,
4096 for coupling and similarity (ARP_SIM_MAX_MODELS = 4096: the second panel of model words, 64 x 64 tiles of models, the
criterion at the integers its 64-bit argument is about, the 64 MiB fetch).  The structures are tiny — isolated atom pairs on a
20 A lattice, one water with four partners — only F is large.

The yardstick is never the device.  Every expected value comes from the planted presence matrix: with Python integers, with
the yardsticks of the tests of each result (``test_coupling.reference_tables`` / ``kept``, ``test_similarity.model_features``,
``bridge_persistence.fold`` on ``test_water_bridges._join``), or — where those loop over the models in Python and F = 65535
would take them minutes — with the vectorised twins below, which work on the fetched resident ids (f = i // n) and are held on
the CPU against the looping ones on small random cases.  In every case the records the pass itself found are asserted equal
to the planted ones first, so a wrong pass over F models is not mistaken for a wrong reduction.  Every comparison is exact:
integers equal, floats as bytes.  No tolerance anywhere, and no time is asserted."""
import math

import numpy as np
import pytest

import test_bridge_persistence as t_bridge
import test_residue_pairs as t_respairs
import test_residue_persistence as t_respersist
from arpeggio_amd import _capi, bridge_persistence as bp, lifetimes
from arpeggio_amd.core import config
from helpers import tiny_complex
from test_coupling import ALL16, ALL20, ANY, PASS, _field_case, _vectors, check, kept, reference_tables
from test_lifetimes import ALL as EVERY_RECORD, _direct, _rows, reference_lifetimes
from test_models import _same
from test_persistence import _ctx_with_models, _random_bags, reference_table
from test_similarity import inter_of, model_features
from test_water_bridges import ALL as SIFT_ALL, _join

F_TOP = 65535                       # the most models the uint16 columns count
TINY, LATE = 3 * 2.0 ** -40, 4.75   # the two separations of the dist_sum rows (both exact in float32, as is their square)
NEAR, AWAY = 3.5, 9.0               # a pair inside / outside the 5 A of the pass
LEG, LEG_AWAY = 4.0, 9.0            # a partner of the water inside / outside
PARTNER_AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float64)      # at 4 A: 5.66 A or 8 A from one another
GAPS = (0, 1, 65532, 65533, 65534)


# ---------------------------------------------------------------------------------------------------- the structures
def _range_field(sep, partners=None):
    """``test_coupling._dimer_field`` with a separation per pair and model, and a water.  ``sep`` float [F, R]: pair r — atoms
    2 r, 2 r + 1, a residue an atom — is sep[f, r] A apart in model f.  The sites lie on a 20 A lattice in the plane x = 0 and
    the pairs point along x, so the x coordinates of a pair are 0 and its separation: float32 holds 3 * 2^-40 exactly.
    ``partners`` bool [F, K <= 4]: on one more site the water 2 R, and partner k — atom 2 R + 1 + k — 4 A from it along its own
    axis in the models where its bit is set and 9 A otherwise.  Returns (pc, xyz [F, n, 3])."""
    sep = np.asarray(sep, np.float64)
    F, R = sep.shape
    K = 0 if partners is None else partners.shape[1]
    sites = R + (1 if K else 0)
    side = max(1, math.ceil(math.sqrt(sites) - 1e-9))
    s = np.arange(sites)
    site = 20.0 * np.stack([0 * s, s % side, s // side], axis=1)
    n = 2 * R + (1 + K if K else 0)
    xyz = np.zeros((F, n, 3), np.float32)
    xyz[:, 0:2 * R:2] = site[None, :R]
    xyz[:, 1:2 * R:2] = site[None, :R]
    xyz[:, 1:2 * R:2, 0] += sep
    flags = np.zeros(n, np.uint16)
    if K:
        xyz[:, 2 * R:] = site[R]
        for k in range(K):
            xyz[:, 2 * R + 1 + k] += (np.where(partners[:, k], LEG, LEG_AWAY)[:, None] * PARTNER_AXES[k][None]).astype(np.float32)
        flags[2 * R] = config.F_WATER
    return tiny_complex(xyz[0], flags=flags), np.ascontiguousarray(xyz)


def _planted_records(sep, partners=None):
    """The records a pass at 5 A must find in the field, in the canonical order of the resident bag: (f, a, b, dist)."""
    sep = np.asarray(sep, np.float64)
    F, R = sep.shape
    f, r = np.nonzero(sep <= 5.0)
    parts = [(f, 2 * r, 2 * r + 1, sep[f, r])]
    if partners is not None:
        f, k = np.nonzero(partners)
        parts.append((f, np.full(len(f), 2 * R), 2 * R + 1 + k, np.full(len(f), LEG)))
    f, a, b, d = (np.concatenate([p[q] for p in parts]) for q in range(4))
    order = np.lexsort((b, a, f))
    return f[order].astype(np.int64), a[order].astype(np.int64), b[order].astype(np.int64), d[order].astype(np.float32)


def _planted_bag(sep, partners, n, rs=None):
    """The resident atom-atom bag of the planted records (resident ids f n + a), for the CPU tests: SIFt and contact type
    fixed per row, or random per record with ``rs``."""
    f, a, b, d = _planted_records(sep, partners)
    k = len(f)
    sift = np.full(k, 1 << 4, np.uint16) if rs is None else rs.randint(1, 1 << 15, k).astype(np.uint16)
    ctype = np.full(k, 2, np.uint8) if rs is None else rs.randint(0, 7, k).astype(np.uint8)
    return dict(i=(f * n + a).astype(np.int32), j=(f * n + b).astype(np.int32), dist=d, sift=sift, ctype=ctype)


def _top_plan(F=F_TOP):
    """The planted rows of the uint16 tables over F models (the CPU tests run the same plan at a small F).  Pairs: 0 in every
    model; 1 in the first and the last model; 2 in every second model; 3 in the last model; 4 and 5 in every model, the
    separation 3 * 2^-40 A in the models below F // 2 and 4.75 A from there on (4), and the halves the other way round (5).
    The water's partners: 0 and 1 in every model, 2 in the first and the last, 3 in the last — so the bridge (0, 1) is in every
    model, (0, 2) and (1, 2) in the first and the last, and (0, 3), (1, 3), (2, 3) in the last only."""
    f = np.arange(F)
    ends = (f == 0) | (f == F - 1)
    sep = np.full((F, 6), AWAY)
    sep[:, 0] = NEAR
    sep[ends, 1] = NEAR
    sep[f % 2 == 0, 2] = NEAR
    sep[F - 1, 3] = NEAR
    sep[:, 4] = np.where(f < F // 2, TINY, LATE)
    sep[:, 5] = np.where(f < F // 2, LATE, TINY)
    partners = np.stack([f >= 0, f >= 0, ends, f == F - 1], axis=1)
    return sep, partners


def _ascending(values):
    s = 0.0
    for v in values:
        s += float(v)
    return s


# ----------------------------------------------------------------------------------- the vectorised yardsticks
def _cut(aa, n):
    """The model and the two topology ids of every record of a resident bag."""
    i, j = np.asarray(aa['i']).astype(np.int64), np.asarray(aa['j']).astype(np.int64)
    f = i // n
    assert np.array_equal(j // n, f), 'a record across two models'
    return f, i - f * n, j - f * n


def _segments(sorted_keys):
    """(start of every run of equal keys, its length, the run of every element)."""
    head = np.ones(len(sorted_keys), bool)
    head[1:] = sorted_keys[1:] != sorted_keys[:-1]
    start = np.nonzero(head)[0]
    return start, np.diff(np.concatenate([start, [len(sorted_keys)]])), np.cumsum(head) - 1


def fast_persistence(aa, n):
    """``test_persistence.reference_table`` without the loop over the models: the records sorted by (row, model), every column
    a reduction over the runs, and dist_sum ONE np.add.at over the sorted records — unbuffered, so a row's distances are
    added one by one in ascending model order, the order the table's contract fixes."""
    f, a, b = _cut(aa, n)
    assert (a < b).all()
    key = a * n + b
    order = np.lexsort((f, key))
    key, f = key[order], f[order]
    assert not ((key[1:] == key[:-1]) & (f[1:] == f[:-1])).any(), 'a pair twice in one model'
    start, nm, row = _segments(key)
    U = len(start)
    assert nm.max(initial=0) <= 65535
    d = np.asarray(aa['dist'], np.float32)[order]
    sift = np.asarray(aa['sift']).astype(np.int64)[order]
    types = (1 << np.asarray(aa['ctype']).astype(np.int64))[order]
    acc = np.zeros(U, np.float64)
    np.add.at(acc, row, d.astype(np.float64))
    red = lambda op, x: op.reduceat(x, start) if U else x[:0]
    uk = key[start]
    return dict(a=(uk // n).astype(np.int32), b=(uk % n).astype(np.int32), n_models=nm.astype(np.uint16), first=f[start].astype(np.int32),
                last=f[start + nm - 1].astype(np.int32), dist_min=red(np.minimum, d), dist_max=red(np.maximum, d), dist_sum=acc,
                bit_count=red(np.add, (sift[:, None] >> np.arange(15)) & 1).astype(np.uint16).reshape(U, 15), ctype_mask=red(np.bitwise_or, types).astype(np.uint8))


def fast_residue_persistence(aa, n, res_id, F):
    """``test_residue_persistence.reference_table`` of ``test_residue_pairs.reference_table`` of every model, for a pass whose
    ring / amide bags are empty, without the loop over the models: the records sorted by (residue pair, model); a (pair, model)
    group is what one model adds to a row — its records, their smallest distance, the OR of their SIFt bits —; dist_sum is one
    np.add.at over the groups in ascending (pair, model)."""
    f, a, b = _cut(aa, n)
    res = np.asarray(res_id).astype(np.int64)
    ra, rb = res[a], res[b]
    assert (ra >= 0).all() and (rb >= 0).all()
    stride = int(res.max()) + 1
    gkey = (np.minimum(ra, rb) * stride + np.maximum(ra, rb)) * F + f
    order = np.argsort(gkey, kind='stable')
    gkey = gkey[order]
    gstart, gcount, _ = _segments(gkey)
    d = np.asarray(aa['dist'], np.float32)[order]
    sift = np.asarray(aa['sift']).astype(np.int64)[order] & 0x7FFF
    types = (1 << np.asarray(aa['ctype']).astype(np.int64))[order]
    G = len(gstart)
    red = lambda op, x, at: op.reduceat(x, at) if len(at) else x[:0]
    gmin, gbits, gtypes = red(np.minimum, d, gstart), red(np.bitwise_or, sift, gstart), red(np.bitwise_or, types, gstart)
    gpair, gf = gkey[gstart] // F, gkey[gstart] % F
    start, nm, row = _segments(gpair)
    U = len(start)
    assert nm.max(initial=0) <= 65535 and G == nm.sum()
    acc = np.zeros(U, np.float64)
    np.add.at(acc, row, gmin.astype(np.float64))
    cls = np.zeros((U, 5), np.uint16)
    cls[:, 0] = nm      # (every group has an atom-atom record; no ring / amide classes)
    up = gpair[start]
    return dict(res_a=(up // stride).astype(np.int32), res_b=(up % stride).astype(np.int32), n_models=nm.astype(np.uint16),
                first=gf[start].astype(np.int32), last=gf[start + nm - 1].astype(np.int32), n_contacts=red(np.add, gcount, start).astype(np.uint32),
                class_models=cls, bit_models=red(np.add, (gbits[:, None] >> np.arange(15)) & 1, start).astype(np.uint16).reshape(U, 15),
                dist_min=red(np.minimum, gmin, start), dist_max=red(np.maximum, gmin, start), dist_sum=acc,
                ctype_mask=red(np.bitwise_or, gtypes, start).astype(np.uint8))


def fast_lifetimes(aa, n, gap, sift_any=EVERY_RECORD[0], ctype_mask=EVERY_RECORD[1]):
    """``test_lifetimes.reference_lifetimes`` without the loop over the models: the participating records sorted by (row,
    model); an interval begins at a row's first record and at every record more than gap + 1 models after its predecessor."""
    f, a, b = _cut(aa, n)
    take = ((np.asarray(aa['sift']).astype(np.int64) & int(sift_any)) != 0) & (((int(ctype_mask) >> np.asarray(aa['ctype']).astype(np.int64)) & 1) != 0)
    key, f = (a * n + b)[take], f[take]
    order = np.lexsort((f, key))
    if not len(key):
        return lifetimes.empty()
    key, f = key[order], f[order]
    start, nm, row = _segments(key)
    U = len(start)
    opens = np.concatenate([[True], (key[1:] != key[:-1]) | (f[1:] - f[:-1] > gap + 1)])
    iv = np.nonzero(opens)[0]                                   # the first record of every interval
    iv_end = np.concatenate([iv[1:], [len(key)]]) - 1
    span, iv_from, iv_row = f[iv_end] - f[iv] + 1, f[iv], row[iv]
    istart, n_int, _ = _segments(iv_row)
    red = lambda op, x: op.reduceat(x, istart) if U else x[:0]
    longest = red(np.maximum, span)
    lstart = red(np.minimum, np.where(span == longest[iv_row], iv_from, np.iinfo(np.int64).max))      # on a tie the earliest
    uk = key[start]
    cols = dict(a=uk // n, b=uk % n, n_models=nm, first=f[start], last=f[start + nm - 1], n_intervals=n_int, longest=longest, longest_start=lstart,
                head=span[istart], tail=span[istart + n_int - 1], span_sum=red(np.add, span))
    assert max(nm.max(initial=0), longest.max(initial=0), n_int.max(initial=0)) <= 65535
    return {k: cols[k].astype(dt) for k, dt in lifetimes.COLUMNS}


def bridge_tables(aa, pc, F, same=False):
    """The water-bridge persistence tables of a resident bag at both levels: ``test_water_bridges._join`` on the whole bag (a
    water's partners lie in its model) and ``bridge_persistence.fold``, the NumPy twin that ``test_bridge_persistence`` holds
    against its loops — as does ``test_the_vectorised_yardsticks_equal_the_looping_ones`` here."""
    joined = _join(aa, np.tile(pc.flags, F), np.tile(pc.res_id, F), SIFT_ALL, same)
    return joined, {'atom': bp.fold(joined, pc.n_atoms), 'residue': bp.fold(joined, pc.n_atoms, pc.res_id)}


def fast_inter(features):
    """``test_similarity.inter_of`` without the F^2 loop: the features as a 0 / 1 matrix [F, all features] and its product with
    its transpose — in float32, exact while the counts stay below 2^24."""
    every = np.unique(np.concatenate(features)) if features else np.zeros(0, np.int64)
    assert len(every) < 1 << 24
    B = np.zeros((len(features), len(every)), np.float32)
    for f, x in enumerate(features):
        B[f, np.searchsorted(every, x)] = 1
    return (B @ B.T).astype(np.uint32)


def _per_model(aa, n, F):
    """A resident bag as per-model bags with model-local ids (for the looping yardsticks)."""
    f, a, b = _cut(aa, n)
    assert (np.diff(f) >= 0).all()
    cuts = np.searchsorted(f, np.arange(1, F))
    cols = dict(i=a.astype(np.int32), j=b.astype(np.int32), **{k: np.asarray(aa[k]) for k in ('dist', 'sift', 'ctype')})
    parts = {k: np.split(v, cuts) for k, v in cols.items()}
    return [{k: parts[k][m] for k in parts} for m in range(F)]


def _resident(bags, n):
    """Per-model bags as the one resident bag (ids f n + a)."""
    out = {k: np.concatenate([np.asarray(b[k]) for b in bags]) for k in ('dist', 'sift', 'ctype')}
    out['i'] = np.concatenate([b['i'].astype(np.int64) + f * n for f, b in enumerate(bags)]).astype(np.int32)
    out['j'] = np.concatenate([b['j'].astype(np.int64) + f * n for f, b in enumerate(bags)]).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------------------- CPU
def test_the_two_dist_sum_rows_depend_on_the_order_of_addition():
    """Row (a), pair 4: 32767 distances of 3 * 2^-40 A, then 32768 of 4.75 A.  Added in ascending model order the small ones
    are summed first and survive; in descending order each is below half an ulp of the running sum and is lost.  Row (b), pair
    5, the halves swapped: one by one in ascending order every small term is lost, while a reduction that first adds 64 of
    them together keeps them."""
    sep, _ = _top_plan()
    a, b = sep[:, 4].astype(np.float32), sep[:, 5].astype(np.float32)
    assert a[:32767].tolist() == [TINY] * 32767 and a[32767:].tolist() == [LATE] * 32768
    assert b[:32767].tolist() == [LATE] * 32767 and b[32767:].tolist() == [TINY] * 32768
    assert _ascending(a) == float.fromhex('0x1.3000000000c00p+17') and _ascending(a[::-1]) == float.fromhex('0x1.3p+17')
    assert _ascending(a) != _ascending(a[::-1])
    by64 = _ascending([_ascending(b[k:k + 64]) for k in range(0, F_TOP, 64)])
    assert _ascending(b) == 32767 * LATE and by64 == 32767 * LATE + 32768 * TINY
    assert _ascending(b) != by64
    # np.add.at is the one-by-one order
    for v in (a, b):
        acc = np.zeros(1)
        np.add.at(acc, np.zeros(F_TOP, np.int64), v.astype(np.float64))
        assert acc[0] == _ascending(v)


def test_the_vectorised_yardsticks_equal_the_looping_ones():
    """Random bags over F = 7, 64 and 130 models — float32 distances whose float64 sum depends on the order —, several atoms
    per residue: the four vectorised tables equal the looping references of the tests of each result, byte for byte."""
    rs = np.random.RandomState(5)
    n = 30
    res_id = np.sort(rs.randint(0, 9, n)).astype(np.int32)
    for F in (7, 64, 130):
        bags = _random_bags(rs, F, n, 60, empty=(3,))
        aa = _resident(bags, n)
        for f, (g, w) in enumerate(zip(_per_model(aa, n, F), bags)):
            _same(g, w, ('round trip', f))
        _same(fast_persistence(aa, n), reference_table(bags, n), ('persistence', F))
        none = np.zeros(0, np.int32)
        want = t_respersist.reference_table([t_respairs.reference_table({'atom_atom': b}, res_id, none, none) for b in bags])
        _same(fast_residue_persistence(aa, n, res_id, F), want, ('residue persistence', F))
        for gap in (0, 1, 2, F - 3, F - 2, F - 1):
            _same(fast_lifetimes(aa, n, gap), reference_lifetimes(bags, n, gap, *EVERY_RECORD), ('lifetimes', F, gap))
        _same(fast_lifetimes(aa, n, 1, 0x00F0, 0x0F), reference_lifetimes(bags, n, 1, 0x00F0, 0x0F), ('lifetimes, masks', F))
    empty = {k: np.zeros(0, dt) for k, dt in (('i', np.int32), ('j', np.int32), ('dist', np.float32), ('sift', np.uint16), ('ctype', np.uint8))}
    _same(fast_persistence(empty, n), reference_table([], n), 'no record')
    _same(fast_lifetimes(empty, n, 0), lifetimes.empty(), 'no record')
    # the planted field itself at F = 129, random SIFt and types: all four tables, the bridges against the loops
    F = 129
    sep, partners = _top_plan(F)
    pc, xyz = _range_field(sep[:1], partners[:1])
    n = pc.n_atoms
    aa = _planted_bag(sep, partners, n, rs)
    bags = _per_model(aa, n, F)
    _same(fast_persistence(aa, n), reference_table(bags, n), 'field')
    none = np.zeros(0, np.int32)
    _same(fast_residue_persistence(aa, n, pc.res_id, F), t_respersist.reference_table([t_respairs.reference_table({'atom_atom': b}, pc.res_id, none, none) for b in bags]),
          'field, residues')
    per = [_join(b, pc.flags, pc.res_id, SIFT_ALL) for b in bags]
    joined, got = bridge_tables(aa, pc, F)
    assert len(joined['water']) == sum(len(t['water']) for t in per) == F + 2 + 5      # one in every model, two more in the first, five in the last
    t_bridge._same(got['atom'], t_bridge.loop_fold(per), 'bridges')
    t_bridge._same(got['residue'], t_bridge.loop_fold(per, pc.res_id), 'bridges, residues')
    # the shared-feature matrix
    feats = [model_features({'atom_atom': b}, ALL16, 0x7F, n) for b in bags]
    assert np.array_equal(fast_inter(feats), inter_of(feats)) and fast_inter(feats).dtype == np.uint32


#          n_models, first, last, n_intervals, longest, longest_start, head, tail, span_sum
def _top_lifetimes(F):
    """The rows of pairs 0 ... 3 of ``_top_plan`` written out for F models (F odd), by gap."""
    every = (F, 0, F - 1, 1, F, 0, F, F, F)
    last = (1, F - 1, F - 1, 1, 1, F - 1, 1, 1, 1)
    apart, joined = (2, 0, F - 1, 2, 1, 0, 1, 1, 2), (2, 0, F - 1, 1, F, 0, F, F, F)
    half = (F + 1) // 2
    second = {0: (half, 0, F - 1, half, 1, 0, 1, 1, half)}
    return {gap: [every, apart if gap < F - 2 else joined, second.get(gap, (half, 0, F - 1, 1, F, 0, F, F, F)), last] for gap in (0, 1, F - 3, F - 2, F - 1)}


def test_lifetimes_of_the_planted_rows_at_the_top_of_uint16():
    """Pairs 0 ... 3 at F = 65535: the rows written out by hand are the definition (``_direct``) applied to each pair's models
    and what the vectorised yardstick makes of the hand-made bag — and what the looping ``reference_lifetimes`` makes of it, at
    gap 0 and 65533 and, at F = 129 with the gaps scaled alike, at every gap.  The values 65535 and 32768 are the largest a uint16 column, and a row's intervals, can
    reach."""
    for F in (129, F_TOP):
        sep, _ = _top_plan(F)
        sep = sep[:, :4]
        models = [np.nonzero(sep[:, r] <= 5.0)[0].tolist() for r in range(4)]
        assert [len(m) for m in models] == [F, 2, (F + 1) // 2, 1]
        aa = _planted_bag(sep, None, 8)
        want = _top_lifetimes(F)
        assert F != F_TOP or sorted(want) == sorted(GAPS)
        for gap, rows in want.items():
            assert rows == [_direct(m, gap) for m in models], (F, gap)
            t = fast_lifetimes(aa, 8, gap)
            assert list(zip(t['a'].tolist(), t['b'].tolist())) == [(0, 1), (2, 3), (4, 5), (6, 7)] and _rows(t) == rows, (F, gap)
            if F == 129 or gap in (0, 65533):      # (the loop over 65535 models takes two seconds a gap: the two that differ most)
                _same(reference_lifetimes(_per_model(aa, 8, F), 8, gap, *EVERY_RECORD), t, (F, gap))
    top = _top_lifetimes(F_TOP)
    assert top[0][0] == (65535, 0, 65534, 1, 65535, 0, 65535, 65535, 65535)
    assert top[65532][1] == (2, 0, 65534, 2, 1, 0, 1, 1, 2) and top[65533][1] == top[65534][1] == (2, 0, 65534, 1, 65535, 0, 65535, 65535, 65535)
    assert top[0][2] == (32768, 0, 65534, 32768, 1, 0, 1, 1, 32768) and top[1][2] == (32768, 0, 65534, 1, 65535, 0, 65535, 65535, 65535)
    assert top[0][3] == (1, 65534, 65534, 1, 1, 65534, 1, 1, 1)


# ---- coupling and similarity: the planted vectors
def _tops_vectors(F):
    """(names, bits [F, U]) of the coupling cases: 24 seeded random vectors; single-model vectors at models 0, 2047, 2048 and
    F - 1 (clipped to F - 1) and the complement of the last; a twin of vector 3 and the complement of vector 5; one record per
    model word (models 0, 64, ...) and the same offset by 63; a vector present in every model, which is outside every band; at
    F = 4096 the five vectors of 2048 models whose pairs put the criterion's integers at their largest."""
    rng = np.random.default_rng(1000 + F)
    rand = _vectors(rng, F, 24)
    cols = [('r%d' % k, rand[:, k]) for k in range(24)]
    m = np.arange(F)
    for name, at in (('at0', 0), ('at2047', 2047), ('at2048', 2048), ('last', F - 1)):
        cols.append((name, m == min(at, F - 1)))
    cols += [('not_last', m != F - 1), ('twin3', rand[:, 3].copy()), ('anti5', ~rand[:, 5]), ('word0', m % 64 == 0), ('word63', m % 64 == 63),
             ('every', m >= 0)]
    if F == 4096:
        v0 = m < 2048
        cols += [('v0', v0), ('v1', v0.copy()), ('v2', ~v0), ('v3', (m >= 512) & (m < 2560)), ('v4', (m >= 1536) & (m < 3584))]
    return [c[0] for c in cols], np.stack([c[1] for c in cols], axis=1)


def _feature_index(names, bits):
    """name -> index among the features of the band 1 ... F - 1 (the rows ascend with the columns of ``bits``)."""
    F = bits.shape[0]
    n = bits.sum(axis=0)
    band = (n >= 1) & (n <= F - 1)
    return {name: int(band[:u].sum()) for u, name in enumerate(names) if band[u]}


def _pair_row(ref, u, v):
    hit = np.nonzero((ref['u'] == u) & (ref['v'] == v))[0]
    assert len(hit) == 1
    return int(hit[0])


def _planted_reference(bits):
    """``test_coupling.reference_tables`` on the planted matrix itself (row r is the pair of atoms 2 r, 2 r + 1 of 2 U atoms)."""
    F, U = bits.shape
    n = 2 * U
    rows = np.array([2 * r * n + 2 * r + 1 for r in range(U)], np.int64)
    return reference_tables(rows, bits, n, 1, F - 1)


SEAM_PAIRS = (('v0', 'v1', 2048, 1 << 54, 1024), ('v0', 'v2', 0, 1 << 54, 1024),
              ('v0', 'v3', 1536, 1 << 52, 256), ('v0', 'v4', 512, 1 << 52, 256))      # (u, v, n11, 1024 d^2, the largest q that keeps it)


def test_the_criterion_at_its_largest_integers():
    """F = 4096, n_u = n_v = 2048: n_u (F - n_u) n_v (F - n_v) = 2^44, |d| = |F n11 - n_u n_v| = 2^22 for the identical and the
    complementary pair — 1024 d^2 = 2^54 = 1024 * 2^44, kept at q = 1024 with equality — and 2^21 for the pairs that share 1536
    and 512 models: 1024 d^2 = 2^52 = 256 * 2^44, kept at q = 256 and dropped at q = 257."""
    names, bits = _tops_vectors(4096)
    assert len(names) == 39 and bits[:, names.index('every')].all()
    ref = _planted_reference(bits)
    at = _feature_index(names, bits)
    assert 'every' not in at and len(at) == 38 == len(ref['features']['a'])
    for u, v, n11, lhs, q_top in SEAM_PAIRS:
        assert ref['features']['count'][at[u]] == ref['features']['count'][at[v]] == 2048
        r = _pair_row(ref, at[u], at[v])
        assert int(ref['n11'][r]) == n11 and int(ref['lhs'][r]) == lhs and int(ref['base'][r]) == 1 << 44, (u, v)
        d = 4096 * n11 - 2048 * 2048
        assert abs(d) == (1 << 22 if lhs == 1 << 54 else 1 << 21) and 1024 * d * d == lhs
        for q in (256, 257, 1024):
            k = kept(ref, q)
            assert ((at[u], at[v]) in set(zip(k['u'].tolist(), k['v'].tolist()))) == (q <= q_top), (u, v, q)
    # the one-record-per-word vectors touch every model word; the single-model vectors sit beside the panel seam
    for F in (2048, 2049, 4095, 4096):
        names, bits = _tops_vectors(F)
        col = lambda name: np.nonzero(bits[:, names.index(name)])[0]
        assert np.array_equal(np.unique(col('word0') // 64), np.arange((F + 63) // 64)) and len(col('word0')) == (F + 63) // 64
        assert np.array_equal(col('word63'), np.arange(63, F, 64))
        assert [col(k).tolist() for k in ('at0', 'at2047', 'at2048', 'last')] == [[0], [2047], [min(2048, F - 1)], [F - 1]]
        assert ((F + 63) // 64 > 32) == (F > 2048)      # a second panel of 32 model words


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def top():
    """One context with the field of ``_top_plan`` over 65535 models resident, one pass at 5 A, and its atom-atom bag — whose
    records must be the planted ones, distances included: that is the test of the pass over F models (k_models_expand,
    k_models_boxes with F blocks, the layout of F partitions, the structure ids of a million atoms)."""
    sep, partners = _top_plan()
    pc, xyz = _range_field(sep, partners)
    n = pc.n_atoms
    assert n == 17 and xyz.shape == (F_TOP, n, 3)
    ctx = _ctx_with_models(pc, xyz, np.zeros((F_TOP, 0, 3)))
    counts = ctx.run_launch(*PASS)
    f, a, b, d = _planted_records(sep, partners)
    assert counts == {'atom_atom': len(f), 'plane_plane': 0, 'atom_plane': 0, 'group_group': 0, 'group_plane': 0}
    aa = {k: np.array(v) for k, v in ctx.fetch_packed()[0]['atom_atom'].items()}
    gf, ga, gb = _cut(aa, n)
    assert np.array_equal(gf, f) and np.array_equal(ga, a) and np.array_equal(gb, b), 'the pass did not find the planted records'
    assert aa['dist'].tobytes() == d.tobytes()
    yield ctx, pc, aa
    ctx.close()


def _row_of(t, a, b, ka='a', kb='b'):
    hit = np.nonzero((t[ka] == a) & (t[kb] == b))[0]
    assert len(hit) == 1, (a, b)
    return int(hit[0])


def _check_planted_persistence(t, ka, kb, bits_key):
    """The planted rows of the two persistence tables, written out."""
    F = F_TOP
    for pair, nm, first, last in ((0, F, 0, F - 1), (1, 2, 0, F - 1), (2, 32768, 0, F - 1), (3, 1, F - 1, F - 1), (4, F, 0, F - 1), (5, F, 0, F - 1)):
        r = _row_of(t, 2 * pair, 2 * pair + 1, ka, kb)
        assert (int(t['n_models'][r]), int(t['first'][r]), int(t['last'][r])) == (nm, first, last), pair
        bits = t[bits_key][r].tolist()
        if pair < 4:      # one geometry in every model: every bit it sets is counted in every model
            assert set(bits) == {0, nm}, (pair, bits)
            assert t['dist_min'][r] == t['dist_max'][r] == np.float32(NEAR) and t['dist_sum'][r] == nm * NEAR
    sep, _ = _top_plan()
    a, b = _row_of(t, 8, 9, ka, kb), _row_of(t, 10, 11, ka, kb)
    assert float(t['dist_sum'][a]) == _ascending(sep[:, 4]) == float.fromhex('0x1.3000000000c00p+17'), float(t['dist_sum'][a]).hex()
    assert float(t['dist_sum'][b]) == _ascending(sep[:, 5]) == 32767 * LATE, float(t['dist_sum'][b]).hex()
    for r in (a, b):
        assert t['dist_min'][r] == np.float32(TINY) and t['dist_max'][r] == np.float32(LATE)
    for k, (nm, first) in enumerate(((F, 0), (F, 0), (2, 0), (1, F - 1))):      # the water's legs
        r = _row_of(t, 12, 13 + k, ka, kb)
        assert (int(t['n_models'][r]), int(t['first'][r]), int(t['last'][r])) == (nm, first, F - 1) and t['dist_sum'][r] == nm * LEG


@pytest.mark.gpu
def test_contact_persistence_over_65535_models(top):
    """k_persist_reduce over runs of 65535 records (1024 wave steps), fbits = 16, every uint16 column at 65535, and dist_sum
    of the two order-sensitive rows to the bit."""
    ctx, pc, aa = top
    got = ctx.models_persistence()
    _same(got, fast_persistence(aa, pc.n_atoms), 'persistence')
    assert len(got['a']) == 10
    _check_planted_persistence(got, 'a', 'b', 'bit_count')


@pytest.mark.gpu
def test_residue_persistence_over_65535_models(top):
    """The same at residue level (a residue an atom: dist_sum adds each model's smallest — its only — distance)."""
    ctx, pc, aa = top
    got = ctx.models_residue_persistence()
    _same(got, fast_residue_persistence(aa, pc.n_atoms, pc.res_id, F_TOP), 'residue persistence')
    assert len(got['res_a']) == 10 and np.array_equal(got['n_contacts'], got['n_models']) and np.array_equal(got['class_models'][:, 0], got['n_models'])
    _check_planted_persistence(got, 'res_a', 'res_b', 'bit_models')


@pytest.mark.gpu
def test_lifetimes_over_65535_models(top):
    """Every uint16 column at 65535, 32768 intervals in one row, and the gap at 65532 | 65533 | 65534."""
    ctx, pc, aa = top
    want = _top_lifetimes(F_TOP)
    for gap in GAPS:
        got = ctx.models_lifetimes(gap)
        _same(got, fast_lifetimes(aa, pc.n_atoms, gap), ('lifetimes', gap))
        rows = _rows(got)
        assert [rows[_row_of(got, 2 * r, 2 * r + 1)] for r in range(4)] == want[gap], gap
        every = want[gap][0]
        assert rows[_row_of(got, 8, 9)] == rows[_row_of(got, 10, 11)] == rows[_row_of(got, 12, 13)] == every, gap


@pytest.mark.gpu
def test_water_bridge_persistence_over_65535_models(top):
    """A bridge in every model (a run of 65535 bridge rows), one in the first and the last model, one in the last model only —
    at both levels, with and without the pairs of one residue (there are none: a residue an atom)."""
    ctx, pc, aa = top
    F = F_TOP
    joined, want = bridge_tables(aa, pc, F)
    assert len(joined['water']) == F + 2 + 5
    for same in (False, True):
        for level, by_res in (('atom', 0), ('residue', t_bridge.BYRES)):
            got = ctx.models_water_bridge_persistence(SIFT_ALL, (1 if same else 0) | by_res)
            t_bridge._same(got, want[level], (same, level))
            ka, kb = ('a', 'b') if level == 'atom' else ('res_a', 'res_b')
            assert list(zip(got[ka].tolist(), got[kb].tolist())) == [(13, 14), (13, 15), (13, 16), (14, 15), (14, 16), (15, 16)]
            assert got['n_models'].tolist() == [F, 2, 1, 2, 1, 1] and got['first'].tolist() == [0, 0, F - 1, 0, F - 1, F - 1]
            assert got['last'].tolist() == [F - 1] * 6 and got['n_waters'].tolist() == got['n_bridges'].tolist() == [F, 2, 1, 2, 1, 1]
            assert got['dist_sum'].tolist() == [2 * LEG * k for k in (F, 2, 1, 2, 1, 1)] and set(got['dist_min'].tolist()) == {2 * LEG}
            for side in ('a', 'b'):
                assert set(got['bit_models_' + side][0].tolist()) == {0, F}


@pytest.fixture(scope='module')
def cases():
    """The coupling case of every F, made once: (ctx, the yardstick's tables from the bags of the pass, pc, names, bits).
    ``test_coupling._field_case`` asserts that the presence matrix cut from the pass's own bags is the planted one."""
    made = {}

    def case(F):
        if F not in made:
            names, bits = _tops_vectors(F)
            made[F] = _field_case(bits) + (names, bits)
        return made[F]
    yield case
    for c in made.values():
        c[0].close()


@pytest.mark.gpu
@pytest.mark.parametrize('F', [2048, 2049, 4095, 4096])
def test_coupling_at_the_panel_seam_and_the_limit(cases, F):
    """The last model word of the first panel of k_couple_gram, the first word of the second, a ragged last word, and
    ARP_SIM_MAX_MODELS; k_couple_bits steps whose 64 records lie in 64 different words; at 4096 the criterion on its seams at
    its largest integers and the band's edges."""
    ctx, ref, pc, names, bits = cases(F)
    U = bits.shape[1]
    at = _feature_index(names, bits)
    assert len(at) == U - 1 == len(ref['features']['a']) and 'every' not in at
    planted = _planted_reference(bits)
    assert all(np.array_equal(planted[k], ref[k]) for k in ('u', 'v', 'n11', 'lhs', 'base'))
    band = dict(min_count=1, max_count=F - 1) if F == 4096 else {}
    for q in (1, 512, 1024) + ((256, 257) if F == 4096 else ()):
        f, p = check(ctx, ref, q, F, **band)
        st = ctx.stats()
        assert st['couple_rows'] == U and st['couple_features'] == U - 1 == len(f['a']) and st['couple_tile_pairs'] == 1, (q, st)
        got = dict(zip(zip(p['u'].tolist(), p['v'].tolist()), p['n11'].tolist()))
        if q == 1024:      # phi^2 = 1: the planted identical and complementary pairs
            assert got[at['r3'], at['twin3']] == int(bits[:, 3].sum()) and got[at['r5'], at['anti5']] == 0 and got[at['last'], at['not_last']] == 0
        if F == 4096:
            for u, v, n11, lhs, q_top in SEAM_PAIRS:
                assert ((at[u], at[v]) in got) == (q <= q_top) and got.get((at[u], at[v]), n11) == n11, (u, v, q)
    count = dict(zip(names, bits.sum(axis=0).tolist()))
    assert [int(f['count'][at[k]]) for k in ('at0', 'at2047', 'at2048', 'last', 'not_last', 'word0', 'word63')] == \
        [1, 1, 1, 1, F - 1, (F + 63) // 64, F // 64] == [count[k] for k in ('at0', 'at2047', 'at2048', 'last', 'not_last', 'word0', 'word63')]


def _split(ctx):
    return _capi.split_models(ctx.fetch_packed()[0], ctx._models)


@pytest.mark.gpu
@pytest.mark.parametrize('F', [4095, 4096])
def test_similarity_at_the_limit(cases, F):
    """k_sim_gram over 64 x 64 tiles of models — the last one ragged at 4095 — and, at 4096, the 64 MiB fetch the limit's
    message names: the whole matrix for the "any atom-atom record" plane alone, for all 16 atom-level planes and, at 4096, at
    residue level for all 20."""
    ctx, ref, pc, names, bits = cases(F)
    n = pc.n_atoms
    per = _split(ctx)
    res = (pc.res_id, np.zeros(0, np.int32), np.zeros(0, np.int32))
    for planes, by_residue in ((ANY, False), (ALL16, False)) + (((ALL20, True),) if F == 4096 else ()):
        feats = [model_features(b, planes, 0x7F, pc.n_residues if by_residue else n, res if by_residue else None) for b in per]
        want = fast_inter(feats)
        got = ctx.models_similarity(planes, by_residue=by_residue)
        assert got.shape == (F, F) and got.dtype == np.uint32 and got.nbytes == 4 * F * F      # (n_models == F; 64 MiB at 4096)
        assert np.array_equal(got, want), (planes, by_residue)
        assert np.array_equal(got, got.T) and np.array_equal(np.diagonal(got), [len(x) for x in feats])
        if planes == ANY:      # the planted matrix itself, in int64
            B = bits.astype(np.int64)
            assert np.array_equal(np.diagonal(got), B.sum(axis=1))
            pick = np.r_[0:3, 2046:2050, F - 3:F]
            assert np.array_equal(got[pick], B[pick] @ B.T)
        else:
            assert (np.diagonal(got) > bits.sum(axis=1)).all()      # more than the one plane
