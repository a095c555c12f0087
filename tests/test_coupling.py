"""Contact coupling over the models of an ensemble, correlated on the device (arp_models_coupling_launch / _fetch / _info,
Context.models_coupling, EnsembleComplex.run_coupling, arpeggio_amd.coupling).

The yardstick is never the device: it is ``reference_tables`` / ``kept`` below — a presence matrix [F, U] of booleans made from
per-model bags that did not come through the new code (the bags ``run_models`` fetches and cuts, and the oracle's; the rows of a
model are ``test_similarity.model_features``' keys), n, ``n11 = P.T @ P`` in int64, and the criterion
``1024 d^2 >= q n_u (F - n_u) n_v (F - n_v)`` evaluated with Python integers.  Every comparison is of exact integers.  No
tolerance anywhere, and no time is asserted."""
import copy
import ctypes as C
import functools
import itertools
import math
import os
import re

import numpy as np
import pytest

import oracle
from arpeggio_amd import _capi, coupling, similarity, synth, tables
from arpeggio_amd.core import config
from arpeggio_amd.core.exceptions import NativeLibraryError
from helpers import tiny_complex
from test_models import CASES, _selectors
from test_persistence import _ctx_with_models, _mask
from test_residue_pairs import PLANE_BAGS, _oracle_pass
from test_similarity import model_features

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
NP_ = similarity.N_PLANES
ALL16 = similarity.ATOM_PLANES
ALL20 = (1 << NP_) - 1
ANY = 1 << 15      # "any atom-atom record"
DEFAULT = similarity.planes(None, ('atom_atom',))
CHUNK = 1 << 17      # pairs the yardstick handles at a time as Python integers


# ------------------------------------------------------------------------------------------------------- the yardstick
def presence(per_model_bags, planes, ctype_mask, n, res=None):
    """(rows, P): the sorted row keys present in any model — atom level a * n + b, residue level res_a * nres + res_b — and
    the boolean presence matrix [F, U]."""
    keys = [np.unique(model_features(b, planes, ctype_mask, n, None if res is None else res[f]) // NP_) for f, b in enumerate(per_model_bags)]
    rows = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    P = np.zeros((len(keys), len(rows)), bool)
    for f, k in enumerate(keys):
        P[f, np.searchsorted(rows, k)] = True
    return rows, P


def reference_tables(rows, P, stride, min_count, max_count):
    """The feature table and, for every pair u < v of features in ascending (u, v): n11, 1024 d^2 and n_u (F - n_u) n_v (F - n_v),
    the last two as Python integers."""
    F = int(P.shape[0])
    n = P.sum(axis=0).astype(np.int64)
    feat = np.nonzero((n >= min_count) & (n <= max_count))[0]
    B = P[:, feat].astype(np.int64)
    n11 = B.T @ B
    nf = n[feat]
    iu, iv = np.triu_indices(len(feat), 1)
    lhs, base = np.zeros(len(iu), np.int64), np.zeros(len(iu), np.int64)
    for s in range(0, len(iu), CHUNK):      # (object arrays: the arithmetic is Python's; kept as int64, which the asserted bound allows)
        e = s + CHUNK
        x11, nu, nv = n11[iu[s:e], iv[s:e]].astype(object), nf[iu[s:e]].astype(object), nf[iv[s:e]].astype(object)
        d = F * x11 - nu * nv
        x, y = 1024 * d * d, nu * (F - nu) * nv * (F - nv)
        assert all(0 <= v < 1 << 58 for v in x) and all(0 <= v < 1 << 58 for v in y)
        lhs[s:e], base[s:e] = x, y
    features = dict(a=(rows[feat] // stride).astype(np.int32), b=(rows[feat] % stride).astype(np.int32), count=nf.astype(np.uint32))
    return dict(F=F, features=features, u=iu.astype(np.uint32), v=iv.astype(np.uint32), n11=n11[iu, iv].astype(np.uint32), lhs=lhs, base=base)


def kept(ref, q):
    """The pair table the device must return for phi2_q = q: 1024 d^2 >= q n_u (F - n_u) n_v (F - n_v) in Python integers."""
    keep = np.zeros(len(ref['lhs']), bool)
    for s in range(0, len(keep), CHUNK):
        keep[s:s + CHUNK] = (ref['lhs'][s:s + CHUNK].astype(object) >= int(q) * ref['base'][s:s + CHUNK].astype(object)).astype(bool)
    return dict(u=ref['u'][keep], v=ref['v'][keep], n11=ref['n11'][keep])


def same(got, want):
    return sorted(got) == sorted(want) and all(got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in want)


def check(ctx, ref, q, what, planes=ANY, ctype_mask=0x7F, by_residue=False, min_count=1, max_count=None):
    """The device's two tables against the yardstick's, and their canonical order."""
    want = kept(ref, q)
    f, p = ctx.models_coupling(planes, ctype_mask, by_residue, min_count, max_count, q, max_pairs=max(len(want['u']), 1))
    assert same(f, ref['features']), (what, 'features')
    assert same(p, want), (what, q, 'pairs')
    ab = f['a'].astype(np.int64) << 32 | f['b'].astype(np.int64)
    uv = p['u'].astype(np.int64) << 32 | p['v'].astype(np.int64)
    assert (np.diff(ab) > 0).all() and (np.diff(uv) > 0).all() and (p['u'] < p['v']).all(), (what, 'order')
    return f, p


def _bag(i, j):
    k = len(i)
    return dict(i=np.array(i, np.int32), j=np.array(j, np.int32), dist=np.zeros(k, np.float32), sift=np.full(k, BIT['proximal'], np.uint16),
                ctype=np.zeros(k, np.uint8))


# ------------------------------------------------------------------------------------------------------------- CPU
HAND = {(0, 1): (1, 1, 0, 0), (0, 2): (1, 1, 0, 0), (1, 2): (0, 0, 1, 1), (1, 3): (1, 0, 1, 0), (2, 3): (1, 1, 1, 1)}


def _hand():
    pairs = sorted(HAND)
    bags = [{'atom_atom': _bag([a for a, b in pairs if HAND[a, b][f]], [b for a, b in pairs if HAND[a, b][f]])} for f in range(4)]
    return presence(bags, ANY, 0x7F, 4)


def test_yardstick_on_a_hand_made_case():
    """Four models, five contacts over 4 atoms.  (0, 1) and (0, 2) are identical (phi = 1); (1, 2) is their complement
    (phi = -1); (1, 3) is independent of all three (n11 = 1 of n = 2 and 2 in 4 models: d = 0); (2, 3) is in every model
    and no feature."""
    rows, P = _hand()
    assert rows.tolist() == [1, 2, 6, 7, 11] and P.T.tolist() == [[bool(x) for x in HAND[k]] for k in sorted(HAND)]
    ref = reference_tables(rows, P, 4, 1, 3)
    assert ref['features']['a'].tolist() == [0, 0, 1, 1] and ref['features']['b'].tolist() == [1, 2, 2, 3]
    assert ref['features']['count'].tolist() == [2, 2, 2, 2]
    assert list(zip(ref['u'].tolist(), ref['v'].tolist(), ref['n11'].tolist())) == [(0, 1, 2), (0, 2, 0), (0, 3, 1), (1, 2, 0), (1, 3, 1), (2, 3, 1)]
    for q in (1, 512, 1024):      # the identical pair and the two complementary ones, at every threshold; the independent ones never
        k = kept(ref, q)
        assert list(zip(k['u'].tolist(), k['v'].tolist(), k['n11'].tolist())) == [(0, 1, 2), (0, 2, 0), (1, 2, 0)], q
    wide = reference_tables(rows, P, 4, 1, 4)      # (not a band the device admits: n = F has no variance; the yardstick keeps 0 >= 0)
    assert wide['features']['count'].tolist() == [2, 2, 2, 2, 4]
    pairs = kept(ref, 1024)
    assert coupling.phi(ref['features'], pairs, 4).tolist() == [1.0, -1.0, -1.0]
    assert coupling.covariance(ref['features'], pairs, 4).tolist() == [4, -4, -4]
    assert coupling.jaccard(ref['features'], pairs).tolist() == [1.0, 0.0, 0.0]


def test_phi2_q_rounding_and_counts():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    assert int(re.search(r'#define\s+ARP_COUPLE_MAX_FEATURES\s+(\d+)', hdr).group(1)) == coupling.MAX_FEATURES == _capi.COUPLE_MAX_FEATURES == 65536
    assert int(re.search(r'#define\s+ARP_COUPLE_BY_RESIDUE\s+(\d+)u', hdr).group(1)) == coupling.BY_RESIDUE == _capi.COUPLE_BY_RESIDUE == 1
    for s in ('arp_models_coupling_launch', 'arp_models_coupling_fetch', 'arp_models_coupling_info'):
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    assert coupling.phi2_q(0.5) == (256, 0.5) and coupling.phi2_q(1.0) == (1024, 1.0) and coupling.phi2_q(0.0) == (1, 1 / 32)
    assert coupling.phi2_q(0.75) == (576, 0.75) and coupling.phi2_q(1 / 32) == (1, 1 / 32) and coupling.phi2_q(2.0) == (1024, 1.0)
    q, eff = coupling.phi2_q(0.7)      # 0.49 * 1024 = 501.76 (and the float 0.7 is a little below 7 / 10)
    assert q == 502 and eff == math.sqrt(502 / 1024) and eff >= 0.7
    assert coupling.phi2_q(np.nextafter(0.5, 1.0))[0] == 257      # just above a representable seam: the next q
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            coupling.phi2_q(bad)
    assert coupling.counts(0.05, 0.95, 20) == (1, 19) and coupling.counts(0.25, 0.75, 64) == (16, 48)
    assert coupling.counts(0.0, 1.0, 10) == (1, 9) and coupling.counts(0.26, 0.74, 64) == (17, 47)
    assert coupling.counts(0.5, 0.5, 3) == (2, 1)      # (no count in between: run_coupling refuses it)
    with pytest.raises(ValueError):
        coupling.counts(0.1, 0.9, 1)


def test_phi_jaccard_and_groups():
    f = dict(a=np.arange(6, dtype=np.int32), b=np.arange(6, dtype=np.int32) + 10, count=np.array([2, 2, 2, 4, 1, 3], np.uint32))
    p = dict(u=np.array([0, 0, 1, 3], np.uint32), v=np.array([1, 2, 2, 4], np.uint32), n11=np.array([2, 0, 0, 1], np.uint32))
    F = 6
    ph = coupling.phi(f, p, F)
    assert ph.dtype == np.float64 and ph[0] == 1.0 and ph[1] == ph[2] == (0 - 4) / math.sqrt(8 * 8)
    assert ph[3] == (6 - 4) / math.sqrt(4 * 2 * 1 * 5)
    assert coupling.jaccard(f, p).tolist() == [1.0, 0.0, 0.0, 0.25]
    g = coupling.groups(f, p, n_models=F)
    assert [x.tolist() for x in g] == [[0, 1], [3, 4]]      # the anti-correlated edges join nothing; 2 and 5 stay alone
    assert [x.tolist() for x in coupling.groups(f, p, positive_only=False)] == [[0, 1, 2], [3, 4]]
    with pytest.raises(ValueError, match='n_models'):
        coupling.groups(f, p)
    e = coupling.empty()
    assert coupling.groups(*e, positive_only=False) == [] and len(coupling.phi(*e, 4)) == 0


def test_csv_text_and_records(tmp_path):
    from arpeggio_amd.core import export
    pc = synth.proteinlike(n_res=6, seed=3, n_waters=0)
    pc.ensure_labels()
    lab = export.Labels(pc, pc.component_types)
    f = dict(a=np.array([0, 2], np.int32), b=np.array([5, 7], np.int32), count=np.array([2, 2], np.uint32))
    p = dict(u=np.array([0], np.uint32), v=np.array([1], np.uint32), n11=np.array([0], np.uint32))
    path = coupling.write_coupling(str(tmp_path), 'ens', f, p, pc, 4)
    assert os.path.basename(path) == 'ens.coupling'
    assert open(path, newline='').read() == ('u_bgn,u_end,v_bgn,v_end,n_u,n_v,n11,phi\r\n%s,%s,%s,%s,2,2,0,-1.0\r\n'
                                             % tuple(lab.atom_macro(k) for k in (0, 5, 2, 7)))
    rec = coupling.to_records(pc, f, p, 4)
    assert rec == [{'bgn': {'bgn': lab.atom_dict(0), 'end': lab.atom_dict(5), 'n_models': 2},
                    'end': {'bgn': lab.atom_dict(2), 'end': lab.atom_dict(7), 'n_models': 2},
                    'type': 'contact-coupling', 'n_both': 0, 'phi': -1.0, 'jaccard': 0.0}]
    fr = dict(f, a=np.array([0, 1], np.int32), b=np.array([2, 3], np.int32))
    coupling.write_csv(str(tmp_path / 'r.csv'), fr, p, pc, 4, level='residue')
    assert open(str(tmp_path / 'r.csv'), newline='').read().split('\r\n')[1] == '%s,%s,%s,%s,2,2,0,-1.0' % tuple(lab.res_macro[k] for k in (0, 2, 1, 3))
    with pytest.raises(ValueError, match='level'):
        coupling.write_csv(str(tmp_path / 'x.csv'), f, p, pc, 4, level='chain')


# ------------------------------------------------------------------------------------------------------------- GPU
PASS = (5.0, 0.1, True)


def _dimer_field(bits):
    """``bits`` bool [F, U]: U isolated atom pairs on a 20 A lattice, a residue an atom (no polypeptide: no sequence-adjacency
    filter); pair r — atoms 2 r, 2 r + 1 — is 3.5 A apart in the models where its bit is set and 9 A apart otherwise.  At 5 A
    row (2 r, 2 r + 1) is present exactly in the models of bits[:, r].  Returns (pc, xyz [F, 2 U, 3], h_xyz)."""
    bits = np.asarray(bits, bool)
    F, U = bits.shape
    side = max(1, math.ceil(U ** (1 / 3) - 1e-9))
    r = np.arange(U)
    site = 20.0 * np.stack([r % side, (r // side) % side, r // (side * side)], axis=1)
    xyz = np.zeros((F, 2 * U, 3), np.float32)
    xyz[:, 0::2] = site[None]
    xyz[:, 1::2] = site[None]
    xyz[:, 1::2, 0] += np.where(bits, 3.5, 9.0)
    return tiny_complex(xyz[0]), np.ascontiguousarray(xyz), np.zeros((F, 0, 3))


def _field_case(bits, min_count=1, max_count=None):
    """A context with the dimer field resident and a pass made, and the yardstick's tables from the bags ``run_models`` cut —
    whose presence matrix must be the planted one."""
    bits = np.asarray(bits, bool)
    pc, xyz, h_xyz = _dimer_field(bits)
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    per = ctx.run_models(*PASS)
    rows, P = presence(per, ANY, 0x7F, pc.n_atoms)
    used = bits.any(axis=0)
    assert rows.tolist() == [2 * r * pc.n_atoms + 2 * r + 1 for r in np.nonzero(used)[0]] and np.array_equal(P, bits[:, used])
    F = bits.shape[0]
    return ctx, reference_tables(rows, P, pc.n_atoms, min_count, F - 1 if max_count is None else max_count), pc


def _vectors(rng, F, U, lo=1, hi=None):
    """U seeded random presence vectors over F models, each with lo ... hi models (default F - 1)."""
    hi = F - 1 if hi is None else hi
    out = np.zeros((F, U), bool)
    for r in range(U):
        out[rng.choice(F, size=int(rng.integers(lo, hi + 1)), replace=False), r] = True
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('F', [63, 64, 65, 129])
def test_model_word_seams(F):
    """The models end inside, at the end of and one past a 64-bit word, and in a third word.  24 random vectors, and planted:
    an identical pair, a complementary pair, vectors of one model each — the first, the last, and the two beside a word seam —
    and the complement of the last-model vector."""
    rng = np.random.default_rng(100 + F)
    bits = _vectors(rng, F, 24)
    twin = bits[:, 3].copy()
    anti = ~bits[:, 5]
    single = np.zeros((F, 4), bool)
    for k, f in enumerate((0, F - 1, min(63, F - 1), min(64, F - 1))):
        single[f, k] = True
    bits = np.concatenate([bits, twin[:, None], anti[:, None], single, ~single[:, 1:2]], axis=1)
    ctx, ref, pc = _field_case(bits)
    U = bits.shape[1]
    for q in (1, 512, 1024):
        f, p = check(ctx, ref, q, F)
        st = ctx.stats()
        assert st['couple_rows'] == st['couple_features'] == U == len(f['a']) and st['couple_tile_pairs'] == 1
    got = set(zip(p['u'].tolist(), p['v'].tolist()))      # at phi^2 = 1: the planted pairs
    assert {(3, 24), (5, 25), (27, 30)} <= got
    assert p['n11'][list(zip(p['u'].tolist(), p['v'].tolist())).index((5, 25))] == 0
    assert f['count'][26:30].tolist() == [1, 1, 1, 1] and f['count'][30] == F - 1
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 2, 63, 64, 65, 130])
def test_tile_seams(K):
    """One ragged tile, one full tile, a diagonal + an off-diagonal + a ragged diagonal tile, three tile rows.  Among the K
    features stand 9 rows outside the band (every model, or one model with min_count = 2), so that the compaction renumbers."""
    F = 8
    rng = np.random.default_rng(K)
    U = K + 9
    out_of_band = np.sort(rng.choice(U, size=9, replace=False))
    bits = np.zeros((F, U), bool)
    bits[:, np.setdiff1d(np.arange(U), out_of_band)] = _vectors(rng, F, K, 2, F - 1)
    for k, r in enumerate(out_of_band):
        if k % 2:
            bits[:, r] = True
        else:
            bits[k % F, r] = True
    ctx, ref, pc = _field_case(bits, 2)
    assert len(ref['features']['a']) == K
    tiles = (K + 63) // 64
    for q in (256, 1024):
        f, p = check(ctx, ref, q, K, min_count=2)
        st = ctx.stats()
        assert st['couple_rows'] == U and st['couple_features'] == K and st['couple_tile_pairs'] == (tiles * (tiles + 1) // 2 if K > 1 else 0)
    if K >= 65:      # kept pairs of a diagonal and of an off-diagonal tile (equal vectors abound among 2^8)
        assert st['couple_tile_pairs'] >= 2
        tu, tv = p['u'] // 64, p['v'] // 64
        assert (tu == tv).any() and (tu != tv).any() and (tv == tiles - 1).any()
    ctx.close()


@pytest.mark.gpu
def test_the_threshold_on_its_seam():
    """F = 64, n_u = n_v = 32.  n11 = 24: d = 64 * 24 - 1024 = 512, 1024 d^2 = 2^28 = 256 * 32^4: phi^2 = 1 / 4 exactly, kept at
    q = 256 and dropped at q = 257; its anti-correlated twin (n11 = 8, d = -512) likewise.  The third pair has d = 0."""
    F = 64
    bits = np.zeros((F, 3), bool)
    bits[0:32, 0] = True
    bits[8:40, 1] = True
    bits[24:56, 2] = True
    ctx, ref, pc = _field_case(bits)
    assert ref['n11'].tolist() == [24, 8, 16] and ref['lhs'].tolist() == [1 << 28, 1 << 28, 0] and ref['base'].tolist() == [1 << 20] * 3
    f, p = check(ctx, ref, 256, 'kept')
    assert list(zip(p['u'].tolist(), p['v'].tolist(), p['n11'].tolist())) == [(0, 1, 24), (0, 2, 8)]
    assert coupling.phi(f, p, F).tolist() == [0.5, -0.5]
    f, p = check(ctx, ref, 257, 'dropped')
    assert len(p['u']) == 0 and len(f['a']) == 3
    ctx.close()


@pytest.mark.gpu
def test_occupancy_seams_and_capacity_and_empty_results():
    """The band is inclusive: of rows with n = min - 1, min, max, max + 1 the middle two are features (twice each, identical:
    two kept pairs).  Then max_pairs one short of the kept pairs, and the two kinds of empty result."""
    F, lo, hi = 10, 3, 6
    bits = np.zeros((F, 8), bool)
    for r, n in enumerate((2, 3, 6, 7, 3, 6, 2, 7)):
        bits[:n, r] = True
    ctx, ref, pc = _field_case(bits, lo, hi)
    assert ref['features']['count'].tolist() == [3, 6, 3, 6] and ref['features']['a'].tolist() == [2, 4, 8, 10]
    f, p = check(ctx, ref, 1024, 'band', min_count=lo, max_count=hi)
    assert list(zip(p['u'].tolist(), p['v'].tolist(), p['n11'].tolist())) == [(0, 2, 3), (1, 3, 6)]
    all_pairs = kept(ref, 1)
    n_pairs = len(all_pairs['u'])
    assert n_pairs == 6      # (nested vectors: every pair is correlated)
    # ---- capacity: one short — the exact count, no result, a fetch refused —, then exactly enough
    L, h = ctx._L, ctx._h
    launches = ctx.stats()['couple_launches']
    with pytest.raises(NativeLibraryError) as e:
        ctx.models_coupling(ANY, min_count=lo, max_count=hi, phi2_q=1, max_pairs=n_pairs - 1)
    assert e.value.code == _capi.ARP_E_CAPACITY and e.value.n_pairs == n_pairs and e.value.n_features == 4
    nk, npr = C.c_int64(-1), C.c_int64(-1)
    buf = [np.full(16, 7, np.uint32) for _ in range(6)]
    assert L.arp_models_coupling_fetch(h, 16, 16, *(_capi._p(x) for x in buf), C.byref(nk), C.byref(npr)) == _capi.ARP_E_ARG
    assert all((x == 7).all() for x in buf)
    st = ctx.stats()
    assert st['couple_rows'] == st['couple_features'] == st['couple_tile_pairs'] == 0 and st['couple_launches'] == launches
    f, p = ctx.models_coupling(ANY, min_count=lo, max_count=hi, phi2_q=1, max_pairs=n_pairs)
    assert same(f, ref['features']) and same(p, all_pairs) and ctx.stats()['couple_launches'] == launches + 1
    # (a fetch into too small buffers: the counts, nothing written; NULL columns are skipped)
    assert L.arp_models_coupling_fetch(h, 3, 16, *(_capi._p(x) for x in buf), C.byref(nk), C.byref(npr)) == _capi.ARP_E_CAPACITY
    assert (nk.value, npr.value) == (4, n_pairs) and all((x == 7).all() for x in buf)
    assert L.arp_models_coupling_fetch(h, 16, n_pairs - 1, *(_capi._p(x) for x in buf), C.byref(nk), C.byref(npr)) == _capi.ARP_E_CAPACITY
    assert L.arp_models_coupling_fetch(h, 16, 16, None, None, _capi._p(buf[2]), None, None, _capi._p(buf[5]), C.byref(nk), C.byref(npr)) == _capi.ARP_OK
    assert buf[2][:4].tolist() == [3, 6, 3, 6] and buf[5][:n_pairs].tolist() == all_pairs['n11'].tolist() and (buf[0] == 7).all()
    # ---- a band that keeps no feature; a threshold that keeps no pair
    f, p = ctx.models_coupling(ANY, min_count=4, max_count=5)
    assert same(f, tables.empty(tables.COUPLING_FEATURES)) and same(p, tables.empty(tables.COUPLING_PAIRS))
    assert ctx.stats()['couple_rows'] == 8 and ctx.stats()['couple_features'] == 0
    ctx.close()
    # ---- no pair at all: two independent vectors (n11 = 1 of n = 2 and 2 in four models: d = 0), kept at no q; max_pairs = 0
    ctx, ref, pc = _field_case(np.array([[1, 1, 0, 0], [1, 0, 1, 0]], bool).T)
    assert ref['lhs'].tolist() == [0] and ref['base'].tolist() == [16]
    for q in (1, 1024):
        f, p = check(ctx, ref, q, 'independent')
        assert len(f['a']) == 2 and len(p['u']) == 0 and p['u'].dtype == np.uint32
    f, p = ctx.models_coupling(ANY, phi2_q=1, max_pairs=0)
    assert len(f['a']) == 2 and len(p['u']) == 0
    ctx.close()


F_ORACLE = 65


@functools.lru_cache(maxsize=None)
def _oracle_models():
    pc = synth.proteinlike(n_res=40, seed=21, n_waters=20)
    pc.ensure_labels()
    return (pc,) + tuple(synth.models_of(pc, F_ORACLE, seed=4, jitter=0.3))


@functools.lru_cache(maxsize=None)
def _oracle_bags():
    """The oracle's atom-atom bag of every model at 5 A, made once (model f of ``models_of`` does not depend on F)."""
    pc, xyz, h_xyz = _oracle_models()
    out = []
    for f in range(F_ORACLE):
        q = copy.copy(pc)
        q.xyz, q.h_xyz = np.ascontiguousarray(xyz[f]), np.ascontiguousarray(h_xyz[f])
        oc = oracle.OracleComplex(q)
        oc.make_selection(None)
        out.append({'atom_atom': oc.atom_contacts(5.0, 0.1, False)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('F', [20, F_ORACLE])
def test_atom_level_against_the_oracle(F):
    """The structure of similarity's tile test, F = 20 and 65 models at 5 A, the band 2 ... F - 2: the features and the pairs at
    q = 512 and at q = 1 (max_pairs sized from the yardstick) equal the yardstick's over run_models' bags and over the oracle's."""
    pc, xyz, h_xyz = _oracle_models()
    ctx = _ctx_with_models(pc, xyz[:F], h_xyz[:F])
    per = [{'atom_atom': m['atom_atom']} for m in ctx.run_models(5.0, 0.1, False)]
    rows, P = presence(per, DEFAULT, 0x7F, pc.n_atoms)
    orows, oP = presence(_oracle_bags()[:F], DEFAULT, 0x7F, pc.n_atoms)
    assert np.array_equal(rows, orows) and np.array_equal(P, oP)      # one yardstick from either source
    ref = reference_tables(rows, P, pc.n_atoms, 2, F - 2)
    K = len(ref['features']['a'])
    assert K > 128 and K < len(rows)
    for q in (512, 1):
        f, p = check(ctx, ref, q, F, planes=DEFAULT, min_count=2, max_count=F - 2)
        print('F', F, 'q', q, 'rows', len(rows), 'features', K, 'pairs', len(p['u']), ctx.stats())
        assert 0 < len(p['u']) < K * (K - 1) // 2
    assert (coupling.covariance(f, p, F) < 0).any() and (coupling.covariance(f, p, F) > 0).any()
    ctx.close()


@pytest.mark.gpu
def test_planes_and_contact_types():
    pc, xyz, h_xyz = _oracle_models()
    F = 9
    ctx = _ctx_with_models(pc, xyz[:F], h_xyz[:F])
    lig = _selectors(pc)[2]
    for sel, ctype_mask in (([], 0x7F), (lig, 1 << CT['INTER']), (lig, 0x7F)):
        ctx.set_selection(np.tile(_mask(pc, sel), F))
        per = [{'atom_atom': m['atom_atom']} for m in ctx.run_models(5.0, 0.1, False)]
        types = np.concatenate([m['atom_atom']['ctype'] for m in per])
        if sel:
            assert (types == CT['INTER']).any() and (types != CT['INTER']).any()      # the mask has something to exclude
        for planes in (BIT['hbond'], BIT['hbond'] | BIT['aromatic'] | ANY, BIT['vdw'] | BIT['hydrophobic'], ALL16):      # single, non-contiguous, all 16
            ref = reference_tables(*presence(per, planes, ctype_mask, pc.n_atoms), pc.n_atoms, 2, F - 2)
            f, p = check(ctx, ref, 512, (sel, ctype_mask, planes), planes=planes, ctype_mask=ctype_mask, min_count=2, max_count=F - 2)
            assert len(f['a']) > 0
    ctx.close()


@pytest.mark.gpu
def test_residue_level():
    """CASES[0] (proteinlike120, F = 20), all 20 planes, against the yardstick over run_models' bags and, whole structure, over the
    oracle's."""
    from arpeggio_amd.core import EnsembleComplex
    name, make, F, jitter = CASES[0]
    pc = make()
    pc.ensure_labels()
    xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=jitter)
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    ens.initialize()
    ctx = ens._ctx
    packs = [ens.model_pack(f) for f in range(F)]
    res = [(q.res_id, q.ring_res, q.amide_res) for q in packs]
    for sel in _selectors(pc)[::2]:
        ctx.set_selection(np.tile(_mask(pc, sel), F))
        per = ctx.run_models(5.0, 0.1, False)
        rows, P = presence(per, ALL20, 0x7F, pc.n_residues, res)
        ref = reference_tables(rows, P, pc.n_residues, 2, F - 2)
        f, p = check(ctx, ref, 512, sel, planes=ALL20, by_residue=True, min_count=2, max_count=F - 2)
        assert len(f['a']) > 0 and len(p['u']) > 0
        if not sel:
            orows, oP = presence([_oracle_pass(q) for q in packs], ALL20, 0x7F, pc.n_residues, res)
            assert np.array_equal(rows, orows) and np.array_equal(P, oP), 'oracle'
            for planes, ctm in ((0x1F << 15, 0x7F), (ALL20, 1 << CT['INTRA_NON_SELECTION'])):      # the class planes alone; a type mask
                r2 = reference_tables(*presence(per, planes, ctm, pc.n_residues, res), pc.n_residues, 2, F - 2)
                check(ctx, r2, 512, (sel, planes, ctm), planes=planes, ctype_mask=ctm, by_residue=True, min_count=2, max_count=F - 2)
        via = ens.run_coupling(sel, 5.0, 0.1, False, contacts=config.SIFT_NAMES[:15], classes=tables.CLASSES, level='residue',
                               min_occupancy=0.1, max_occupancy=0.9, min_abs_phi=0.7071)      # (0.7071^2 * 1024 = 511.99: q = 512)
        assert same(via[0], f) and same(via[1], p), (sel, 'ensemble')


@pytest.mark.gpu
def test_residue_level_leaves_out_records_without_a_residue():
    """``test_residue_persistence.seam_sentinel_tie`` in four models, the stacked amides of residue 3 pulled apart in model 1, with
    an installed selection state and the five bags launched one by one (a complete pass): the group-group records of the amide
    without a residue (-1) are left out — they trail the last row, (3, 3), whose key in model 3 is all ones."""
    from test_residue_persistence import _translated, seam_sentinel_tie
    pc = seam_sentinel_tie()
    F = 4
    xyz, h_xyz = _translated(pc, F)
    xyz[1, 6:, 2] += np.float32(30.0)      # model 1: the second and the third amide leave the first
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    ones = lambda k: np.ones(F * k, np.uint8)
    ctx.set_selection_state(ones(pc.n_atoms), ones(pc.n_atoms), ones(pc.n_rings), ones(pc.n_rings), ones(pc.n_amides), ones(pc.n_amides))
    ctx.atom_contacts_launch(5.0, 0.1, False)
    bags = {name: (ctx.launch_bag(name), ctx.fetch_bag(name))[1] for name, *_ in PLANE_BAGS}
    bags['atom_atom'] = ctx.atom_contacts_fetch(F * pc.n_atoms * pc.n_atoms)
    per = _capi.split_models(bags, ctx._models)
    res = [(pc.res_id, pc.ring_res, pc.amide_res)] * F
    left_out = 0
    for f, m in enumerate(per):
        gg = np.stack([pc.amide_res[m['group_group']['bgn']], pc.amide_res[m['group_group']['end']]], axis=1)
        left_out += int((gg.min(axis=1) < 0).sum())
    assert left_out > 0
    for planes in (ALL20, 1 << 18, (1 << 18) | ANY):
        rows, P = presence(per, planes, 0x7F, pc.n_residues, res)
        ref = reference_tables(rows, P, pc.n_residues, 1, F - 1)
        f, p = check(ctx, ref, 1, planes, planes=planes, by_residue=True)
        if planes == 1 << 18:      # the one row (3, 3): a feature, absent in model 1 only
            assert (f['a'].tolist(), f['b'].tolist(), f['count'].tolist()) == ([3], [3], [3])
    ctx.close()


def _everything(ctx):
    """The five bags, both persistence tables, the similarity matrix and the lifetimes table as bytes."""
    bags, _ = ctx.fetch_packed()
    out = {(name, k): np.asarray(v).tobytes() for name, b in bags.items() if isinstance(b, dict) for k, v in b.items()}
    for name, t in (('persist', ctx.models_persistence()), ('respersist', ctx.models_residue_persistence()), ('lifetimes', ctx.models_lifetimes())):
        out.update({(name, k): v.tobytes() for k, v in t.items()})
    out['similarity'] = ctx.models_similarity(DEFAULT).tobytes()
    return out


@pytest.mark.gpu
def test_nothing_else_changes_and_a_second_launch_does_no_work():
    pc, xyz, h_xyz = _oracle_models()
    F = 6
    xyz, h_xyz = xyz[:F], h_xyz[:F]
    plain = _ctx_with_models(pc, xyz, h_xyz, sort_after=False)      # never calls the new code
    per = plain.run_models(5.0, 0.1, False)
    planes_dev = plain.models_planes()
    res = [(pc.res_id, planes_dev['ring_res'][f], pc.amide_res) for f in range(F)]
    aa = [{'atom_atom': m['atom_atom']} for m in per]
    ref_atom = reference_tables(*presence(aa, DEFAULT, 0x7F, pc.n_atoms), pc.n_atoms, 1, F - 1)
    ref_band = reference_tables(*presence(aa, DEFAULT, 0x7F, pc.n_atoms), pc.n_atoms, 2, F - 2)
    ref_res = reference_tables(*presence(per, ALL20, 0x7F, pc.n_residues, res), pc.n_residues, 1, F - 1)
    big = 1 << 22

    def got(ctx, ref, q, **kw):
        f, p = ctx.models_coupling(kw.pop('planes', DEFAULT), phi2_q=q, max_pairs=big, **kw)
        return same(f, ref['features']) and same(p, kept(ref, q))
    for rows in (False, True):
        plain.set_packed_layout(rows)
        plain.run_launch(5.0, 0.1, False)
        ref = _everything(plain)
        for sort_after, order in itertools.product((False, True), ('fetch first', 'coupling first')):
            what = (rows, sort_after, order)
            ctx = _ctx_with_models(pc, xyz, h_xyz, sort_after=sort_after)
            ctx.set_packed_layout(rows)
            ctx.run_launch(5.0, 0.1, False)
            if order == 'fetch first':
                assert _everything(ctx) == ref, what
            n0 = ctx.stats()['couple_launches']
            assert got(ctx, ref_atom, 512), what
            st = ctx.stats()
            assert st['couple_launches'] == n0 + 1 and st['couple_features'] == len(ref_atom['features']['a'])
            keep = {k: v for k, v in st.items() if k.startswith('couple_')}
            assert got(ctx, ref_atom, 512) and ctx.stats() == st, what      # the resident result
            assert _everything(ctx) == ref, what
            assert got(ctx, ref_atom, 512) and {k: v for k, v in ctx.stats().items() if k.startswith('couple_')} == keep, what      # nothing voided it
            for n, (r, q, kw) in enumerate(((ref_atom, 768, {}), (ref_band, 768, dict(min_count=2, max_count=F - 2)),
                                            (ref_res, 768, dict(planes=ALL20, by_residue=True))), 2):      # other arguments remake it
                assert got(ctx, r, q, **kw) and ctx.stats()['couple_launches'] == n0 + n, (what, n)
            assert _everything(ctx) == ref, what
            # a residue-level result reads the ring / amide bags: refilling one voids it
            ctx.launch_bag('plane_plane')
            assert got(ctx, ref_res, 768, planes=ALL20, by_residue=True) and ctx.stats()['couple_launches'] == n0 + 5, what
            # an atom-level result reads the atom-atom bag alone: the same refill leaves it
            assert got(ctx, ref_atom, 512) and ctx.stats()['couple_launches'] == n0 + 6
            ctx.launch_bag('group_group')
            ctx.set_packed_layout(not rows)
            ctx.set_packed_layout(rows)
            assert got(ctx, ref_atom, 512) and ctx.stats()['couple_launches'] == n0 + 6, what
            ctx.run_launch(5.0, 0.1, False)      # a new pass voids it: made again
            assert got(ctx, ref_atom, 512) and ctx.stats()['couple_launches'] == n0 + 7, what
            ctx.set_models(xyz, h_xyz)           # new models void it with the results
            with pytest.raises(ValueError, match='no results'):
                ctx.models_coupling(DEFAULT)
            ctx.close()
    plain.close()


@pytest.mark.gpu
def test_refusals():
    pc, xyz, h_xyz = _oracle_models()
    F = 4
    xyz, h_xyz = xyz[:F], h_xyz[:F]
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.run_launch(5.0, 0.1, False)
    L, h = ctx._L, ctx._h
    nk, npr = C.c_int64(-1), C.c_int64(-1)

    def launch(L, h, planes=DEFAULT, ctm=0x7F, flags=0, lo=1, hi=F - 1, q=512, max_pairs=1 << 20):
        return L.arp_models_coupling_launch(h, planes, ctm, flags, lo, hi, q, max_pairs, C.byref(nk), C.byref(npr))
    assert launch(L, h) == _capi.ARP_E_ARG and 'no models resident' in L.arp_last_error(h).decode()
    with pytest.raises(ValueError, match='no models resident'):
        ctx.models_coupling(DEFAULT)
    ctx.set_topology(pc)
    ctx.set_models(xyz, h_xyz)
    with pytest.raises(ValueError, match='no results'):
        ctx.models_coupling(DEFAULT)
    buf = [np.full(8, 7, np.uint32) for _ in range(6)]
    assert L.arp_models_coupling_fetch(h, 8, 8, *(_capi._p(x) for x in buf), C.byref(nk), C.byref(npr)) == _capi.ARP_E_ARG      # nothing launched
    ctx.atom_contacts_launch(5.0, 0.1, False)      # the atom-atom bag alone: atom level runs, residue level refuses
    f, p = ctx.models_coupling(DEFAULT, phi2_q=1024)
    assert len(f['a']) > 0
    with pytest.raises(ValueError, match='complete pass'):
        ctx.models_coupling(DEFAULT, by_residue=True)
    for kw, what in ((dict(planes=0), 'mask of 0'), (dict(planes=1 << 20), 'beyond'), (dict(ctm=0), 'mask of 0'), (dict(ctm=0x80), 'beyond'),
                     (dict(planes=1 << 16), 'residue level only'), (dict(planes=ALL20), 'residue level only'),
                     (dict(flags=2), 'unknown flag'), (dict(planes=ALL20, flags=3), 'unknown flag'),
                     (dict(q=0), 'phi2_q'), (dict(q=1025), 'phi2_q'), (dict(max_pairs=-1), 'max_pairs'),
                     (dict(lo=3, hi=2), 'min_count'), (dict(lo=0), 'min_count'), (dict(hi=F), 'min_count')):
        assert launch(L, h, **kw) == _capi.ARP_E_ARG, (kw, what)
        assert what in L.arp_last_error(h).decode(), (kw, what)
    # a refused launch leaves the resident result
    got = tables.alloc(tables.COUPLING_FEATURES, len(f['a']))
    assert L.arp_models_coupling_fetch(h, len(f['a']), len(p['u']), *(_capi._p(got[k]) for k in ('a', 'b', 'count')), None, None, None,
                                       C.byref(nk), C.byref(npr)) == _capi.ARP_OK and same(got, f)
    # a selection change voids it with the results
    ctx.set_selection(np.tile(_mask(pc, []), F))
    with pytest.raises(ValueError, match='no results'):
        ctx.models_coupling(DEFAULT)
    assert L.arp_models_coupling_fetch(h, 8, 8, *(_capi._p(x) for x in buf), C.byref(nk), C.byref(npr)) == _capi.ARP_E_ARG
    ctx.close()
    # a shard
    c2 = _capi.Context(0)
    c2.set_complex(pc)
    c2.set_ownership(np.ones(pc.n_atoms, np.uint8), np.arange(pc.n_atoms, dtype=np.int32))
    assert launch(c2._L, c2._h) == _capi.ARP_E_ARG and 'shard' in c2._L.arp_last_error(c2._h).decode()
    c2.close()
    # one model: no band exists; more models than ARP_SIM_MAX_MODELS: refused at the launch, before anything is sized
    two = tiny_complex([(0.0, 0.0, 0.0), (3.0, 0.0, 0.0)])
    for many, rc, what in ((1, _capi.ARP_E_ARG, 'F >= 2'), (similarity.MAX_MODELS + 1, _capi.ARP_E_CAPACITY, '4096')):
        c3 = _ctx_with_models(two, np.repeat(np.asarray(two.xyz, np.float32)[None], many, axis=0), np.zeros((many, 0, 3)))
        c3.run_launch(*PASS)
        for lo, hi in ((1, 1), (1, max(many - 1, 0))):
            assert launch(c3._L, c3._h, planes=ANY, lo=lo, hi=hi) == rc and what in c3._L.arp_last_error(c3._h).decode(), (many, lo, hi)
        c3.close()


@pytest.mark.gpu
def test_more_features_than_the_limit():
    """65 537 dimers in two models, each present in one of them: every row is a feature of the band 1 ... 1, one more than
    ARP_COUPLE_MAX_FEATURES.  Refused after the second wait with the exact K, before the product is sized; no result is left."""
    U = coupling.MAX_FEATURES + 1
    bits = np.zeros((2, U), bool)
    bits[np.arange(U) % 2, np.arange(U)] = True
    pc, xyz, h_xyz = _dimer_field(bits)
    ctx = _ctx_with_models(pc, xyz, h_xyz)
    assert ctx.run_launch(*PASS)['atom_atom'] == U
    with pytest.raises(NativeLibraryError, match='65 536 features') as e:
        ctx.models_coupling(ANY)
    assert e.value.code == _capi.ARP_E_CAPACITY and e.value.n_features == U and e.value.n_pairs == 0
    st = ctx.stats()
    assert st['couple_features'] == 0 and st['couple_launches'] == 0
    ctx.close()


@pytest.mark.gpu
def test_run_coupling_and_write_coupling(tmp_path):
    """End to end on a planted case: beside a random background, three groups of contacts that switch as one — and one
    contact that is the complement of group 0.  ``groups`` returns the planted sets."""
    from arpeggio_amd.core import EnsembleComplex, export
    F = 40
    rng = np.random.default_rng(7)
    proto = np.zeros((F, 3), bool)
    proto[:20, 0] = True
    proto[::2, 1] = True
    proto[rng.choice(F, size=13, replace=False), 2] = True
    members = {0: [2, 9, 17, 30], 1: [4, 5], 2: [11, 20, 33]}
    U = 36
    bits = _vectors(rng, F, U, 8, 32)
    for g, rs in members.items():
        bits[:, rs] = proto[:, g:g + 1]
    bits[:, 25] = ~proto[:, 0]
    pc, xyz, h_xyz = _dimer_field(bits)
    pc.ensure_labels()
    ens = EnsembleComplex((copy.copy(pc), xyz, h_xyz))
    with pytest.raises(AttributeError, match='run_coupling first'):
        ens.write_coupling(str(tmp_path))
    with pytest.raises(ValueError, match='residue'):
        ens.run_coupling([], *PASS, classes=('plane_plane',))
    with pytest.raises(ValueError, match='level'):
        ens.run_coupling([], *PASS, level='chain')
    f, p = ens.run_coupling([], *PASS, contacts=(), classes=('atom_atom',), min_occupancy=0.2, max_occupancy=0.8, min_abs_phi=0.99)
    assert ens.coupling[0] is f and ens.coupling[1] is p and ens.coupling_threshold == math.sqrt(1004 / 1024) and ens._results is None
    assert ens.stats['couple_features'] == U == len(f['a']) and f['a'].tolist() == [2 * r for r in range(U)]
    per = ens._ctx.run_models(*PASS)
    ref = reference_tables(*presence(per, ANY, 0x7F, pc.n_atoms), pc.n_atoms, 8, 32)
    assert same(f, ref['features']) and same(p, kept(ref, 1004))
    assert [g.tolist() for g in coupling.groups(f, p, n_models=F)] == [members[0], members[1], members[2]]
    assert [g.tolist() for g in coupling.groups(f, p, positive_only=False)] == [sorted(members[0] + [25]), members[1], members[2]]
    path = ens.write_coupling(str(tmp_path))
    assert os.path.basename(path) == ens.id + '.coupling'
    lines = open(path, newline='').read().split('\r\n')
    lab = export.Labels(pc, pc.component_types)
    ph = coupling.phi(f, p, F)
    assert lines[0] == ','.join(coupling.CSV_HEADER) and len(lines) == len(p['u']) + 2 and lines[-1] == ''
    for r in range(len(p['u'])):
        u, v = int(p['u'][r]), int(p['v'][r])
        assert lines[r + 1] == '%s,%s,%s,%s,%d,%d,%d,%s' % (lab.atom_macro(2 * u), lab.atom_macro(2 * u + 1), lab.atom_macro(2 * v), lab.atom_macro(2 * v + 1),
                                                             f['count'][u], f['count'][v], p['n11'][r], repr(float(ph[r]))), r
    assert set(np.round(ph, 12).tolist()) == {1.0, -1.0}
    # more kept pairs than max_pairs: the error carries the exact number
    with pytest.raises(NativeLibraryError) as e:
        ens.run_coupling([], *PASS, contacts=(), classes=('atom_atom',), min_occupancy=0.2, max_occupancy=0.8, min_abs_phi=0.99, max_pairs=3)
    assert e.value.code == _capi.ARP_E_CAPACITY and e.value.n_pairs == len(p['u'])
