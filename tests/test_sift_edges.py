"""The decision shortcuts of the per-pair kernel (k_sift) at their edges, against the oracle.

k_sift decides most pairs by shortcuts and runs the reference's operation sequence only in narrow bands around a threshold:
dist_le_fast (relative 1e-14 about thr^2), angle_ge_fast (cosine within 1e-12 of cos(a_min), |cos| within 2e-12 of 1, a
zero-length vector), angle_in_fast (1e-5), the reach bound of the `dead` mask, the escapes M_HCNT_ESC (4 or more hydrogens),
M_RAD4_ESC (a radius pair beyond table entry 14) and nbr.w == -2 (more than three bonded neighbours in other residues), and
the float32 halogen-bond angle.  tests/edge_packs.py builds inputs ON those seams (bisection on the oracle's predicates);
here the CPU tests show that the corpus is what it claims and that the two restatements of the reference (oracle/ref_c.c with
glibc, oracle/ref_py.py with NumPy) agree on it, and the GPU tests compare every record of every pack with the oracle: ids,
float32 distances, contact types and the 15-bit masks exactly.

A case on which ref_c and ref_py disagree is ambiguous between math libraries: it is printed by name and left out of the GPU
assertion; at most 1 % of a family may be left out (none is, at the time of writing)."""
import functools
import os
import pickle
import re
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'arpeggio_amd', 'csrc')
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_packs as ep      # noqa: E402

HBOND, WEAK_HBOND, XBOND, COVALENT = 1 << 5, 1 << 6, 1 << 7, 1 << 1
# the shortcuts and escapes this file covers (test_every_shortcut_is_named): name -> the family that reaches it
COVERED = {'dist_le_fast': 'family2', 'angle_ge_fast': 'family1, family4', 'angle_in_fast': 'family3',
           'M_HCNT_ESC': 'family7 (hcount)', 'M_RAD4_ESC': 'family7 (radii), family2, family5'}
REF_PY_STRIDE = {}      # family -> k: ref_py compares every k-th case only (none subsampled: the whole corpus takes ~15 s)


def _sift_names():
    from arpeggio_amd.core import config
    assert [config.SIFT_NAMES[k] for k in (1, 5, 6, 7)] == ['covalent', 'hbond', 'weak_hbond', 'xbond']


def _lookup(exp, n, pairs):
    """Rows of the (i, j)-sorted contact list for the given pairs; -1 where a pair has no record."""
    key = exp['i'].astype(np.int64) * n + exp['j']
    want = np.array([i * n + j for i, j in pairs], np.int64)
    pos = np.searchsorted(key, want)
    pos[pos >= len(key)] = 0
    return np.where(key[pos] == want, pos, -1) if len(key) else np.full(len(want), -1)


def _decisions(family, k):
    """Per case of pack k: the oracle's mask of the deciding pair (sequence-adjacent pairs included, so every case has one)."""
    p = ep.packs(family)[k]
    exp = ep.oracle_contacts(family, k, None, True)
    rows = _lookup(exp, p.pc.n_atoms, [c['pair'] for c in p.cases])
    assert (rows >= 0).all(), (family, k, [p.cases[q]['name'] for q in np.nonzero(rows < 0)[0][:5]])
    return exp['sift'][rows]


def _sides(family, k, pick, bit=None):
    """(cases with the bit set, cases without) among the cases `pick` selects."""
    p = ep.packs(family)[k]
    s = _decisions(family, k)
    idx = [q for q, c in enumerate(p.cases) if pick(c)]
    on = sum(1 for q in idx if (s[q] >> (p.cases[q]['bit'] if bit is None else bit)) & 1)
    return on, len(idx) - on


# ---- CPU: the corpus is what it claims ------------------------------------------------------------------------------------------
def _band_counts(family, k, seam, report):
    p = ep.packs(family)[k]
    out = {}
    for where, pick in (('in', lambda c: c['seam'] == seam and abs(c['margin']) < c['band']),
                        ('out', lambda c: c['seam'] == seam and abs(c['margin']) >= c['band'])):
        out[where] = _sides(family, k, pick)
    report.append(f'{p.name} {seam}: inside the band {out["in"]} (set, clear), outside {out["out"]}')
    return out


def test_corpus_reaches_every_seam_from_both_sides(capsys):
    """Per family: cases on each side of the decision (the oracle's) and inside / outside each band (float64, from the
    constants of the shortcuts) — each count non-zero; every escape is taken."""
    _sift_names()
    rep = []
    # 1: angle seams 1.57 (hbond) and 2.27 (weak), band 1e-12 in the cosine
    for seam in ('hbond', 'weak'):
        c = _band_counts('family1', 0, seam, rep)
        assert min(c['in'] + c['out']) > 0, (seam, c)
        geos = {x['name'].split('/')[2] for x in ep.packs('family1')[0].cases if x['seam'] == seam}
        assert len(geos) >= 32, (seam, len(geos))
        for orient in ('bgn', 'end'):
            assert min(_sides('family1', 0, lambda x: x['seam'] == seam and f'/{orient}/' in x['name'])) > 0, (seam, orient)
    # 2: distance seam, relative 1e-14 about thr^2; table and escaped radius, three comps
    assert [p.comp for p in ep.packs('family2')] == [0.1, 0.0, 0.2371]
    for k in range(3):
        c = _band_counts('family2', k, 'dist', rep)
        assert min(c['in'] + c['out']) > 0, (k, c)
        for esc in (False, True):
            assert min(_sides('family2', k, lambda x: x['escaped'] == esc)) > 0, (k, esc)
    # 3: both bounds of the halogen angle, band 1e-5
    for seam in ('lo', 'hi'):
        c = _band_counts('family3', 0, seam, rep)
        assert min(c['in'] + c['out']) > 0, (seam, c)
    # 4: the 2e-12 guard about |cos| = 1 from both sides, for cos = -1 (set) and cos = +1 (clear); zero-length vectors
    c = _band_counts('family4', 0, 'collinear', rep)
    assert min(c['in'] + c['out']) > 0, c
    c = _band_counts('family4', 0, 'zero', rep)
    assert min(c['out']) > 0 and sum(c['out']) == 2 * 2 * 6 * 2 + 6 * 2 * 3, c      # (band 0: every case counts as outside)
    # 5: the oracle's answer flips inside the +-12 ulp window about 1.2 + vdw + comp + |D - H|; pairs on both sides of the float32
    # reach bound; no hydrogen bond beyond it (what pruning relies on); the long hydrogen makes a bond at 4.4 A
    for k, p in enumerate(ep.packs('family5')):
        assert min(_sides('family5', k, lambda x: x['seam'] == 'seam')) > 0
        s = _decisions('family5', k)
        beyond = [q for q, x in enumerate(p.cases) if x['seam'] == 'reach' and np.float32(x['d']) > np.float32(x['reach'])]
        within = [q for q, x in enumerate(p.cases) if x['seam'] == 'reach' and np.float32(x['d']) <= np.float32(x['reach'])]
        assert beyond and within
        assert not any(s[q] & (HBOND | WEAK_HBOND) for q in beyond)
        assert min(_sides('family5', k, lambda x: x['seam'] == 'seam' and x['escaped'])) > 0
        rep.append(f'{p.name}: seam {_sides("family5", k, lambda x: x["seam"] == "seam")}, beyond the reach bound {len(beyond)}, within {len(within)}')
        h = np.linalg.norm(p.pc.h_xyz - np.repeat(p.pc.xyz.astype(np.float64), np.diff(p.pc.h_off), axis=0), axis=1)
        if k == 0:
            assert h.max() == ep.H_LONGEST
        else:
            assert 2.0 <= h.max() <= 3.0 and (h > 1.2).sum() == 2
            assert _sides('family5', k, lambda x: x['seam'] == 'long')[1] == 0
    # 6: all 1024 type pairs x 4 hydrogen placements x neighbours x 3 distances; the 'fail' copy clears a weak bit the 'ok' copy sets
    p = ep.packs('family6')[0]
    ok = [c for c in p.cases if c['seam'] == 'ok']
    assert len(ok) == 1024 * 4 * 2 * 3 and len({(c['combo'], c['hyd'], c['nbrs'], c['dist']) for c in ok}) == len(ok)
    s = _decisions('family6', 0)
    by = {(c['combo'], c['hyd'], c['dist'], c['nbrs']): s[q] for q, c in enumerate(p.cases) if c['seam'] == 'ok'}
    fail = [(q, c) for q, c in enumerate(p.cases) if c['seam'] == 'fail']
    cleared = sum(1 for q, c in fail if not s[q] & WEAK_HBOND and by[(c['combo'], c['hyd'], 3.2, True)] & WEAK_HBOND)
    assert cleared > 0 and not any(s[q] & WEAK_HBOND for q, c in fail), cleared      # (the last applicable branch decides)
    far = [q for q, c in enumerate(p.cases) if c['seam'] == 'ok' and c['dist'] == 4.3]
    assert not any(s[q] & (HBOND | WEAK_HBOND) for q in far)
    for dist in (3.2, 3.9):
        for bit in (5, 6):
            assert min(_sides('family6', 0, lambda x: x['seam'] == 'ok' and x['dist'] == dist, bit)) > 0, (dist, bit)
    rep.append(f'family6: {len(ok)} + {len(fail)} cases, {p.pc.n_atoms} atoms; last applicable weak branch fails: bit cleared in {cleared}')
    # 7: the escapes
    p = ep.packs('family7')[0]
    s = _decisions('family7', 0)
    for q, c in enumerate(p.cases):
        if c['seam'] == 'hcount':      # only the LAST hydrogen qualifies, and it does
            assert (s[q] >> c['bit']) & 1, c['name']
            i = [a for a in c['pair'] if p.pc.h_off[a + 1] - p.pc.h_off[a] == c['nh']]
            assert len(i) == 1
    assert {c['nh'] for c in p.cases if c['seam'] == 'hcount'} == {3, 4, 5, 8}
    radii = list(zip(p.pc.vdw.tolist(), p.pc.cov.tolist()))
    order = list(dict.fromkeys(radii))                          # by first appearance (arp_set_atoms); ascending = pack_blob's order
    assert len(order) >= 17 and order == sorted(order)
    entry = {r: k for k, r in enumerate(order)}
    seen = set()
    for c in p.cases:
        if c['seam'] == 'radii':
            e = tuple(entry[radii[a]] for a in c['pair'])
            seen.add(e)
            assert (max(e) >= 15) == c['escaped'] and (min(e) >= 15) == c['both_escaped'], (c['name'], e)
    assert {15, 16, 17, 18} <= {x for e in seen for x in e} and any(min(e) < 15 <= max(e) for e in seen) and any(min(e) >= 15 for e in seen)
    exp = ep.oracle_contacts('family7', 0, None, True)
    for c in p.cases:
        if c['seam'] == 'nbrs':
            rows = _lookup(exp, p.pc.n_atoms, [tuple(sorted((c['hub'], a))) for a in c['bonded'] + [c['loose']]])
            assert (rows >= 0).all()
            assert all(exp['sift'][r] & COVALENT for r in rows[:-1]) and not exp['sift'][rows[-1]] & COVALENT, c['name']
            assert abs(exp['dist'][rows[-1]] - exp['dist'][rows[:-1]]).max() < 1e-4      # (1.5 A up to the float32 rounding of coordinates of a few hundred A)
    assert {c['nn'] for c in p.cases if c['seam'] == 'nbrs'} == {3, 4, 5, 9}
    # 8: 100 000 triples, both sides, and cases within two float32 ulp of (float)2.09
    p = ep.packs('family8')[0]
    assert len(p.cases) >= 100_000
    c = _band_counts('family8', 0, 'xbond', rep)
    assert min(c['in'] + c['out']) > 0, c
    for orient in ('bgn', 'end'):
        assert min(_sides('family8', 0, lambda x: f'/{orient}/' in x['name'])) > 0
    with capsys.disabled():
        print('\n' + '\n'.join(rep))


def test_hydrogen_counts_of_the_older_fixtures():
    """No pack of tests/helpers.py has an atom with more than three hydrogens.  The M_HCNT_ESC branch of geo_atom
    (`h1 = h_off[lid + 1]`) was reached before by one GPU test, test_gpu_edge_cases.py::
    test_atoms_with_hundreds_of_hydrogens_and_bonds (it catches the `h1 = hoff + 4` mutant); family 7 adds the counts next to the
    escape (3, 4, 5, 8) with only the LAST hydrogen qualifying, in every branch kind and both orientations."""
    assert 'def test_atoms_with_hundreds_of_hydrogens_and_bonds' in open(os.path.join(ROOT, 'tests', 'test_gpu_edge_cases.py'), encoding='utf-8').read()
    from helpers import known_answer_packs, random_dense_pack, threshold_edge_pack
    most = max(int(np.diff(pc.h_off).max()) if pc.n_atoms else 0 for pc in
               [pc for _, pc in known_answer_packs()] + [random_dense_pack(s) for s in range(1, 7)] + [threshold_edge_pack()])
    assert most == 3
    assert int(np.diff(ep.packs('family7')[0].pc.h_off).max()) == 8


# ---- CPU: ref_c and ref_py agree on every decision of the corpus ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ambiguous(family):
    """{pack index: set of case indices} on which oracle/ref_c.c and oracle/ref_py.py give different records, and the number of
    cases compared."""
    from oracle import ref_py
    out, compared = {}, 0
    stride = REF_PY_STRIDE.get(family, 1)
    for k, p in enumerate(ep.packs(family)):
        exp = ep.oracle_contacts(family, k, None, True)
        rp = ref_py.RefPy(p.pc)
        idx = list(range(0, len(p.cases), stride))
        rows = _lookup(exp, p.pc.n_atoms, [p.cases[q]['pair'] for q in idx])
        bad = set()
        for q, r in zip(idx, rows):
            i, j = p.cases[q]['pair']
            got = rp.pair(i, j, p.comp, True)
            same = got is not None and r >= 0 and np.float32(got[0]).view(np.uint32) == exp['dist'][r].view(np.uint32) \
                and got[1] == exp['sift'][r] and got[2] == exp['ctype'][r]
            if not same:
                bad.add(q)
        compared += len(idx)
        out[k] = bad
    return out, compared


@pytest.mark.parametrize('family', list(ep.FAMILIES))
def test_ref_c_and_ref_py_agree_on_the_corpus(family, capsys):
    amb, compared = ambiguous(family)
    total = sum(len(p.cases) for p in ep.packs(family))
    names = [ep.packs(family)[k].cases[q]['name'] for k, bad in amb.items() for q in sorted(bad)]
    with capsys.disabled():
        print(f'\n{family}: {compared} of {total} cases compared with ref_py, {len(names)} ambiguous' + ''.join('\n  ' + n for n in names))
    assert compared >= total // REF_PY_STRIDE.get(family, 1)
    assert len(names) * 100 <= compared, f'{family}: more than 1 % of the cases are ambiguous between the two restatements'


def test_every_shortcut_is_named():
    """A new *_ESC constant in arp_pairs.h or *_fast function in arp_numerics.h fails here until this file covers it."""
    esc = set(re.findall(r'#define\s+(\w+_ESC)\b', open(os.path.join(CSRC, 'arp_pairs.h'), encoding='utf-8').read()))
    fast = set(re.findall(r'\b(\w+_fast)\s*\(', open(os.path.join(CSRC, 'arp_numerics.h'), encoding='utf-8').read()))
    assert esc and len(fast) >= 3
    missing = sorted((esc | fast) - set(COVERED))
    assert not missing, f'shortcuts without an edge test (add a family to tests/edge_packs.py and an entry to COVERED): {missing}'
    stale = sorted(set(COVERED) - esc - fast)
    assert not stale, f'shortcuts the source no longer has: {stale}'


def test_threshold_cosines_are_the_last_that_pass_in_both_restatements():
    """Inside its bands k_sift makes the reference's cosine and compares it with a constant instead of taking an acos (the device
    library's acos differs from glibc's in the last bit, which flipped one weak hydrogen bond of family 1).  Each constant of
    arp_numerics.h is the last double whose arccosine still passes its threshold, by glibc's acos (what oracle/ref_c.c links)
    and by NumPy's arccos (oracle/ref_py.py) alike, and both are monotonic for 10 000 doubles either side of it."""
    import ctypes as C
    libm = C.CDLL('libm.so.6')
    libm.acos.restype, libm.acos.argtypes = C.c_double, [C.c_double]
    src = open(os.path.join(CSRC, 'arp_numerics.h'), encoding='utf-8').read()
    consts = {k: float.fromhex(v) for k, v in re.findall(r'#define\s+ARP_COS_(\w+)\s+\(?(-?0x[0-9a-fp.+-]+)\)?', src)}
    assert set(consts) == {'LAST_GE_1_57', 'LAST_GE_2_27', 'LAST_GE_0_52', 'FIRST_LE_2_62'}, consts
    for name, passes in (('LAST_GE_1_57', lambda a: a >= 1.57), ('LAST_GE_2_27', lambda a: a >= 2.27), ('LAST_GE_0_52', lambda a: a >= 0.52),
                         ('FIRST_LE_2_62', lambda a: not a <= 2.62)):
        for acos in (libm.acos, lambda x: float(np.arccos(np.float64(x)))):
            last, _ = ep.bisect(lambda x: passes(acos(x)), -1.0, 1.0)
            if name == 'FIRST_LE_2_62':      # (bisected on the complement: the first double that passes is the next one)
                last = float(np.nextafter(last, 2.0))
            assert last == consts[name], (name, last.hex(), consts[name].hex())
            c = consts[name]
            xs = sorted(float(np.sign(c)) * ep.step_ulps(abs(c), k) for k in range(-10_000, 10_001))
            seq = np.array([acos(x) for x in xs])
            assert (np.diff(seq) <= 0).all(), name


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from arpeggio_amd import _capi
    c = _capi.Context(0)
    yield c
    c.close()


def _hex3(v):
    return ' '.join(float(x).hex() for x in v)


def _describe(p, family, i, j, got_s, exp_s):
    pc = p.pc
    q = int(pc.case_of_atom[i])
    name = p.cases[q]['name'] if q >= 0 else '(ballast)'
    hs = [f'    H of {a}: {_hex3(h)}' for a in (i, j) for h in pc.h_xyz[pc.h_off[a]:pc.h_off[a + 1]]]
    return '\n'.join([f'{family} / {p.name} case {q} {name}: pair ({i}, {j})  got {got_s}  oracle {exp_s}',
                      f'    bgn {_hex3(pc.xyz[i])}', f'    end {_hex3(pc.xyz[j])}'] + hs[:6])


def _mask(v):
    return 'none' if v is None else f'{int(v):015b}'


def _compare(p, family, k, got, exp, where):
    """Every record of the pack, exactly; ambiguous cases (ref_c != ref_py) left out.  Fails with one block per differing pair."""
    pc, n = p.pc, p.pc.n_atoms
    skip = ambiguous(family)[0].get(k, set())

    def table(c):
        keep = np.array([int(pc.case_of_atom[i]) not in skip for i in c['i']], bool) if skip else np.ones(len(c['i']), bool)
        key = c['i'].astype(np.int64)[keep] * n + c['j'][keep]
        return key, c['dist'][keep].view(np.uint32), c['sift'][keep], c['ctype'][keep]

    gk, gd, gs, gc = table(got)
    ek, ed, es, ec = table(exp)
    if np.array_equal(gk, ek) and np.array_equal(gd, ed) and np.array_equal(gs, es) and np.array_equal(gc, ec):
        return len(ek)
    g = {int(a): (int(b), int(c), int(d)) for a, b, c, d in zip(gk, gd, gs, gc)}
    e = {int(a): (int(b), int(c), int(d)) for a, b, c, d in zip(ek, ed, es, ec)}
    bad = sorted(key for key in set(g) | set(e) if g.get(key) != e.get(key))
    lines = [_describe(p, family, key // n, key % n, _mask(g[key][1]) if key in g else 'none', _mask(e[key][1]) if key in e else 'none')
             + ('' if key not in g or key not in e or (g[key][0] == e[key][0] and g[key][2] == e[key][2]) else
                f'\n    dist bits {g[key][0]:08x} / {e[key][0]:08x}, contact type {g[key][2]} / {e[key][2]}') for key in bad[:12]]
    pytest.fail(f'{where}: {len(bad)} of {len(e)} records differ from the oracle\n' + '\n'.join(lines))


def _pass(ctx, family, k, comp=None, seq=False, sel=None):
    import oracle
    p = ep.packs(family)[k]
    comp = p.comp if comp is None else comp
    ctx.set_complex(p.pc)
    masks = ctx.make_selection(sel)
    got = ctx.atom_contacts(5.0, comp, seq)
    if sel is None:
        exp = ep.oracle_contacts(family, k, comp, seq)
    else:
        oc = oracle.OracleComplex(p.pc)
        plus = oc.make_selection(sel)
        assert np.array_equal(masks['plus'], plus)
        exp = oc.atom_contacts(5.0, comp, seq)
        assert exp['err'] == 0
    return _compare(p, family, k, got, exp, f'{p.name} (comp {comp}, sequence-adjacent {seq}, {"whole" if sel is None else "partial selection"})')


def _family_test(ctx, family, more=False):
    t0 = time.time()
    records = 0
    for k in range(len(ep.packs(family))):
        records += _pass(ctx, family, k)
        if more:
            from test_gpu_paths import partial_selection
            records += _pass(ctx, family, k, seq=True)
            records += _pass(ctx, family, k, sel=partial_selection(ep.packs(family)[k].pc))
            records += _pass(ctx, family, k, seq=True, sel=partial_selection(ep.packs(family)[k].pc))
    print(f'{family}: {records} records equal to the oracle in {time.time() - t0:.1f} s')


@pytest.mark.gpu
def test_family1_hbond_angle_seam(ctx):
    _family_test(ctx, 'family1')


@pytest.mark.gpu
def test_family2_hydrogen_distance_seam(ctx):
    """Each pack at its own vdw_comp (0.1, 0.0, 0.2371), where its hydrogens sit on 1.2 + vdw + comp."""
    _family_test(ctx, 'family2')


@pytest.mark.gpu
def test_family3_halogen_weak_hbond_bounds(ctx):
    _family_test(ctx, 'family3')


@pytest.mark.gpu
def test_family4_degenerate_vectors(ctx):
    _family_test(ctx, 'family4')


@pytest.mark.gpu
def test_family5_reach_of_the_hydrogen_tests(ctx):
    """5a / 5b alone (both settings of include_sequence_adjacent, whole and under a partial selection), then 5c: the short-hydrogen
    pack in a batch beside a structure that holds a 2.5 A hydrogen, and as one of two models whose other model has one."""
    import copy
    import oracle
    from arpeggio_amd import _capi
    _family_test(ctx, 'family5', more=True)
    p, carrier = ep.packs('family5')[0], ep.long_h_carrier()
    ctx.set_batch([p.pc, carrier.pc])
    per = ctx.run_batch(5.0, p.comp, False)
    _compare(p, 'family5', 0, per[0]['atom_atom'], ep.oracle_contacts('family5', 0, p.comp, False), 'family5b in a batch')
    oc = oracle.OracleComplex(carrier.pc)
    oc.make_selection(None)
    _compare(carrier, 'family5', -1, per[1]['atom_atom'], oc.atom_contacts(5.0, p.comp, False), 'the long-hydrogen carrier in a batch')
    # two models: the second has the last donor's first hydrogen at 2.5 A
    pc = p.pc
    h2 = pc.h_xyz.copy()
    last = int(np.nonzero(np.diff(pc.h_off))[0][-1])
    h2[pc.h_off[last]] = pc.xyz[last].astype(np.float64) + [0.0, 2.5, 0.0]
    c2 = _capi.Context(0)
    try:
        c2.set_topology(pc)
        c2.set_models(np.stack([pc.xyz, pc.xyz]), np.stack([pc.h_xyz, h2]))
        per = c2.run_models(5.0, p.comp, False)
    finally:
        c2.close()
    _compare(p, 'family5', 0, per[0]['atom_atom'], ep.oracle_contacts('family5', 0, p.comp, False), 'family5b as model 1 of 2')
    pc2 = copy.copy(pc)
    pc2.h_xyz = h2
    oc = oracle.OracleComplex(pc2)
    oc.make_selection(None)
    _compare(ep.Pack('family5b+long', pc2, p.comp, p.cases), 'family5', 0, per[1]['atom_atom'], oc.atom_contacts(5.0, p.comp, False),
             'family5b with one long hydrogen as model 2 of 2')


@pytest.mark.gpu
def test_family6_applicable_and_dead_branches(ctx):
    _family_test(ctx, 'family6', more=True)


@pytest.mark.gpu
def test_family7_escapes(ctx):
    """Classic setters (radius table by first appearance) and pack_blob (sorted): the escaped radii are entries 15 .. 18 in both."""
    import oracle
    from arpeggio_amd import _capi
    _family_test(ctx, 'family7')
    p = ep.packs('family7')[0]
    ctx.set_blob(_capi.pack_blob(p.pc))
    ctx.make_selection(None)
    _compare(p, 'family7', 0, ctx.atom_contacts(5.0, p.comp, False), ep.oracle_contacts('family7', 0, p.comp, False), 'family7 by blob')


@pytest.mark.gpu
def test_family8_xbond_threshold(ctx):
    _family_test(ctx, 'family8')


@pytest.mark.gpu
def test_streaming_store_variant_on_the_seams(tmp_path):
    """Families 1 - 5 and 8 once through k_sift<1, 0> (the 'stream_out' configuration of tests/test_gpu_paths.py, its child
    runner and its comparison: the seven passes of its schedule, every record against the oracle)."""
    import test_gpu_paths as paths
    import copy
    items = []
    for f in ('family1', 'family2', 'family3', 'family4', 'family5', 'family8'):
        for k, p in enumerate(ep.packs(f)):
            pc, skip = p.pc, ambiguous(f)[0].get(k, set())
            if skip:      # the runner compares every record: the atoms of an ambiguous case lose their types (no predicate runs on them)
                pc = copy.copy(pc)
                pc.type_mask = np.where(np.isin(pc.case_of_atom, sorted(skip)), 0, pc.type_mask).astype(np.uint16)
            items.append((p.name, 'classic', pc))
    corpus = str(tmp_path / 'edges.pkl')
    with open(corpus, 'wb') as fh:
        pickle.dump(items, fh)
    npz, meta = paths.run_config('stream_out', corpus, str(tmp_path))
    try:
        bad = paths._check_child(npz, items)
    finally:
        npz.close()
    assert not bad, f'{len(bad)} differences\n' + '\n'.join(bad[:40])
