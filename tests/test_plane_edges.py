"""The decisions of the four ring / amide loops (arp_planes.h: ap_eval, pp_eval, gg_eval, gp_eval) on their seams, against the oracle.

The loops decide on folded angles that come out of an acos: theta <= 30 gates four atom - ring bits, pp_class cuts two angles at
30 / 60 / 90, the intra-residue EE skip decides whether a ring - ring record exists and which ring is bgn, and !(dih > 30 || theta > 30)
decides whether an amide record exists (float32 for amide - amide, mixed for amide - ring); they cut centre distances at 4.5 and 6.0 A
behind a tree test and candidate lists that are supersets.  tests/plane_edge_packs.py builds inputs ON those seams; here the CPU tests
show that the corpus is what it claims, that oracle/ref_c.c (glibc) and oracle/ref_py.py (NumPy) differ only on cosines where the two
acos implementations themselves decide differently (measured where the test runs, printed), and the GPU tests compare every record of
every family with oracle/ref_c.c — ids, classes, masks, contact types and existence exactly, distances as bytes, reported angles by
helpers.deg_close — with no case left out.

Measured on one MI355X against the kernels of the parent commit, which took these decisions on the device library's acos / acosf:
families A, B, E, G and H equalled the oracle; C differed in 34 of 2303 records (seams dih60, theta_ab60, theta_ba60), D in 40 of 1088
(theta on the 60 cut: a record missing, extra, or made by the other visit) and F in 129 of 669 (float32, e.g. dih150), the same counts
in a whole pass, in a batch and with each loop alone.  The float64 flips sat on the cosine 0x1p-1 exactly: glibc folds acos(0.5) to
60.00000000000001, the device library to 59.99999999999999.  The loops now decide on the reference's cosine against pinned constants
(num::fold_le, test_fold_cosines_are_the_last_that_pass), as angle_ge_exact does for k_sift; profiles/plane_edges.md has the figures."""
import ctypes as C
import functools
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import plane_edge_packs as pp      # noqa: E402
from helpers import deg_close      # noqa: E402

FAMILIES = list(pp.FAMILIES)
# loop -> (exact columns, distance column compared as bytes, angle columns compared by deg_close)
COLUMNS = {'atom_plane': (('mask', 'ctype'), 'dist', ('theta',)),
           'plane_plane': (('type1', 'type2', 'ctype'), 'dist', ('dihedral', 'theta_bgn', 'theta_end')),
           'group_group': (('ctype',), 'dist', ('dihedral', 'theta')),
           'group_plane': (('ctype',), 'dist', ('dihedral', 'theta'))}


def _libm():
    m = C.CDLL('libm.so.6')
    m.acos.restype, m.acos.argtypes = C.c_double, [C.c_double]
    m.acosf.restype, m.acosf.argtypes = C.c_float, [C.c_float]
    return m


def fold64(rad):
    """utils.py:656-660 and abs(), float64."""
    rad = np.float64(rad)
    if rad > np.pi / 2:
        rad = rad - np.pi
    return abs(rad * 180 / np.pi)


def fold32(rad):
    rad = np.float32(rad)
    if rad > np.pi / 2:
        rad = rad - np.pi
    r = rad * 180 / np.pi
    assert r.dtype == np.float32
    return abs(r)


def numpy_decides(case, which='cos'):
    """NumPy's opinion on a case's deciding cosine: folded arccos <= cut, in the case's own arithmetic."""
    c = case.get(which)
    if c is None:
        return None
    with np.errstate(all='ignore'):
        if case['path'] == 'f32':
            return bool(fold32(np.arccos(np.float32(c))) <= case['cut'])
        return bool(fold64(np.arccos(np.float64(c))) <= case['cut'])


# ---- records by case ------------------------------------------------------------------------------------------------------------------
def _records(loop, bag):
    """{(first id, second id): tuple of every column} of one bag."""
    a, b = pp.LOOPS[loop]
    cols = [k for k in bag if k not in (a, b)]
    return {(int(i), int(j)): {k: bag[k][n] for k in cols} for n, (i, j) in enumerate(zip(bag[a], bag[b]))}


def _same_record(loop, g, e):
    exact, dist, angles = COLUMNS[loop]
    if g is None or e is None:
        return g is e
    return all(g[k] == e[k] for k in exact) and np.asarray(g[dist]).tobytes() == np.asarray(e[dist]).tobytes() \
        and all(deg_close(np.asarray(g[k]), np.asarray(e[k])) for k in angles)


def _decision(case, recs):
    """What the oracle decided for a case, from its loop's records: the mask, (bgn, type1, type2) or existence."""
    i, j = case['pair']
    if case['loop'] == 'atom_plane':
        r = recs.get((i, j))
        return None if r is None else int(r['mask'])
    if case['loop'] == 'plane_plane':
        for key in ((i, j), (j, i)):
            if key in recs:
                return (key[0] == i, int(recs[key]['type1']), int(recs[key]['type2']), bool(np.isnan(recs[key]['theta_end'])))
        return None
    return (i, j) in recs


def _case_of(pc, loop, i, j):
    table = {'atom_plane': pc.case_of_ring, 'plane_plane': pc.case_of_ring, 'group_group': pc.case_of_amide, 'group_plane': pc.case_of_amide}[loop]
    return int(table[i])


def _hex3(v):
    return ' '.join(float(x).hex() for x in v)


def _describe(p, loop, key, g, e):
    """One block per differing record: the case, both records, the inputs as hex floats, the oracle's cosine and NumPy's decision."""
    pc = p.pc
    q = _case_of(pc, loop, *key)
    case = p.cases[q] if q >= 0 else dict(name='(no case)')
    lines = [f'{p.name} case {q} {case["name"]}: {loop} record {key}', f'    got    {g}', f'    oracle {e}']
    for r in case.get('rings', []):
        lines.append(f'    ring {r}: centre {_hex3(pc.ring_center[r])}  normal {_hex3(pc.ring_normal[r])}  residue {int(pc.ring_res[r])}')
    for a in case.get('amides', []):
        lines.append(f'    amide {a}: centre {_hex3(pc.amide_center[a])}  normal {_hex3(pc.amide_normal[a])}')
    for a in case.get('atoms', []):
        lines.append(f'    atom {a}: {_hex3(pc.xyz[a])}  types {int(pc.type_mask[a]):#06x} flags {int(pc.flags[a]):#04x}')
    for which in ('cos', 'cos_b'):
        if case.get(which) is not None:
            lines.append(f'    oracle {which} {float(case[which]).hex()} ({case["path"]}, cut {case["cut"]}): NumPy decides folded arccos <= cut = '
                         f'{numpy_decides(case, which)}')
    return '\n'.join(lines)


def compare(p, got, exp, where):
    """Every record of every loop of a pack against the oracle's; returns the number of records compared, fails with one block per
    differing record.  Nothing is left out."""
    bad, n = [], 0
    for loop, (exact, dist, angles) in COLUMNS.items():
        a, b = pp.LOOPS[loop]
        g, e = got[loop], exp[loop]
        n += len(e[a])
        if len(g[a]) == len(e[a]) and all(np.array_equal(g[k], e[k]) for k in (a, b) + exact) \
                and np.asarray(g[dist]).tobytes() == np.asarray(e[dist]).tobytes() and all(deg_close(g[k], e[k]) for k in angles):
            continue
        gr, er = _records(loop, g), _records(loop, e)
        for key in sorted(set(gr) | set(er)):
            if not _same_record(loop, gr.get(key), er.get(key)):
                bad.append(_describe(p, loop, key, gr.get(key), er.get(key)))
    if bad:
        pytest.fail(f'{where}: {len(bad)} of {n} records differ from the oracle\n' + '\n'.join(bad[:12]))
    return n


def _ulps(a, b, path):
    if path == 'f32':
        return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


# ---- CPU: the corpus is what it claims ------------------------------------------------------------------------------------------------------
def test_corpus_reaches_every_seam_from_both_sides(capsys):
    """Per family and seam: cases on both sides of the oracle's decision, at least 16 geometries where the seam is bisected, and a pair
    of cases on opposite sides whose oracle cosines are within 4 ulps (float64 and the mixed path) or 2 ulps (float32); every bit, class
    and orientation outcome occurs; every case is more than 13 A from every other."""
    rep, masks, classes, type2, created = [], set(), set(), set(), set()
    for f in FAMILIES:
        p = pp.packs(f)
        pc = p.pc
        recs = {loop: _records(loop, bag) for loop, bag in pp.oracle_bags(f).items()}
        # isolation: all items of a case near its origin, origins 24 A apart
        pts = np.concatenate([pc.xyz.astype(np.float64), pc.ring_center, pc.amide_center.astype(np.float64)])
        case = np.concatenate([pc.case_of_atom, pc.case_of_ring, pc.case_of_amide])
        assert (case >= 0).all()
        org = np.array([[0.0, 24.0 * (q % 48), 24.0 * (q // 48)] for q in range(len(p.cases))])
        assert np.linalg.norm(pts - org[case], axis=1).max() < 5.5, f       # two cases: at least 24 - 2 x 5.5 = 13 A apart
        seams = {}
        for q, c in enumerate(p.cases):
            seams.setdefault(c['seam'], []).append((c, _decision(c, recs[c['loop']])))
        for seam, lst in seams.items():
            sides = {d for _, d in lst}
            line = f'{p.name} {seam}: {len(lst)} cases, decisions {len(sides)}'
            labelled = f == 'H' or seam in ('tree',) or seam.endswith(('superset', 'fold', 'coincident', 'zero_normal', 'right'))
            if not labelled:
                assert len(sides) >= 2, (f, seam, sides)
            if any('/geo' in c['name'] for c, _ in lst) and not labelled:
                geos = {c['name'].split('/geo')[1].split('/')[0] for c, _ in lst}
                assert len(geos) >= 16, (f, seam, len(geos))
                # (the mixed path is held to the float64 bound on the seams that move its float64 side, `*_ring`; where a float32
                # component moves, neighbouring cosines are a float32 step apart and the float32 bound applies to them as float32)
                if lst[0][0].get('cos') is not None:
                    path = lst[0][0]['path']
                    if path == 'mix' and not seam.endswith('_ring'):
                        path = 'f32'
                    best = min((_ulps(c1[which], c2[which], path) for which in ('cos', 'cos_b') for c1, d1 in lst for c2, d2 in lst
                                if c1.get(which) is not None and d1 != d2 and c1['name'].split('/ulp')[0] == c2['name'].split('/ulp')[0]), default=None)
                    assert best is not None and best <= (2 if path == 'f32' else 4), (f, seam, best)
                    line += f', closest cosines on opposite sides {best} ulp ({path})'
            rep.append(line)
            for c, d in lst:
                if c['loop'] == 'atom_plane' and d is not None:
                    masks.add(d)
                if c['loop'] == 'plane_plane' and d is not None:
                    classes.add(d[1])
                    type2.add('same' if d[2] == 254 else 'skipped' if d[2] == 255 else "''" if d[2] == 9 else 'different')
                    if f == 'D':
                        created.add('reverse' if not d[0] else 'forward')
                        assert d[0] or (d[2] == 255 and d[3]), c['name']      # made by the reverse visit: bgn / end swapped, theta_end NaN
                if f == 'D' and d is None:
                    created.add('none')
        if f == 'B':
            labels = {c['label'] for c in p.cases if c['seam'] == 'tree'}
            # both orders of disagreement between the tree's plain sum and the FMA-chained norm, and neither makes a record
            assert {'tree_only', 'norm_only', 'agree'} <= labels, labels
            for c in p.cases:
                if c['seam'] == 'tree' and c['label'] != 'agree':
                    assert _decision(c, recs['atom_plane']) is None, c['name']
        if f == 'E':
            for loop in ('plane_plane', 'group_plane', 'group_group'):
                labels = [c['label'] for c in p.cases if c['seam'] == f'{loop}/superset']
                assert labels.count('on_list') >= 6 and labels.count('beyond') >= 6 and 'inside' not in labels, (loop, labels)
            assert not any(_decision(c, recs[c['loop']]) for c in p.cases if c['seam'].endswith('superset'))
        if f == 'H':
            for loop in pp.LOOPS:
                for q_ in ('dih', 'theta'):
                    got = {c['label'] for c in p.cases if c['seam'] == f'{loop}/{q_}'}
                    if loop == 'atom_plane' and q_ == 'dih':
                        continue
                    assert got == {'inside', 'one', 'beyond'}, (loop, q_, got)
            for c in p.cases:      # beyond 1: NaN, then class '' / a record all the same / no gated bit
                if c.get('label') == 'beyond':
                    d = _decision(c, recs[c['loop']])
                    ok = d == 16 if c['loop'] == 'atom_plane' else (d is not None and 9 in d[1:3]) if c['loop'] == 'plane_plane' else d is True
                    assert ok, (c['name'], d)
    assert {1, 2, 4, 8, 15, 16} <= masks, masks
    assert classes == set(range(10)), classes
    assert type2 == {'same', 'different', 'skipped', "''"}, type2
    assert created == {'forward', 'reverse', 'none'}, created
    with capsys.disabled():
        print('\n' + '\n'.join(rep))


# ---- CPU: ambiguity between the two math libraries is accounted for ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ambiguous_cosines():
    """{(path, cut, folded): set of cosines} on which glibc's acos / acosf and NumPy's arccos decide `folded angle <= cut` differently:
    +-2000 doubles and +-200 floats about cos 30 / 60 / 120 / 150 degrees (mixed arithmetic takes the float64 acos)."""
    m = _libm()
    out = {}
    for deg in (30, 60, 120, 150):
        cut, c0 = float(min(deg, 180 - deg)), float(np.cos(np.deg2rad(deg)))
        xs = [pp.step64(c0, k) for k in range(-2000, 2001)]
        with np.errstate(all='ignore'):
            dg = [fold64(m.acos(x)) <= cut for x in xs]
            dn = [fold64(np.arccos(np.float64(x))) <= cut for x in xs]
            out[('f64', cut, deg > 90)] = {x for x, a, b in zip(xs, dg, dn) if a != b}
            assert sum(a != b for a, b in zip(dg, dg[1:])) == 1, deg           # glibc: monotonic in the window, one flip
            xs = [float(pp.step32(np.float32(c0), k)) for k in range(-200, 201)]
            dg = [fold32(m.acosf(x)) <= cut for x in xs]
            dn = [fold32(np.arccos(np.float32(x))) <= cut for x in xs]
            out[('f32', cut, deg > 90)] = {x for x, a, b in zip(xs, dg, dn) if a != b}
            assert sum(a != b for a, b in zip(dg, dg[1:])) == 1, deg
    assert fold64(m.acos(0.0)) == 90.0 and fold32(m.acosf(0.0)) == 90.0 and fold64(np.arccos(0.0)) == 90.0 and fold32(np.arccos(np.float32(0))) == 90.0
    return out


@functools.lru_cache(maxsize=None)
def ref_py_bags(family):
    from oracle import ref_py
    rp = ref_py.RefPy(pp.packs(family).pc)
    out = {}
    for loop, order in pp.LOOPS.items():
        e = getattr(rp, loop)()
        o = np.lexsort((e[order[1]], e[order[0]]))
        out[loop] = {k: v[o] for k, v in e.items()}
    return out


def test_ref_c_and_ref_py_differ_only_where_the_two_acos_do(capsys):
    """The sets of cosines on which the libraries decide differently are measured here (at most 2 per cut and dtype path; 0 or 1 were
    measured) and printed.  A case on which ref_c and ref_py give different records must have a deciding cosine in its set: any other
    difference is a bug in a restatement."""
    amb = ambiguous_cosines()
    rep = ['cosines on which glibc and NumPy decide differently:']
    for key, xs in sorted(amb.items()):
        assert len(xs) <= 2, (key, xs)
        rep.append(f'  {key[0]} cut {key[1]:g}{" (folded)" if key[2] else ""}: {sorted(float(x).hex() for x in xs) or "none"}')
    t0, total, unexplained = time.time(), 0, []
    for f in FAMILIES:
        p = pp.packs(f)
        c_bags, py_bags = pp.oracle_bags(f), ref_py_bags(f)
        differing = []
        for loop in pp.LOOPS:
            cr, pr = _records(loop, c_bags[loop]), _records(loop, py_bags[loop])
            total += len(cr)
            for key in sorted(set(cr) | set(pr)):
                if not _same_record(loop, pr.get(key), cr.get(key)):
                    differing.append((loop, key, pr.get(key), cr.get(key)))
        names = set()
        for loop, key, g, e in differing:
            case = p.cases[_case_of(p.pc, loop, *key)]
            path = 'f32' if case['path'] == 'f32' else 'f64'
            explained = any(case.get(w) is not None and float(case[w]) in amb.get((path, float(case['cut']), float(case[w]) < 0), ())
                            for w in ('cos', 'cos_b'))
            names.add(case['name'] + ('' if explained else '  UNEXPLAINED'))
            if not explained:
                unexplained.append(_describe(p, loop, key, g, e).replace('got   ', 'ref_py'))
        rep.append(f'{p.name}: {len(p.cases)} cases, ref_c != ref_py on {len(names)}' + ''.join('\n    ' + n for n in sorted(names)))
    rep.append(f'{total} records compared in {time.time() - t0:.1f} s')
    with capsys.disabled():
        print('\n' + '\n'.join(rep))
    assert not unexplained, f'{len(unexplained)} differences between ref_c and ref_py outside the ambiguous cosines\n' + '\n'.join(unexplained[:8])


def test_the_comparison_leaves_no_case_out():
    """The GPU tests' comparison counts every record of every case and fails on one changed class, one missing record and one swapped
    orientation, naming the case.  The yardstick is oracle/ref_c.c: deterministic, and what the pinned constants are held against."""
    for f in FAMILIES:
        p, exp = pp.packs(f), pp.oracle_bags(f)
        assert compare(p, exp, exp, f) == sum(len(exp[loop][pp.LOOPS[loop][0]]) for loop in pp.LOOPS)
        seen = {_case_of(p.pc, loop, int(i), int(j)) for loop in pp.LOOPS for i, j in zip(*(exp[loop][k] for k in pp.LOOPS[loop]))}
        assert len(seen) >= len(p.cases) // 4 and -1 not in seen, f            # (the other cases decide that there is no record)
    p, exp = pp.packs('D'), pp.oracle_bags('D')
    for change in ('class', 'missing', 'swapped'):
        bag = {k: v.copy() for k, v in exp['plane_plane'].items()}
        if change == 'class':
            bag['type1'][5] = (bag['type1'][5] + 1) % 9
        elif change == 'missing':
            bag = {k: np.delete(v, 5) for k, v in bag.items()}
        else:
            bag['bgn'][5], bag['end'][5] = bag['end'][5], bag['bgn'][5]
        with pytest.raises(pytest.fail.Exception, match=r'planes_D case \d+ D/'):
            compare(p, dict(exp, plane_plane=bag), exp, change)


# ---- CPU: the pinned cosines of the kernels' decisions ---------------------------------------------------------------------------------
CSRC = os.path.join(ROOT, 'arpeggio_amd', 'csrc')


def _bisect_cos(passes, lo, hi, single):
    """passes(lo) true, passes(hi) false -> the last value on lo's side that passes (doubles, or floats when single)."""
    assert passes(lo) and not passes(hi)
    while True:
        mid = float(np.float32(lo) + (np.float32(hi) - np.float32(lo)) / np.float32(2)) if single else lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            return lo
        if passes(mid):
            lo = mid
        else:
            hi = mid


def test_fold_cosines_are_the_last_that_pass(capsys):
    """ap_eval, pp_eval, gg_eval and gp_eval decide `folded angle <= cut` on the reference's cosine against constants of arp_numerics.h.
    Each is re-derived here by bisection on glibc's acos / acosf (what oracle/ref_c.c links) through the reference's fold: the smallest
    cosine that passes without the fold and the largest that passes through it, for 30 and 60 in float64 and 30 in float32, and the
    decision is monotonic for 10 000 values either side.  Where NumPy's last passing cosine is another one it is printed, not failed:
    which it is depends on the SIMD path NumPy takes on the CPU at hand."""
    import re
    m = _libm()
    src = open(os.path.join(CSRC, 'arp_numerics.h'), encoding='utf-8').read()
    consts = {k: float.fromhex(v) for k, v in re.findall(r'#define\s+ARP_FOLD_(COSF?_\w+)\s+\(?(-?0x[0-9a-fp.+-]+?)f?\)?\s', src)}
    assert set(consts) == {'COS_30_POS', 'COS_30_NEG', 'COS_60_POS', 'COS_60_NEG', 'COSF_30_POS', 'COSF_30_NEG'}, consts
    rep = []
    with np.errstate(all='ignore'):
        for name, c in sorted(consts.items()):
            single, cut, pos = name.startswith('COSF'), float(name.split('_')[1]), name.endswith('POS')
            if single:
                libs = (('glibc', lambda x: fold32(m.acosf(x)) <= cut), ('NumPy', lambda x: fold32(np.arccos(np.float32(x))) <= cut))
                step = lambda x, k: float(pp.step32(np.float32(x), k))
                assert float(np.float32(c)) == c
            else:
                libs = (('glibc', lambda x: fold64(m.acos(x)) <= cut), ('NumPy', lambda x: fold64(np.arccos(np.float64(x))) <= cut))
                step = pp.step64
            for lib, passes in libs:
                last = _bisect_cos(passes, 1.0 if pos else -1.0, 0.0 if pos else -2.0 ** -10, single)
                if lib == 'glibc':
                    assert last == c, (name, last.hex(), c.hex())
                    # k > 0 steps away from zero: towards +-1, where the folded angle shrinks
                    seq = [passes(step(c, k)) for k in range(-10_000, 10_001)]
                    assert seq == [False] * 10_000 + [True] * 10_001, name
                elif last != c:
                    rep.append(f'{name}: NumPy\'s last passing cosine is {last.hex()}, glibc\'s {c.hex()}')
    with capsys.disabled():
        print('\n' + ('\n'.join(rep) if rep else 'NumPy and glibc have the same six last passing cosines'))


def test_no_decision_on_a_folded_angle_from_acos():
    """The twin of test_sift_edges.py::test_every_shortcut_is_named for the ring / amide loops.  In arp_planes.h and arp_numerics.h:
    no comparison has a degree cut (30 / 60 / 90, as a literal in either operand position) on one side, and no constant or variable is
    defined as one; fold_deg(acos ..), the reported angle, is made in arp_planes.h only, each result goes into a local whose only uses are
    assignments to the record (rec.d*), and arp_numerics.h hands no folded angle back from any function.  A decision therefore goes
    through fold_le / fold_num on the cosine, which this file covers (families A, C, D, F, G, H)."""
    import re
    code = {name: re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, name), encoding='utf-8').read()) for name in ('arp_planes.h', 'arp_numerics.h')}
    cut = r'\(?\s*(?:\(\s*(?:float|double)\s*\))?\s*(?:30|60|90)(?:\.0*)?f?\s*\)?'
    for name, text in code.items():
        hits = re.findall(rf'[^\n]*(?:(?:[<>]=?|[=!]=)\s*{cut}(?![\w.])|(?<![\w.]){cut}\s*(?:[<>]=?|[=!]=))[^\n]*', text)
        hits += re.findall(rf'[^\n]*(?:#define\s+\w+\s+|\b(?:double|float)\s+\w+\s*=\s*){cut}\s*;?\s*(?=\n)', text)
        assert not hits, f'{name} holds a degree cut (decide on the cosine with fold_le and add the case to tests/plane_edge_packs.py): {hits}'
    planes, numerics = code['arp_planes.h'], code['arp_numerics.h']
    # arp_numerics.h: acos feeds get_angle (k_sift's reported-free radian angles, covered by test_sift_edges.py) and nothing that folds
    assert not re.search(r'fold_deg\s*\(\s*acosf?', numerics) and 'group_angle' not in numerics and 'group_angle' not in planes
    for fn in re.findall(r'__device__[^;{]*?\b(\w+)\s*\([^)]*\)\s*\{[^}]*fold_deg[^}]*\}', numerics):
        assert fn == 'fold_deg', f'arp_numerics.h: {fn} returns a folded angle'
    calls = re.findall(r'\bacosf?\s*\(', planes)
    made = re.findall(r'\b(\w+)\s*=\s*num::fold_deg\(acosf?\(\w+\)\)', planes)
    assert len(calls) == len(made) == 8, (len(calls), made)          # theta | dih, t_ab, t_ba | dih, theta | dih, theta
    for var in sorted(set(made) | {'t1', 't2'}):          # (t1 / t2: the two thetas of a ring - ring record in the order of its ids)
        for line in planes.split('\n'):
            if not re.search(rf'\b{var}\b', line) or re.search(rf'\b{var}\s*=\s*num::fold_deg\(', line) or re.fullmatch(r'\s*double t1, t2;\s*', line):
                continue
            stmts = [x.strip() for x in line.split(';') if x.strip()]
            ok = all(re.fullmatch(r'(?:rec\.d\d|t[12]) = [^<>=!&|]*', x) for x in stmts)
            assert ok, f'arp_planes.h: the reported angle {var} is used outside the record: {line.strip()}'


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from arpeggio_amd import _capi
    c = _capi.Context(0)
    yield c
    c.close()


def _fetch(ctx):
    return {loop: ctx.fetch_bag(loop, sort=True) for loop in pp.LOOPS}


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
def test_family_whole_and_under_a_partial_selection(ctx, family):
    """A whole pass (arp_run_launch: the candidate lists in the leading blocks of k_sift_planes), then the pass under the pack's partial
    selection: the first item of every case selected, the other in selection_plus only, so every contact type is INTER (family D's two
    rings share a residue and are both selected)."""
    import oracle
    p = pp.packs(family)
    t0 = time.time()
    ctx.set_complex(p.pc)
    ctx.run_launch()
    n = compare(p, _fetch(ctx), pp.oracle_bags(family), f'{p.name}, whole structure')
    masks = ctx.make_selection(p.pc.partial_selection)
    oc = oracle.OracleComplex(p.pc)
    assert np.array_equal(masks['plus'], oc.make_selection(p.pc.partial_selection))
    assert np.array_equal(masks['ring_sel'], oc.ring_sel) and np.array_equal(masks['amide_plus'], oc.amide_plus)
    ctx.run_launch()
    exp = pp.oracle_bags(family, True)
    # the second item of every case reaches selection_plus: the same pairs have a record as in the whole structure, and (but for
    # family D, whose two rings share the selected residue) every one of them lies between the selection and the rest
    whole = pp.oracle_bags(family)
    for loop, (a, b) in pp.LOOPS.items():
        assert np.array_equal(exp[loop][a], whole[loop][a]) and np.array_equal(exp[loop][b], whole[loop][b]), loop
        assert family == 'D' or (exp[loop]['ctype'] == 2).all(), loop
    assert sum(len(exp[loop]['ctype']) for loop in pp.LOOPS) > 0
    n += compare(p, _fetch(ctx), exp, f'{p.name}, partial selection')
    print(f'{p.name}: {n} records equal to the oracle in {time.time() - t0:.1f} s')


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['A', 'C', 'D', 'F', 'H'])
def test_family_in_a_batch_beside_an_unrelated_structure(ctx, family):
    import oracle
    p, other = pp.packs(family), pp.unrelated_structure()
    ctx.set_batch([p.pc, other])
    per = ctx.run_batch()
    compare(p, per[0], pp.oracle_bags(family), f'{p.name} as structure 1 of a batch of 2')
    oc = oracle.OracleComplex(other)
    oc.make_selection(None)
    exp = {}
    for loop, order in pp.LOOPS.items():
        e = getattr(oc, loop)()
        o = np.lexsort((e[order[1]], e[order[0]]))
        exp[loop] = {k: v[o] for k, v in e.items()}
    other.case_of_ring = np.full(other.n_rings, -1)
    other.case_of_amide = np.full(other.n_amides, -1)
    compare(pp.Pack('unrelated', other, 0.1, []), per[1], exp, 'the unrelated structure as structure 2 of a batch of 2')


_CHILD = '''
import pickle, sys
import numpy as np
sys.path.insert(0, %r)
from arpeggio_amd import _capi
packs = pickle.load(open(sys.argv[1], 'rb'))
out = {}
c = _capi.Context(0)
for name, pc in packs:
    c.set_complex(pc)
    for loop, order in %r.items():
        c.launch_bag(loop)
        for k, v in c.fetch_bag(loop, sort=True).items():
            out[name + ':' + loop + ':' + k] = v
c.close()
np.savez(sys.argv[2], **out)
'''


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['0', '15'])
def test_each_loop_alone_by_its_grid_walk_and_from_its_list(tmp_path, mode):
    """arp_*_launch alone on every family, ARP_BAG_LISTS=0 (every loop by its grid walk) and =15 (every loop from its candidate list), in a
    fresh process each: the switch is read once.  One GPU child at a time, under a time limit."""
    corpus, result = str(tmp_path / 'packs.pkl'), str(tmp_path / 'bags.npz')
    with open(corpus, 'wb') as fh:
        pickle.dump([(f, pp.packs(f).pc) for f in FAMILIES], fh)
    r = subprocess.run([sys.executable, '-c', _CHILD % (ROOT, pp.LOOPS), corpus, result], env=dict(os.environ, ARP_BAG_LISTS=mode),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(result) as z:
        for f in FAMILIES:
            got = {loop: {k.split(':')[2]: z[k] for k in z.files if k.startswith(f'{f}:{loop}:')} for loop in pp.LOOPS}
            compare(pp.packs(f), got, pp.oracle_bags(f), f'{pp.packs(f).name}, each loop alone, ARP_BAG_LISTS={mode}')
