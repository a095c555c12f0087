"""Seam corpus of the four ring / amide loops (arp_planes.h: ap_eval, pp_eval, gg_eval, gp_eval), built on the CPU.

Every case is an isolated group (two rings, two amides, an amide and a ring, or an atom and a ring) on a flat lattice of
24 A pitch, so a wrong class, mask or record points at one case and a case makes one deciding record at most.  Rings and
amides go in as centre / normal arrays.  Each ring / amide has a residue of its own (family D: one for both rings) whose
only atom is a typeless carrier at the case's origin: it makes the item a member of the selection (or of selection_plus)
and takes part in nothing else.

Seam positions are found by bisection on the ORACLE's arithmetic (the C entry points under OracleComplex.atom_plane() ...
group_plane(): orc_group_angle_*, orc_norm_*, orc_dot_*) in a random frame that is along no axis; no kernel code is
restated here and the expected records always come from the oracle's loops over the whole pack.  Lattice origins are
integers with x = 0 and every offset from them that is not the bisected quantity is a multiple of 2^-12, so the differences
the loops take are the same at every origin: a seam is bisected once per geometry and its cases (the flip and 1, 2, 3, 8,
64 and 4096 ulps either side of it) sit on origins of their own.  float64 inputs: the bisected quantity is an angle of the
construction or the x coordinate of a centre; float32 inputs: the bit pattern of one float32 component.

packs(family) -> Pack (edge_packs.Pack: pc, cases).  A case: dict(name, seam, loop, k = offset in ulps, rings / amides /
atoms = the ids of its items, pair = the ids of the deciding record in its loop's (first, second) columns, decides = what
the seam decides, cos = the oracle's deciding cosine where there is one, path = 'f64' | 'f32' | 'mix', cut = 30 | 60)."""
import functools

import numpy as np

from edge_packs import Builder, Pack, _lib, _types, _vp, bisect, frame
from helpers import tiny_complex

OFFSETS = (0, 1, -1, 2, -2, 3, -3, 8, -8, 64, -64, 4096, -4096)
N_GEO = 16
DEG = np.pi / 180.0
LOOPS = {'atom_plane': ('ring', 'atom'), 'plane_plane': ('bgn', 'end'), 'group_group': ('bgn', 'end'), 'group_plane': ('amide', 'ring')}


def quant(v):
    return np.round(np.asarray(v, np.float64) * 4096.0) / 4096.0


def f64(v):
    return np.ascontiguousarray(v, np.float64)


def f32(v):
    return np.ascontiguousarray(v, np.float32)


# ---- the oracle's arithmetic ----------------------------------------------------------------------------------------------------
def ga64(n, p):
    return _lib().orc_group_angle_f64(_vp(f64(n)), _vp(f64(p)))


def ga32(n, p):
    return np.float32(_lib().orc_group_angle_f32(_vp(f32(n)), _vp(f32(p))))


def gamix(n, p):
    return _lib().orc_group_angle_f32n_f64p(_vp(f32(n)), _vp(f64(p)))


def norm64(v):
    return _lib().orc_norm_f64(_vp(f64(v)))


def norm32(v):
    return np.float32(_lib().orc_norm_f32(_vp(f32(v))))


def cos64(n, p):
    """The cosine the float64 loops hand to acos: dot / (norm * norm), every step the oracle's."""
    n, p = f64(n), f64(p)
    with np.errstate(all='ignore'):
        return float(np.float64(_lib().orc_dot_f64(_vp(n), _vp(p))) / np.float64(norm64(n) * norm64(p)))


def cos32(n, p):
    n, p = f32(n), f32(p)
    with np.errstate(all='ignore'):
        return np.float32(_lib().orc_dot_f32(_vp(n), _vp(p))) / (norm32(n) * norm32(p))


def cosmix(n, p):
    n, p = f32(n), f64(p)
    with np.errstate(all='ignore'):
        return float(np.float64(_lib().orc_dot_f64(_vp(n.astype(np.float64)), _vp(p))) / np.float64(float(norm32(n)) * norm64(p)))


def kd2(a, b):
    """Bio.PDB.kdtrees membership: float64 sum of squares, one rounding per operation."""
    d = [float(x) - float(y) for x, y in zip(a, b)]
    r = d[0] * d[0]
    r += d[1] * d[1]
    r += d[2] * d[2]
    return r


def step64(x, k):
    """The double k ulps from x in magnitude (k > 0: away from zero)."""
    return float(np.copysign((np.array([abs(x)], np.float64).view(np.int64) + np.int64(k)).view(np.float64)[0], x))


def step32(x, k):
    return np.float32(np.copysign((np.array([abs(x)], np.float32).view(np.int32) + np.int32(k)).view(np.float32)[0], x))


def bisect_bits32(pred, lo, hi):
    """pred(lo) true, pred(hi) false, lo and hi float32 of one sign -> adjacent float32 (lo, hi) with the same."""
    lo, hi = np.float32(lo), np.float32(hi)
    assert pred(lo) and not pred(hi) and np.sign(lo) == np.sign(hi) != 0
    a, b = int(np.abs(lo).view(np.int32)), int(np.abs(hi).view(np.int32))
    sg = np.sign(lo)

    def val(i):
        return np.float32(sg) * np.array([i], np.int32).view(np.float32)[0]

    while abs(a - b) > 1:
        m = (a + b) // 2
        if pred(val(m)):
            a = m
        else:
            b = m
    return val(a), val(b)


def pair_normals(fr, ta, tb, dl):
    """Unit normals na, nb: na at the angle ta from u (the centre line), nb at tb from u and at dl from na."""
    u, w, n = fr
    na = np.cos(ta) * u + np.sin(ta) * w
    cpsi = (np.cos(dl) - np.cos(ta) * np.cos(tb)) / (np.sin(ta) * np.sin(tb))
    assert abs(cpsi) <= 1.0, (ta / DEG, tb / DEG, dl / DEG)
    spsi = np.sqrt(1.0 - cpsi * cpsi)
    return na, np.cos(tb) * u + np.sin(tb) * (cpsi * w + spsi * n)


def feasible_dl(ta, tb, dl):
    """dl, or its folded twin pi - dl, whichever the two angles from the centre line allow."""
    for d in (dl, np.pi - dl):
        c = (np.cos(d) - np.cos(ta) * np.cos(tb)) / (np.sin(ta) * np.sin(tb))
        if abs(c) <= 0.98:
            return d
    raise AssertionError((ta / DEG, tb / DEG, dl / DEG))


def far_tb(ta, dl):
    """An angle of the second normal from the centre line that the other two allow and whose folded value is far from 30."""
    lo, hi = abs(ta - dl) + 4 * DEG, min(ta + dl, 2 * np.pi - ta - dl) - 4 * DEG      # (4 degrees of room: the seams move ta or dl by up to 3)
    cands = [0.5 * (lo + hi), lo, hi]
    return max(cands, key=lambda t: min(t, np.pi - t) / DEG - 30.0 if min(t, np.pi - t) / DEG > 30.0 else -1.0)


def side_range(target_deg, width=1.0):
    """(true side, false side) of `folded angle <= cut` about a target angle of the construction, in radians."""
    if target_deg < 90:
        return (target_deg - width) * DEG, (target_deg + width) * DEG
    return (target_deg + width) * DEG, (target_deg - width) * DEG


def x_frame(rng):
    while True:
        fr = frame(rng)
        if abs(fr[0][0]) > 0.4:
            return fr


class PlaneBuilder(Builder):
    def __init__(self):
        super().__init__(pitch=24.0, side=48, flat=True)
        self.rc, self.rn, self.rr, self.ac, self.an, self.ar = [], [], [], [], [], []
        self.case_of_ring, self.case_of_amide, self.first_carrier = [], [], []
        self._o, self._ncar = None, 0

    def begin(self):
        self._o, self._ncar = self.origin(), 0
        self.begin_case()
        return self._o

    def carrier(self):
        i = self.atom(self._o + [0.0, 0.25 * self._ncar, 0.0])
        if self._ncar == 0:
            self.first_carrier.append(i)
        self._ncar += 1
        return self.res[i]

    def ring(self, c, n, res=None):
        self.rc.append(f64(c)); self.rn.append(f64(n)); self.rr.append(self.carrier() if res is None else res)
        self.case_of_ring.append(self._case)
        return len(self.rc) - 1

    def amide(self, c, n, res=None):
        self.ac.append(f32(c)); self.an.append(f32(n)); self.ar.append(self.carrier() if res is None else res)
        self.case_of_amide.append(self._case)
        return len(self.ac) - 1

    def end(self, name, seam, loop, pair, **kw):
        self.cases.append(dict(name=name, seam=seam, loop=loop, pair=tuple(pair), **kw))
        self._case = -1

    def build(self, name):
        z = np.zeros
        pc = tiny_complex(np.array(self.xyz, np.float32).reshape(-1, 3), type_mask=np.array(self.tm, np.uint16), flags=np.array(self.fl, np.uint16),
                          res_id=np.array(self.res, np.int32),
                          rings=(np.array(self.rc, np.float64).reshape(-1, 3), np.array(self.rn, np.float64).reshape(-1, 3), np.array(self.rr, np.int32)),
                          amides=(np.array(self.ac, np.float32).reshape(-1, 3), np.array(self.an, np.float32).reshape(-1, 3), np.array(self.ar, np.int32)))
        pc.case_of_atom = np.array(self.case_of_atom, np.int32)
        pc.case_of_ring = np.array(self.case_of_ring, np.int32) if self.rc else z(0, np.int32)
        pc.case_of_amide = np.array(self.case_of_amide, np.int32) if self.ac else z(0, np.int32)
        sel = z(pc.n_atoms, np.uint8)
        sel[self.first_carrier] = 1
        pc.partial_selection = sel          # the first item of every case selected, the others reach selection_plus only
        pc.id = name
        return Pack(name, pc, 0.1, self.cases)


def _atom_kinds():
    T, config = _types()
    four = T['weak hbond donor'] | T['pos ionisable'] | T['hbond donor'] | T['xbond donor']
    return {'carbon': (T['weak hbond donor'], config.F_ELEM_C, 1), 'cation': (T['pos ionisable'], 0, 2), 'donor': (T['hbond donor'], 0, 4),
            'halogen': (T['xbond donor'], 0, 8), 'all': (four, config.F_ELEM_C, 15),
            'met': (0, config.F_RES_MET | config.F_ELEM_S, 16), 'all+met': (four, config.F_RES_MET | config.F_ELEM_S, 14 | 16)}


# ---- family A: the atom - ring angle (I:1005-1007) ---------------------------------------------------------------------------------
def family_a(seed=201):
    """theta about 30 and, through the fold, about 150 at 3.5 A; the rotation angle of the normal is bisected."""
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    kinds = _atom_kinds()
    for target in (30, 150):
        for g in range(20):
            kind = ('carbon', 'cation', 'donor', 'halogen', 'all')[g % 5]
            tm, fl, bits = kinds[kind]
            u, w, _ = frame(rng)
            half, s = quant(1.75 * u), rng.uniform(0.5, 2.0)
            point = 2.0 * half                                           # centre - atom, the same exact value at every origin

            def normal(phi):
                return s * (np.cos(phi) * u + np.sin(phi) * w)

            phi0, _ = bisect(lambda p: ga64(normal(p), point) <= 30.0, *side_range(target))
            for k in OFFSETS:
                o = b.begin()
                nrm = normal(step64(phi0, k))
                r = b.ring(o + half, nrm)
                a = b.atom(o - half, tm=tm, fl=fl)
                assert np.array_equal(f64(b.rc[r]) - b.xyz[a].astype(np.float64), point)
                b.end(f'A/theta{target}/{kind}/geo{g}/ulp{k:+d}', f'theta{target}', 'atom_plane', (r, a), rings=[r], atoms=[a], k=k, decides=bits,
                      cos=cos64(nrm, point), path='f64', cut=30, kind=kind)
    return b.build('planes_A')


# ---- family B: the atom - ring distances ---------------------------------------------------------------------------------------------
def family_b(seed=202):
    """4.5 A with theta = 10 degrees (the four gated bits), 6.0 A for a MET sulphur (I:1021), and the tree radius (I:960): the x
    coordinate of the ring centre is bisected on norm(atom - centre) <= cut and stepped; about 6.0 the steps are scanned for centres on
    which the tree's plain sum of squares and the FMA-chained norm disagree."""
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    kinds = _atom_kinds()

    def geometry(dist, tilt_deg):
        u, w, _ = x_frame(rng)
        half = quant(0.5 * dist * u)
        nrm = rng.uniform(0.5, 2.0) * (np.cos(tilt_deg * DEG) * u + np.sin(tilt_deg * DEG) * w)
        sg = np.sign(u[0])

        def centre(x):           # relative to the origin; the atom sits at -half
            return np.array([x, half[1], half[2]])

        return half, nrm, sg, centre

    for seam, cut, kind, tilt in (('dist4.5', 4.5, 'all', 10.0), ('dist6.0', 6.0, 'met', 45.0)):
        tm, fl, bits = kinds[kind]
        for g in range(N_GEO):
            half, nrm, sg, centre = geometry(cut, tilt)
            x0, _ = bisect(lambda x: norm64(-half - centre(x)) <= cut, half[0] - sg * 0.05, half[0] + sg * 0.05)
            for k in OFFSETS:
                o = b.begin()
                r = b.ring(o + centre(step64(x0, k)), nrm)
                a = b.atom(o - half, tm=tm, fl=fl)
                b.end(f'B/{seam}/geo{g}/ulp{k:+d}', seam, 'atom_plane', (r, a), rings=[r], atoms=[a], k=k, decides=bits, path='f64', cut=cut)
    # the tree radius.  The two tests differ only where the squares are inexact, so the centre is not on the 2^-12 lattice here and
    # each case is searched at its own origin: +-48 ulps of x about the flip of the norm, the first step on which the tree's plain
    # sum and the FMA-chained norm disagree (8 of each order are kept, and 16 cases on which they agree)
    tm, fl, bits = kinds['met']
    have = {'tree_only': 0, 'norm_only': 0, 'agree': 0}
    for g in range(600):
        if have['tree_only'] >= 8 and have['norm_only'] >= 8:
            break
        half, nrm, sg, _ = geometry(6.0, 45.0)
        o = b.origin()
        b.slot -= 1
        atom = (o - half).astype(np.float32).astype(np.float64)
        cy, cz = o[1] + 3.0 * (half[1] / 3.0) * 1.0000001, o[2] + 3.0 * (half[2] / 3.0) * 0.9999999

        def centre(x):
            return np.array([x, cy, cz])

        x0, _ = bisect(lambda x: norm64(atom - centre(x)) <= 6.0, half[0] - sg * 0.05, half[0] + sg * 0.05)
        found = None
        for k in sorted(range(-48, 49), key=abs):
            c = centre(step64(x0, k))
            tree, near = kd2(c, atom) <= 36.0, norm64(atom - c) <= 6.0
            if tree != near:
                found = (k, 'tree_only' if tree else 'norm_only')
                break
        k, label = found or (0, 'agree')
        if have[label] >= (16 if label == 'agree' else 8):
            continue
        have[label] += 1
        b.begin()
        r = b.ring(centre(step64(x0, k)), nrm)
        a = b.atom(atom, tm=tm, fl=fl)
        b.end(f'B/tree/{label}/geo{g}/ulp{k:+d}', 'tree', 'atom_plane', (r, a), rings=[r], atoms=[a], k=k, decides=bits, path='f64', cut=6.0, label=label)
    return b.build('planes_B')


# ---- families C and D: ring - ring classes and the intra-residue EE skip ---------------------------------------------------------------
def _ring_pair(b, fr, d, sa, sb, na, nb, swap, intra, name, seam, **kw):
    """Two rings d apart along u; the ring of `na` gets the lower id unless swap.  Returns the case's pab (lower id - higher id)."""
    half = quant(0.5 * d * fr[0])
    o = b.begin()
    res = b.carrier() if intra else None
    if not swap:
        i = b.ring(o + half, sa * na, res)
        j = b.ring(o - half, sb * nb, res)
    else:
        i = b.ring(o - half, sb * nb, res)
        j = b.ring(o + half, sa * na, res)
    b.end(name, seam, 'plane_plane', (i, j), rings=[i, j], **kw)
    return i, j


def _ring_seams(b, rng, fam, seam, param, target, cut, ta, tb, dl, swap, intra, both=False, n_geo=N_GEO):
    """One seam of a ring pair: `param` ('ta', 'tb' = 'ta' on the ring with the higher id, 'dl') is bisected about `target` degrees with
    the other two angles at their nominal values.  both: then the other theta is bisected onto the same cut for every step."""
    for g in range(n_geo):
        fr = frame(rng)
        d, sa, sb = rng.uniform(4.0, 5.5), rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
        half = quant(0.5 * d * fr[0])
        pab = 2.0 * half                                   # centre of the `na` ring minus centre of the other
        dl_ = feasible_dl(target * DEG if param == 'ta' else ta * DEG, tb * DEG, target * DEG if param == 'dl' else dl * DEG)
        assert param != 'dl' or dl_ == target * DEG

        def normals(t, tb_=tb * DEG):
            if param == 'ta':
                return pair_normals(fr, t, tb_, dl_)
            return pair_normals(fr, ta * DEG, tb_, t)

        def angle(t):
            na, nb = normals(t)
            return ga64(sa * na, pab) if param == 'ta' else ga64(sa * na, sb * nb)

        t0, _ = bisect(lambda t: angle(t) <= cut, *side_range(target))
        for k in OFFSETS:
            t = step64(t0, k)
            if not both:
                na, nb = normals(t)
                c = cos64(sa * na, pab) if param == 'ta' else cos64(sa * na, sb * nb)
                _ring_pair(b, fr, d, sa, sb, na, nb, swap, intra, f'{fam}/{seam}/geo{g}/ulp{k:+d}', seam, k=k, cos=c, path='f64', cut=cut,
                           decides='theta_end' if swap and param == 'ta' else 'theta_bgn' if param == 'ta' else 'dihedral')
                continue
            tb0, _ = bisect(lambda x: ga64(sb * normals(t, x)[1], -pab) <= cut, *side_range(target))
            for kb in sorted({k, -k}):
                na, nb = normals(t, step64(tb0, kb))
                _ring_pair(b, fr, d, sa, sb, na, nb, swap, intra, f'{fam}/{seam}/geo{g}/ulp{k:+d}{kb:+d}', seam, k=k, kb=kb, cos=cos64(sa * na, pab),
                           cos_b=cos64(sb * nb, -pab), path='f64', cut=cut, decides='both thetas')


def family_c(seed=203):
    """Every cut of I:1127-1148 with the other two angles mid-class, inter-residue; exact right angles."""
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    for target in (30, 60):
        _ring_seams(b, rng, 'C', f'dih{target}', 'dl', target, float(target), 45, 45, None, False, False)
    for target in (30, 60, 120, 150):
        cut = float(min(target, 180 - target))
        _ring_seams(b, rng, 'C', f'theta_ab{target}', 'ta', target, cut, None, 45, 45, False, False)
        _ring_seams(b, rng, 'C', f'theta_ba{target}', 'ta', target, cut, None, 45, 45, True, False)
    _ring_seams(b, rng, 'C', 'theta_ab60_dih20', 'ta', 60, 60.0, None, 72, 20, False, False)      # OF | EE between two residues: EE is kept
    # cos == 0.0 exactly: products of small integers are exact, (12, 3, 4) . (0, 4, -3) = 0; and a last-place amount either side of it
    for name, eps in (('zero', 0.0), ('plus', 2.0 ** -60), ('minus', -2.0 ** -60), ('plus30', 2.0 ** -30), ('minus30', -2.0 ** -30)):
        for what in ('dih', 'theta', 'both'):
            o = b.begin()
            na = np.array([12.0, 3.0, 4.0]) * 0.125          # (the last-place amount goes into x, where the origins are 0)
            nb = np.array([eps, 4.0, -3.0]) if what != 'theta' else np.array([0.25, 0.5, 0.75])
            pab = np.array([eps, 4.0, -3.0]) if what != 'dih' else np.array([4.0, 2.0, 1.0])
            i = b.ring(o + 0.5 * pab, na)
            j = b.ring(o - 0.5 * pab, nb)
            assert np.array_equal(b.rc[i] - b.rc[j], pab)
            b.end(f'C/right/{what}/{name}', 'right', 'plane_plane', (i, j), rings=[i, j], k=0, path='f64', cut=90.0, decides=what,
                  cos=cos64(na, nb) if what != 'theta' else cos64(na, pab))
    return b.build('planes_C')


def family_d(seed=204):
    """Rings of one residue about the EE class (dihedral <= 30, 60 < theta <= 90), which I:1154 drops: theta_ab on the 60 cut with
    theta_ba inside EE (72) or inside OF (50: the reverse visit then creates the record), the mirror cases, both on the cut; and the
    same with the dihedral in (60, 90], where no class is EE and the record always exists."""
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    for dl, tag in ((20, 'ee'), (75, 'control')):
        for tb, other in ((72, 'in'), (50, 'of')):
            _ring_seams(b, rng, 'D', f'{tag}/theta_ab60/ba_{other}', 'ta', 60, 60.0, None, tb, dl, False, True)
            _ring_seams(b, rng, 'D', f'{tag}/theta_ba60/ab_{other}', 'ta', 60, 60.0, None, tb, dl, True, True)
        _ring_seams(b, rng, 'D', f'{tag}/both60', 'ta', 60, 60.0, None, 60, dl, False, True, both=True)
    return b.build('planes_D')


# ---- amide pairs and amide - ring pairs ----------------------------------------------------------------------------------------------
def _vary_component(pred, nominal, true_side, false_side):
    """(j, lo): component j of the float32 vector `nominal` bisected between its values on the two sides; lo = the last that passes."""
    nominal, a, z = f32(nominal), f32(true_side), f32(false_side)
    for j in np.argsort(-np.abs(a - z)):
        def p(x, j=j):
            v = nominal.copy()
            v[j] = x
            return pred(v)

        # (one component alone may move the angle the other way, or change sign between the two sides: any pair of its values
        # of one sign that the cut separates will do)
        for t, f in ((a[j], z[j]), (z[j], a[j]), (a[j], nominal[j]), (nominal[j], z[j]), (z[j], nominal[j]), (nominal[j], a[j])):
            if t != f and np.sign(t) == np.sign(f) != 0 and p(t) and not p(f):
                return int(j), bisect_bits32(p, t, f)[0]
    raise AssertionError('no component crosses the cut')


def _with(v, j, x):
    v = f32(v).copy()
    v[j] = x
    return v


def _amide_seams(b, rng, fam, loop, seam, param, target, both=False):
    """An amide against an amide (float32 end to end) or a ring (float32 normal and norm(normal), float64 dot and vector): the bit
    pattern of one component of the amide's normal is bisected so that theta ('ta') or the dihedral ('dl') crosses 30; both: theta by
    the amide's normal, then the dihedral by a component of the second amide's normal / the rotation of the ring's normal."""
    gg = loop == 'group_group'
    ang = ga32 if gg else gamix
    cosf = cos32 if gg else cosmix
    for g in range(N_GEO):
        fr = frame(rng)
        d, sa, sb = rng.uniform(4.0, 5.5), rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
        half = quant(0.5 * d * fr[0])
        pab = f32(2.0 * half) if gg else 2.0 * half          # exact in float32 too
        ta = target * DEG if param == 'ta' or both else 10 * DEG
        dl = target * DEG if param == 'dl' or both else 10 * DEG
        if both:
            dl = 30 * DEG                                     # (theta about 150 and a dihedral about 150 at once leave no room for tb)
        tb = far_tb(ta, dl)

        def normals(ta_, dl_):           # the second normal is fixed at tb from the centre line; the amide's follows ta and dl
            nb, na = pair_normals(fr, tb, ta_, dl_)
            return f32(sa * na), (f32(sb * nb) if gg else sb * nb)

        def second(x, na):                # the second normal turned towards (x > 1) or away from (x < 1) the direction of na
            v = np.asarray(na, np.float64)
            return nb0 + (x - 1.0) * (v * (np.linalg.norm(nb0) / np.linalg.norm(v)) - nb0)

        na0, nb0 = normals(ta, dl)
        w = 3.0
        if param == 'ta' or both:
            t_true, t_false = side_range(target, w)
            j, lo = _vary_component(lambda v: ang(v, pab) <= 30.0, na0, normals(t_true, dl)[0], normals(t_false, dl)[0])
        else:
            d_true, d_false = side_range(target, w)
            j, lo = _vary_component(lambda v: ang(v, nb0) <= 30.0, na0, normals(ta, d_true)[0], normals(ta, d_false)[0])
        for k in OFFSETS:
            na = _with(na0, j, step32(lo, k))
            variants = [(nb0, None)]
            if both:
                if gg:
                    j2, lo2 = _vary_component(lambda v: ang(na, v) <= 30.0, nb0, second(1.25, na), second(0.75, na))
                    variants = [(_with(nb0, j2, step32(lo2, kb)), kb) for kb in sorted({k, -k})]
                else:
                    x0, _ = bisect(lambda x: ang(na, second(x, na)) <= 30.0, 1.25, 0.75)
                    variants = [(second(step64(x0, kb), na), kb) for kb in sorted({k, -k})]
            for nb, kb in variants:
                o = b.begin()
                i = b.amide(o + half, na)
                jj = b.amide(o - half, nb) if gg else b.ring(o - half, nb)
                kw = dict(amides=[i, jj]) if gg else dict(amides=[i], rings=[jj])
                c_t, c_d = cosf(na, pab), cosf(na, nb)
                b.end(f'{fam}/{seam}/geo{g}/ulp{k:+d}' + ('' if kb is None else f'{kb:+d}'), seam, loop, (i, jj), k=k, kb=kb, path='f32' if gg else 'mix',
                      cut=30.0, cos=float(c_t if param == 'ta' or both else c_d), cos_b=float(c_d) if both else None,
                      decides='both' if both else 'theta' if param == 'ta' else 'dihedral', **kw)


def _amide_ring_f64_seams(b, rng, target):
    """The amide - ring pair moved by its float64 side, where neighbouring cases are single float64 steps of the cosine apart: the
    dihedral by turning the ring's normal, theta by the x coordinate of the ring's centre."""
    for param in ('dl', 'ta'):
        g = 0
        while g < N_GEO:
            fr = x_frame(rng)
            d, sa, sb = rng.uniform(4.0, 5.5), rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
            half = quant(0.5 * d * fr[0])
            ta = target * DEG if param == 'ta' else 10 * DEG
            dl = target * DEG if param == 'dl' else 10 * DEG
            nb, na = pair_normals(fr, far_tb(ta, dl), ta, dl)
            na, nb = f32(sa * na), sb * nb

            def ring(t):                  # (normal, centre relative to the origin) of the ring for the parameter t about 1
                if param == 'dl':
                    v = na.astype(np.float64)
                    return nb + (t - 1.0) * (v * (np.linalg.norm(nb) / np.linalg.norm(v)) - nb), -half
                return nb, np.array([-half[0] * t, -half[1], -half[2]])

            def passes(t):
                n_, c_ = ring(t)
                return (gamix(na, n_) if param == 'dl' else gamix(na, half - c_)) <= 30.0

            ends = [(x, y) for x, y in ((1.3, 0.7), (0.7, 1.3)) if passes(x) and not passes(y)]
            if not ends:                  # (the centre's x alone does not carry theta across the cut in this frame: another one)
                continue
            t0, _ = bisect(passes, *ends[0])
            for k in OFFSETS:
                n_, c_ = ring(step64(t0, k))
                o = b.begin()
                i, j = b.amide(o + half, na), b.ring(o + c_, n_)
                seam = f'{"dih" if param == "dl" else "theta"}{target}_ring'
                b.end(f'G/{seam}/geo{g}/ulp{k:+d}', seam, 'group_plane', (i, j), amides=[i], rings=[j], k=k, path='mix', cut=30.0,
                      cos=cosmix(na, n_) if param == 'dl' else cosmix(na, half - c_), decides='dihedral' if param == 'dl' else 'theta')
            g += 1


def family_f(seed=206):
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    for target in (30, 150):
        _amide_seams(b, rng, 'F', 'group_group', f'dih{target}', 'dl', target)
        _amide_seams(b, rng, 'F', 'group_group', f'theta{target}', 'ta', target)
        _amide_seams(b, rng, 'F', 'group_group', f'both{target}', 'ta', target, both=True)
    return b.build('planes_F')


def family_g(seed=207):
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    for target in (30, 150):
        _amide_seams(b, rng, 'G', 'group_plane', f'dih{target}', 'dl', target)
        _amide_seams(b, rng, 'G', 'group_plane', f'theta{target}', 'ta', target)
        _amide_seams(b, rng, 'G', 'group_plane', f'both{target}', 'ta', target, both=True)
        _amide_ring_f64_seams(b, rng, target)
    return b.build('planes_G')


# ---- family E: the 6.0 A centre distance of the three pair loops and their list supersets ---------------------------------------------------
def family_e(seed=205):
    """!(dist > 6.0) in float64 (ring - ring I:1113, amide - ring I:1351) and in float32 (amide - amide I:1270): the x coordinate of the
    second centre is bisected (float32: its bit pattern; y and z are exact and the origin has x = 0, so the steps are single ulps of a
    value of a few A).  Then centres between 6.0 and the candidate lists' supersets, 36 (1 + 1e-9) and 36 (1 + 1e-5) in the squared
    distance, and just beyond them: on the list or not, no record."""
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    for loop in ('plane_plane', 'group_plane', 'group_group'):
        gg, eps = loop == 'group_group', 1e-5 if loop == 'group_group' else 1e-9
        for g in range(N_GEO):
            fr = x_frame(rng)
            sg = np.sign(fr[0][0])
            half = quant(3.0 * fr[0])
            if loop == 'plane_plane':
                na, nb = pair_normals(fr, 45 * DEG, 45 * DEG, 45 * DEG)
            else:
                na, nb = pair_normals(fr, 10 * DEG, far_tb(10 * DEG, 10 * DEG), 10 * DEG)
            na, nb = rng.uniform(0.5, 2.0) * na, rng.uniform(0.5, 2.0) * nb
            first = half if loop == 'plane_plane' else f32(half)          # relative to the origin; float32 for an amide

            def second(x):
                c = np.array([x, -half[1], -half[2]])
                return f32(c) if gg else c

            def dist_ok(x):
                if gg:
                    return not norm32(first - second(x)) > np.float32(6.0)
                return not norm64(first.astype(np.float64) - second(x)) > 6.0

            def add(x, name, seam, **kw):
                o = b.begin()
                if loop == 'plane_plane':
                    i, j = b.ring(o + first, na), b.ring(o + second(x), nb)
                    items = dict(rings=[i, j])
                elif gg:
                    i, j = b.amide(o + first, na), b.amide(o + second(x), nb)
                    items = dict(amides=[i, j])
                else:
                    i, j = b.amide(o + first, na), b.ring(o + second(x), nb)
                    items = dict(amides=[i], rings=[j])
                assert b.ac[i][0] == first[0] if loop != 'plane_plane' else b.rc[i][0] == first[0]
                d2 = kd2(np.asarray(first, np.float64), np.asarray(second(x), np.float64))
                b.end(name, seam, loop, (i, j), path='f32' if gg else 'f64', cut=6.0, decides='record', d2=d2, eps=eps, **items, **kw)

            if gg:
                x0, _ = bisect_bits32(dist_ok, np.float32(-half[0] + sg * 0.05), np.float32(-half[0] - sg * 0.05))
            else:
                x0, _ = bisect(dist_ok, -half[0] + sg * 0.05, -half[0] - sg * 0.05)
            for k in OFFSETS:
                add(step32(x0, k) if gg else step64(x0, k), f'E/{loop}/dist6/geo{g}/ulp{k:+d}', f'{loop}/dist6', k=k)
            if g < 6:
                dy2 = float(first[1]) + half[1], float(first[2]) + half[2]
                for frac in (0.05, 0.5, 0.95, 0.999, 1.001, 1.05, 2.0):
                    x = float(first[0]) - sg * np.sqrt(36.0 * (1.0 + frac * eps) - dy2[0] ** 2 - dy2[1] ** 2)
                    x = float(np.float32(x)) if gg else x
                    d2 = kd2(np.asarray(first, np.float64), np.asarray(second(x), np.float64))
                    label = 'on_list' if 36.0 < d2 <= 36.0 * (1.0 + eps) else 'beyond' if d2 > 36.0 * (1.0 + eps) else 'inside'
                    add(x, f'E/{loop}/superset/{label}/geo{g}/frac{frac}', f'{loop}/superset', k=0, label=label)
    return b.build('planes_E')


# ---- family H: degenerate cosines ------------------------------------------------------------------------------------------------------
def family_h(seed=208, want=4, trials=4000):
    """Parallel and antiparallel normals and normals along the centre line, searched for components whose dot / (norm * norm) rounds to
    just inside 1, to exactly 1 and beyond 1 (NaN: class '' in the ring - ring loop, a record in the !(a > 30 || b > 30) loops, no gated
    bit in the atom - ring loop); cosines a last place either side of the fold at pi / 2; coincident centres and zero normals."""
    rng = np.random.default_rng(seed)
    b = PlaneBuilder()
    kinds = _atom_kinds()
    tm_all, fl_all, _ = kinds['all+met']

    def outcome(c):
        c = abs(float(c))
        return 'nan' if np.isnan(c) else 'beyond' if c > 1.0 else 'one' if c == 1.0 else 'inside'

    def emit(loop, q, sign, have, what, na, nb, half, c):
        have[what] += 1
        o = b.begin()
        name = f'H/{loop}/{q}/{"par" if sign > 0 else "anti"}/{what}{have[what]}'
        kw = dict(k=0, path={'plane_plane': 'f64', 'atom_plane': 'f64', 'group_group': 'f32', 'group_plane': 'mix'}[loop], cut=30.0, cos=float(c),
                  decides=q, label=what)
        if loop == 'plane_plane':
            if q == 'theta' and have[what] % 2 == 0:      # the degenerate theta on the ring of the reverse visit: type2 takes the ''
                j, i = b.ring(o - half, nb), b.ring(o + half, na)
            else:
                i, j = b.ring(o + half, na), b.ring(o - half, nb)
            b.end(name, f'{loop}/{q}', loop, (min(i, j), max(i, j)), rings=[i, j], **kw)
        elif loop == 'atom_plane':
            i = b.ring(o + half, na)
            a = b.atom(o - half, tm=tm_all, fl=fl_all)
            b.end(name, f'{loop}/{q}', loop, (i, a), rings=[i], atoms=[a], **kw)
        elif loop == 'group_group':
            i, j = b.amide(o + half, na), b.amide(o - half, nb)
            b.end(name, f'{loop}/{q}', loop, (i, j), amides=[i, j], **kw)
        else:
            i, j = b.amide(o + half, na), b.ring(o - half, nb)
            b.end(name, f'{loop}/{q}', loop, (i, j), amides=[i], rings=[j], **kw)

    specs = [(loop, q, sign) for loop in ('plane_plane', 'group_group', 'group_plane', 'atom_plane') for q in ('dih', 'theta') for sign in (1, -1)
             if not (loop == 'atom_plane' and q == 'dih')]
    for loop, q, sign in specs:
        have = {'inside': 0, 'one': 0, 'beyond': 0}
        if loop == 'group_plane':
            # amide - ring: norm(normal) is rounded to float32 before it meets the float64 dot, so a quotient of exactly 1 needs a normal
            # whose length is a float32, which no random normal has.  Constructed: (3, 4, 12) has the length 13, its multiples by powers
            # of two are exact in both formats, and so are the dot and both norms; the other angle is 20 degrees as above.
            for m in range(want):
                v = np.roll(np.array([3.0, 4.0, 12.0]), m % 3)
                if m >= 3:
                    v[0] = -v[0]
                p_ = np.cross(v, rng.standard_normal(3))
                tilt = np.cos(20 * DEG) * v / 13.0 + np.sin(20 * DEG) * p_ / np.linalg.norm(p_)
                if q == 'dih':
                    na = f32(v * 0.125 * 2.0 ** (m - 1))
                    nb = sign * 2.0 ** (1 - m) * na.astype(np.float64)
                    half = quant(2.0 * tilt)
                    c = cosmix(na, nb)
                else:
                    half = v * 0.15625
                    na, nb = f32(sign * v * 0.125 * 2.0 ** (m - 1)), rng.uniform(0.5, 2.0) * tilt
                    c = cosmix(na, 2.0 * half)
                assert c == float(sign) and np.array_equal(quant(half), half), (q, sign, m, c)
                emit(loop, q, sign, have, 'one', na, nb, half, c)
        for _ in range(trials):
            if min(have.values()) >= want:
                break
            fr = frame(rng)
            u = fr[0]
            half = quant(rng.uniform(1.6, 2.4) * u)
            pab64 = 2.0 * half
            s, t = rng.uniform(0.5, 2.0), sign * rng.uniform(0.5, 2.0)
            tilt = np.cos(20 * DEG) * u + np.sin(20 * DEG) * fr[1]          # the other quantity: 20 degrees, inside every cut
            if loop in ('plane_plane', 'atom_plane'):
                if q == 'dih':
                    na = s * tilt
                    nb = t * na
                    c = cos64(na, nb)
                else:
                    na, nb = t * pab64, s * tilt
                    c = cos64(na, pab64)
            elif loop == 'group_group':
                if q == 'dih':
                    na = f32(s * tilt)
                    nb = f32(np.float32(t) * na)
                    c = cos32(na, nb)
                else:
                    na, nb = f32(np.float32(t) * f32(pab64)), f32(s * tilt)
                    c = cos32(na, f32(pab64))
            else:
                if q == 'dih':
                    na = f32(s * tilt)
                    nb = t * na.astype(np.float64)
                    c = cosmix(na, nb)
                else:
                    na, nb = f32(np.float32(t) * f32(pab64)), s * tilt
                    c = cosmix(na, pab64)
            what = outcome(c)
            if what == 'nan' or have[what] >= want:
                continue
            emit(loop, q, sign, have, what, na, nb, half, c)
    # the fold at pi / 2: exact small-integer components, cos = 0 and a last place either side, in the three pair loops
    for loop in ('plane_plane', 'group_group', 'group_plane'):
        for name, eps in (('zero', 0.0), ('plus', 2.0 ** -40), ('minus', -2.0 ** -40)):
            o = b.begin()
            na, nb, pab = np.array([3.0, 4.0, 12.0]) * 0.125, np.array([4.0, -3.0, eps]), np.array([4.0, -3.0, 0.0])
            if loop == 'plane_plane':
                i, j = b.ring(o + 0.5 * pab, na), b.ring(o - 0.5 * pab, nb)
                kw, c = dict(rings=[i, j]), cos64(na, nb)
            elif loop == 'group_group':
                i, j = b.amide(o + 0.5 * pab, na), b.amide(o - 0.5 * pab, nb)
                kw, c = dict(amides=[i, j]), cos32(na, nb)
            else:
                i, j = b.amide(o + 0.5 * pab, na), b.ring(o - 0.5 * pab, nb)
                kw, c = dict(amides=[i], rings=[j]), cosmix(na, nb)
            b.end(f'H/{loop}/fold/{name}', f'{loop}/fold', loop, (i, j), k=0, path='f64', cut=90.0, cos=float(c), decides='fold', label=name, **kw)
    # coincident centres (theta NaN) and zero normals (both angles NaN)
    for loop in ('plane_plane', 'group_group', 'group_plane', 'atom_plane'):
        for name in ('coincident', 'zero_normal'):
            o = b.begin()
            fr = frame(rng)
            off = np.zeros(3) if name == 'coincident' else quant(2.0 * fr[0])
            na = fr[1] if name == 'coincident' else np.zeros(3)
            nb = np.cos(0.2) * fr[1] + np.sin(0.2) * fr[2]
            if loop == 'plane_plane':
                i, j = b.ring(o + off, na), b.ring(o - off, nb)
                kw = dict(rings=[i, j])
            elif loop == 'group_group':
                i, j = b.amide(o + off, na), b.amide(o - off, nb)
                kw = dict(amides=[i, j])
            elif loop == 'group_plane':
                i, j = b.amide(o + off, na), b.ring(o - off, nb)
                kw = dict(amides=[i], rings=[j])
            else:
                i, j = b.ring(o + off, na), b.atom(o - off, tm=tm_all, fl=fl_all)
                kw = dict(rings=[i], atoms=[j])
            b.end(f'H/{loop}/{name}', f'{loop}/{name}', loop, (i, j), k=0, path='f64', cut=30.0, decides='nan', label=name, **kw)
    return b.build('planes_H')


FAMILIES = {'A': family_a, 'B': family_b, 'C': family_c, 'D': family_d, 'E': family_e, 'F': family_f, 'G': family_g, 'H': family_h}


@functools.lru_cache(maxsize=None)
def packs(family):
    return FAMILIES[family]()


def unrelated_structure():
    """A small structure with rings, amides and typed atoms of its own: the batch partner of a family."""
    from arpeggio_amd import synth
    return synth.proteinlike(n_res=40, n_waters=10, seed=31)


@functools.lru_cache(maxsize=None)
def oracle_bags(family, partial=False):
    """The oracle's four ring / amide bags of a family's pack, each in its canonical order; whole structure or the pack's partial selection."""
    import oracle
    pc = packs(family).pc
    oc = oracle.OracleComplex(pc)
    oc.make_selection(pc.partial_selection if partial else None)
    out = {}
    for loop, order in LOOPS.items():
        e = getattr(oc, loop)()
        o = np.lexsort((e[order[1]], e[order[0]]))
        out[loop] = {k: v[o] for k, v in e.items()}
    return out
