"""ref_py — second, independent restatement of the per-pair loop in the reference's own idiom: Python control flow
and *real NumPy calls* (np.linalg.norm, np.dot, np.arccos on float32 / float64 arrays), so that it inherits whatever
NumPy + BLAS actually do on the machine it runs on.  TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Purpose: (1) cross-check oracle/ref_c.c, whose arithmetic is an explicit model of these NumPy calls (float32 dot with
float64 accumulation, FMA-chained float64 dot, NEP-50 comparisons); (2) the interpreter-bound "B1" baseline of
BASELINE.md.  Only small inputs: it is as slow as the reference.

Follows arpeggio/core/interactions.py:693-936 and arpeggio/core/utils.py:73-179, 696-745 on a PackedComplex; the four
ring / amide loops (interactions.py:947-1382 with utils.py:638-693) are the methods atom_plane, plane_plane, group_group
and group_plane of RefPy.
"""
from __future__ import annotations

import numpy as np

from arpeggio_amd.core import config

T = config.ATOM_TYPE_BIT
S = {name: 1 << k for k, name in enumerate(config.SIFT_NAMES)}
CT = {name: k for k, name in enumerate(config.CONTACT_TYPE_NAMES)}
TH = config.CONTACT_TYPES


def get_angle(pa, pb, pc):
    """utils.py:696-745 with NumPy scalars: the dtype follows the operands exactly as in the reference."""
    v1 = pa - pb
    v2 = pc - pb
    with np.errstate(all='ignore'):
        m1 = np.sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2])
        n1 = np.array([v1[0] / m1, v1[1] / m1, v1[2] / m1])
        m2 = np.sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2])
        n2 = np.array([v2[0] / m2, v2[1] / m2, v2[2] / m2])
        ang = np.arccos(n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2])
    return np.pi if np.isnan(ang) else ang


def group_angle(normal, point):
    """utils.py:638-660 and 663-693 (the two are one expression) with degrees=True, signed=True: the dtype follows the operands
    (float32 scalars against the Python floats np.pi, 180: NEP 50 keeps float32)."""
    with np.errstate(all='ignore'):
        cosangle = np.dot(normal, point) / (np.linalg.norm(normal) * np.linalg.norm(point))
        rad = np.arccos(cosangle)
    rad = rad - np.pi if rad > np.pi / 2 else rad
    return rad * 180 / np.pi


def plane_contact_type(a_sel, b_sel, a_plus, b_plus):
    """The chain of four ifs of interactions.py:985-997, 1095-1108, 1252-1265, 1333-1346."""
    ct = None
    if not a_sel and not b_sel:
        ct = 'INTRA_NON_SELECTION'
    if a_plus and b_plus:
        ct = 'INTRA_BINDING_SITE'
    if a_sel and b_sel:
        ct = 'INTRA_SELECTION'
    if (a_sel and not b_sel) or (b_sel and not a_sel):
        ct = 'INTER'
    return CT[ct]


def plane_plane_class(dihedral, theta):
    """interactions.py:1127-1148; '' when no branch applies (an angle is NaN)."""
    int_type = ''
    if dihedral <= 30.0 and theta <= 30.0:
        int_type = 'FF'
    elif dihedral <= 30.0 and theta <= 60.0:
        int_type = 'OF'
    elif dihedral <= 30.0 and theta <= 90.0:
        int_type = 'EE'
    elif 30.0 < dihedral <= 60.0 and theta <= 30.0:
        int_type = 'FT'
    elif 30.0 < dihedral <= 60.0 and theta <= 60.0:
        int_type = 'OT'
    elif 30.0 < dihedral <= 60.0 and theta <= 90.0:
        int_type = 'ET'
    elif 60.0 < dihedral <= 90.0 and theta <= 30.0:
        int_type = 'FE'
    elif 60.0 < dihedral <= 90.0 and theta <= 60.0:
        int_type = 'OE'
    elif 60.0 < dihedral <= 90.0 and theta <= 90.0:
        int_type = 'EF'
    return int_type


class RefPy:
    def __init__(self, pc, in_sel=None, in_plus=None):
        self.pc = pc
        n = pc.n_atoms
        self.sel = np.ones(n, bool) if in_sel is None else np.asarray(in_sel, bool)
        self.plus = np.ones(n, bool) if in_plus is None else np.asarray(in_plus, bool)
        # interactions.py:1413-1437: a ring / amide belongs to the selection (selection_plus) when its residue does
        res_sel, res_plus = set(pc.res_id[self.sel].tolist()), set(pc.res_id[self.plus].tolist())
        self.ring_sel = [int(r) in res_sel for r in pc.ring_res]
        self.ring_plus = [int(r) in res_plus for r in pc.ring_res]
        self.amide_sel = [int(r) in res_sel for r in pc.amide_res]
        self.amide_plus = [int(r) in res_plus for r in pc.amide_res]
        self.h = [pc.h_xyz[pc.h_off[i]:pc.h_off[i + 1]] for i in range(n)]                  # float64 rows
        self.bonded = [set(pc.bond_idx[pc.bond_off[i]:pc.bond_off[i + 1]].tolist()) for i in range(n)]

    # utils.py:73-116
    def _hbond(self, donor, acceptor, comp, angle_min):
        pc = self.pc
        for h in self.h[donor]:
            if np.linalg.norm(h - pc.xyz[acceptor]) <= config.VDW_RADII['H'] + float(pc.vdw[acceptor]) + comp:
                if get_angle(pc.xyz[donor], h, pc.xyz[acceptor]) >= angle_min:
                    return True
        return False

    # utils.py:119-155
    def _halogen_weak(self, donor, halogen, comp):
        pc = self.pc
        nbr = int(pc.sb_nbr[halogen])
        if nbr < 0:
            return False
        for h in self.h[donor]:
            if np.linalg.norm(pc.xyz[halogen] - h) <= config.VDW_RADII['H'] + float(pc.vdw[halogen]) + comp:
                a = get_angle(pc.xyz[nbr], pc.xyz[halogen], h)
                if TH['weak hbond']['cx angle min rad'] <= a <= TH['weak hbond']['cx angle max rad']:
                    return True
        return False

    # utils.py:158-179
    def _xbond(self, donor, acceptor):
        pc = self.pc
        nbr = int(pc.sb_nbr[donor])
        if nbr < 0:
            raise AttributeError("'NoneType' object has no attribute 'GetId'")
        return get_angle(pc.xyz[nbr], pc.xyz[donor], pc.xyz[acceptor]) >= TH['xbond']['angle theta 1 rad']

    # interactions.py:643-691
    def _ctype(self, b, e):
        pc = self.pc
        bs, es = self.sel[b], self.sel[e]
        bw, ew = bool(pc.flags[b] & config.F_WATER), bool(pc.flags[e] & config.F_WATER)
        ct = None
        if not bs and not es:
            ct = 'INTRA_NON_SELECTION'
        if bs and es:
            ct = 'INTRA_SELECTION'
        if (bs and not es) or (es and not bs):
            ct = 'INTER'
        if (bs and ew) or (es and bw):
            ct = 'SELECTION_WATER'
        if (not bs and ew) or (not es and bw):
            ct = 'NON_SELECTION_WATER'
        if bw and ew:
            ct = 'WATER_WATER'
        return ct

    def pair(self, b, e, comp=0.1, include_sequence_adjacent=False):
        """One iteration of interactions.py:707-936 for the ordered pair (bgn=b, end=e); None when it `continue`s."""
        pc = self.pc
        fb, fe = int(pc.flags[b]), int(pc.flags[e])
        tb, te = int(pc.type_mask[b]), int(pc.type_mask[e])
        if (fb | fe) & config.F_HYDROGEN:
            return None
        ct = self._ctype(b, e)
        sum_cov = float(pc.cov[b]) + float(pc.cov[e])
        sum_vdw = float(pc.vdw[b]) + float(pc.vdw[e])
        rb, re = int(pc.res_id[b]), int(pc.res_id[e])
        if rb == re:
            return None
        if not include_sequence_adjacent and pc.res_flags[re] & config.R_POLYPEPTIDE:
            if pc.res_flags[rb] & config.R_HAS_SEQ and pc.res_flags[re] & config.R_HAS_SEQ:
                if pc.res_next[rb] == re or pc.res_prev[rb] == re or pc.res_next[re] == rb or pc.res_prev[re] == rb:
                    return None
        d = np.linalg.norm(pc.xyz[b] - pc.xyz[e])                 # float32 scalar
        s = 0
        if e in self.bonded[b]:
            s |= S['covalent']
        elif d < sum_cov:                                          # float32 vs Python float: NEP 50 -> float32 compare
            s |= S['clash']
        elif d < sum_vdw:
            s |= S['vdw_clash']
        elif d <= sum_vdw + comp:
            s |= S['vdw']
        else:
            s |= S['proximal']
        if d <= TH['metal']['distance']:
            if tb & T['hbond acceptor'] and fe & config.F_METAL:
                s |= S['metal_complex']
            elif te & T['hbond acceptor'] and fb & config.F_METAL:
                s |= S['metal_complex']
        if not s & S['clash'] and d <= config.CONTACT_TYPES_DIST_MAX:
            bw, ew = fb & config.F_WATER, fe & config.F_WATER
            if bw and d <= sum_vdw + comp:
                if te & (T['hbond acceptor'] | T['hbond donor']):
                    s |= S['hbond'] | S['polar']
            elif ew and d <= sum_vdw + comp:
                if tb & (T['hbond acceptor'] | T['hbond donor']):
                    s |= S['hbond'] | S['polar']
            else:
                if tb & T['hbond donor'] and te & T['hbond acceptor']:
                    if self._hbond(b, e, comp, TH['hbond']['angle rad']):
                        s |= S['hbond']
                    if d <= TH['hbond']['polar distance']:
                        s |= S['polar']
                elif te & T['hbond donor'] and tb & T['hbond acceptor']:
                    if self._hbond(e, b, comp, TH['hbond']['angle rad']):
                        s |= S['hbond']
                    if d <= TH['hbond']['polar distance']:
                        s |= S['polar']
            weak = False
            wp = d <= TH['weak hbond']['weak polar distance']
            if tb & T['hbond acceptor'] and te & T['weak hbond donor']:
                weak = self._hbond(e, b, comp, TH['weak hbond']['angle rad'])
                s |= S['weak_polar'] if wp else 0
            if tb & T['weak hbond donor'] and te & T['hbond acceptor']:
                weak = self._hbond(b, e, comp, TH['weak hbond']['angle rad'])
                s |= S['weak_polar'] if wp else 0
            if tb & T['weak hbond acceptor'] and fb & config.F_HALOGEN and te & (T['hbond donor'] | T['weak hbond donor']):
                weak = self._halogen_weak(e, b, comp)
                s |= S['weak_polar'] if wp else 0
            if te & T['weak hbond acceptor'] and fe & config.F_HALOGEN and tb & (T['hbond donor'] | T['weak hbond donor']):
                weak = self._halogen_weak(b, e, comp)
                s |= S['weak_polar'] if wp else 0
            if weak:
                s |= S['weak_hbond']
            if d <= sum_vdw + comp:
                if tb & T['xbond donor'] and te & T['xbond acceptor']:
                    s |= S['xbond'] if self._xbond(b, e) else 0
                elif te & T['xbond donor'] and tb & T['xbond acceptor']:
                    s |= S['xbond'] if self._xbond(e, b) else 0
            if d <= TH['ionic']['distance']:
                if (tb & T['pos ionisable'] and te & T['neg ionisable']) or (tb & T['neg ionisable'] and te & T['pos ionisable']):
                    s |= S['ionic']
            if d <= TH['carbonyl']['distance']:
                if (tb & T['carbonyl oxygen'] and te & T['carbonyl carbon']) or (te & T['carbonyl oxygen'] and tb & T['carbonyl carbon']):
                    s |= S['carbonyl']
            if tb & te & T['aromatic'] and d <= TH['aromatic']['distance']:
                s |= S['aromatic']
            if tb & te & T['hydrophobe'] and d <= TH['hydrophobic']['distance']:
                s |= S['hydrophobic']
        return d, s, CT[ct]

    def atom_contacts(self, cutoff=5.0, comp=0.1, include_sequence_adjacent=False):
        """Brute-force search_all over selection_plus (float64 d^2 <= r^2), canonical orientation, sorted by (i, j)."""
        pc = self.pc
        idx = np.nonzero(self.plus)[0]
        x = pc.xyz[idx].astype(np.float64)
        out = []
        for a in range(len(idx)):
            dv = x[a + 1:] - x[a]
            d2 = dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]
            d2 = d2 + dv[:, 2] * dv[:, 2]
            for k in np.nonzero(d2 <= cutoff * cutoff)[0]:
                b, e = int(idx[a]), int(idx[a + 1 + k])
                r = self.pair(b, e, comp, include_sequence_adjacent)
                if r is not None:
                    out.append((b, e) + r)
        out.sort(key=lambda t: (t[0], t[1]))
        return dict(i=np.array([t[0] for t in out], np.int32), j=np.array([t[1] for t in out], np.int32),
                    dist=np.array([t[2] for t in out], np.float32), sift=np.array([t[3] for t in out], np.uint16),
                    ctype=np.array([t[4] for t in out], np.uint8))

    # ---- the ring / amide loops ------------------------------------------------------------------------------------
    @staticmethod
    def _near(centres, c, reach=7.0):
        """Items whose centre is within `reach` of c, ascending: a vectorised superset of the loops' own 6.0 A tests (which
        still run, in the reference's arithmetic, on every item it lets through) so that the double loops stay affordable."""
        d = np.asarray(centres, np.float64) - np.asarray(c, np.float64)
        return np.nonzero((d * d).sum(axis=1) <= reach * reach)[0].tolist()

    # interactions.py:947-1062
    def atom_plane(self):
        pc = self.pc
        AP = {name: 1 << k for k, name in enumerate(config.ATOM_PLANE_NAMES)}
        x64 = pc.xyz.astype(np.float64)
        out = []
        for r in range(pc.n_rings):
            if not self.ring_plus[r]:
                continue
            center, normal = pc.ring_center[r], pc.ring_normal[r]
            # NeighborSearch.search(center, 6.0) on the tree of selection_plus: float64 sum of squares, inclusive
            d = center - x64
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            d2 = d2 + d[:, 2] * d[:, 2]
            for a in np.nonzero((d2 <= 6.0 * 6.0) & self.plus)[0].tolist():
                fl, tm = int(pc.flags[a]), int(pc.type_mask[a])
                if fl & config.F_HYDROGEN:
                    continue
                distance = np.linalg.norm(pc.xyz[a] - center)
                if tm & T['aromatic']:
                    continue
                ct = plane_contact_type(self.ring_sel[r], self.sel[a], self.ring_plus[r], self.plus[a])
                theta = abs(group_angle(normal, center - pc.xyz[a]))
                m = 0
                if distance <= TH['aromatic']['atom_aromatic_distance'] and theta <= 30.0:
                    if fl & config.F_ELEM_C and tm & T['weak hbond donor']:
                        m |= AP['CARBONPI']
                    if tm & T['pos ionisable']:
                        m |= AP['CATIONPI']
                    if tm & T['hbond donor']:
                        m |= AP['DONORPI']
                    if tm & T['xbond donor']:
                        m |= AP['HALOGENPI']
                if distance <= TH['aromatic']['met_sulphur_aromatic_distance']:
                    if fl & config.F_RES_MET and fl & config.F_ELEM_S:
                        m |= AP['METSULPHURPI']
                if not m:
                    continue
                out.append((r, a, distance, theta, m, ct))
        out.sort(key=lambda t: (t[0], t[1]))
        return dict(atom=np.array([t[1] for t in out], np.int32), ring=np.array([t[0] for t in out], np.int32),
                    dist=np.array([t[2] for t in out], np.float64), theta=np.array([t[3] for t in out], np.float64),
                    mask=np.array([t[4] for t in out], np.uint8), ctype=np.array([t[5] for t in out], np.uint8))

    # interactions.py:1064-1194: the ordered double loop and its dedupe, records in creation order
    def plane_plane(self):
        pc = self.pc
        names = {n: k for k, n in enumerate(config.PLANE_PLANE_NAMES)}
        contacts, index = [], {}
        for r1 in range(pc.n_rings):
            for r2 in self._near(pc.ring_center, pc.ring_center[r1]):
                if not self.ring_plus[r1] or not self.ring_plus[r2]:
                    continue
                if r1 == r2:
                    continue
                intra_residue = pc.ring_res[r1] == pc.ring_res[r2]
                ct = plane_contact_type(self.ring_sel[r1], self.ring_sel[r2], self.ring_plus[r1], self.ring_plus[r2])
                distance = np.linalg.norm(pc.ring_center[r1] - pc.ring_center[r2])
                if distance > TH['aromatic']['centroid_distance']:
                    continue
                theta_point = pc.ring_center[r1] - pc.ring_center[r2]
                dihedral = abs(group_angle(pc.ring_normal[r1], pc.ring_normal[r2]))
                theta = abs(group_angle(pc.ring_normal[r1], theta_point))
                int_type = plane_plane_class(dihedral, theta)
                if intra_residue and int_type == 'EE':
                    continue
                identity = index.get((r1, r2), index.get((r2, r1)))
                if identity is not None:
                    if int_type not in identity['types']:
                        identity['types'].append(int_type)
                    identity['seen'], identity['theta_end'] = True, theta
                else:
                    index[(r1, r2)] = dict(bgn=r1, end=r2, dist=distance, dihedral=dihedral, theta_bgn=theta, theta_end=np.nan,
                                           types=[int_type], seen=False, ctype=ct)
                    contacts.append(index[(r1, r2)])
        type2 = [names[c['types'][1]] if len(c['types']) > 1 else (config.PP_SAME if c['seen'] else config.PP_SKIPPED) for c in contacts]
        return dict(bgn=np.array([c['bgn'] for c in contacts], np.int32), end=np.array([c['end'] for c in contacts], np.int32),
                    dist=np.array([c['dist'] for c in contacts], np.float64), dihedral=np.array([c['dihedral'] for c in contacts], np.float64),
                    theta_bgn=np.array([c['theta_bgn'] for c in contacts], np.float64),
                    theta_end=np.array([c['theta_end'] for c in contacts], np.float64),
                    type1=np.array([names[c['types'][0]] for c in contacts], np.uint8), type2=np.array(type2, np.uint8),
                    ctype=np.array([c['ctype'] for c in contacts], np.uint8))

    # interactions.py:1217-1300, float32 throughout
    def group_group(self):
        pc = self.pc
        out = []
        for a1 in range(pc.n_amides):
            if not self.amide_plus[a1]:
                continue
            for a2 in self._near(pc.amide_center, pc.amide_center[a1]):
                if a1 == a2:
                    continue
                if not self.amide_plus[a2]:
                    continue
                ct = plane_contact_type(self.amide_sel[a1], self.amide_sel[a2], self.amide_plus[a1], self.amide_plus[a2])
                distance = np.linalg.norm(pc.amide_center[a1] - pc.amide_center[a2])
                if distance > TH['amide']['centroid_distance']:
                    continue
                theta_point = pc.amide_center[a1] - pc.amide_center[a2]
                dihedral = abs(group_angle(pc.amide_normal[a1], pc.amide_normal[a2]))
                theta = abs(group_angle(pc.amide_normal[a1], theta_point))
                if dihedral > 30.0 or theta > 30.0:
                    continue
                out.append((a1, a2, distance, dihedral, theta, ct))
        return dict(bgn=np.array([t[0] for t in out], np.int32), end=np.array([t[1] for t in out], np.int32),
                    dist=np.array([t[2] for t in out], np.float32), dihedral=np.array([t[3] for t in out], np.float32),
                    theta=np.array([t[4] for t in out], np.float32), ctype=np.array([t[5] for t in out], np.uint8))

    # interactions.py:1302-1382: float32 amide against float64 ring
    def group_plane(self):
        pc = self.pc
        out = []
        for a in range(pc.n_amides):
            if not self.amide_plus[a]:
                continue
            for r in self._near(pc.ring_center, pc.amide_center[a]):
                if not self.ring_plus[r]:
                    continue
                ct = plane_contact_type(self.amide_sel[a], self.ring_sel[r], self.amide_plus[a], self.ring_plus[r])
                distance = np.linalg.norm(pc.amide_center[a] - pc.ring_center[r])
                if distance > TH['amide']['centroid_distance']:
                    continue
                theta_point = pc.amide_center[a] - pc.ring_center[r]
                dihedral = abs(group_angle(pc.amide_normal[a], pc.ring_normal[r]))
                theta = abs(group_angle(pc.amide_normal[a], theta_point))
                if dihedral > 30.0 or theta > 30.0:
                    continue
                out.append((a, r, distance, dihedral, theta, ct))
        return dict(amide=np.array([t[0] for t in out], np.int32), ring=np.array([t[1] for t in out], np.int32),
                    dist=np.array([t[2] for t in out], np.float64), dihedral=np.array([t[3] for t in out], np.float64),
                    theta=np.array([t[4] for t in out], np.float64), ctype=np.array([t[5] for t in out], np.uint8))


# ---- geometric part of initialize() -----------------------------------------------------------
def ring_geometry(xyz, ring_atoms):
    """interactions.py:1697-1733 -> OBRing::findCenterAndNormal (OpenBabel ring.cpp, third party, restated from its
    published source; PARITY UNPINNED — OpenBabel is not installed here): centre = sum of the atom vectors times
    1/n, normal = sum of cross(v_j - centre, v_j+1 - centre) times 1/n, normalised unless its length is < 2e-6
    (vector3::normalize / IsNearZero; operator/= multiplies by the reciprocal).  float64 on the float32 coordinates."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    ctr, nrm = np.zeros((len(ring_atoms), 3)), np.zeros((len(ring_atoms), 3))
    for r, atoms in enumerate(ring_atoms):
        na = len(atoms)
        c = np.zeros(3)
        for a in atoms:
            c = c + x[a]
        inv = 1.0 / float(na)
        c = c * inv
        n = np.zeros(3)
        for j in range(na):
            v1 = x[atoms[j]] - c
            v2 = x[atoms[0 if j + 1 == na else j + 1]] - c
            n = n + np.array([v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]])
        n = n * inv
        length = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        if not abs(length) < 2e-6:
            n = n * (1.0 / length)
        ctr[r], nrm[r] = c, n
    return ctr, nrm


def amide_geometry(xyz, amide_atoms):
    """interactions.py:1566-1580 with the reference's own NumPy calls: bond centroid of C-N (float32) and the plane
    normal from np.linalg.svd of the centred C, O, N coordinates (float32; the sign is whatever LAPACK returns)."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    at = np.asarray(amide_atoms).reshape(-1, 4)
    ctr, nrm = np.zeros((len(at), 3), np.float32), np.zeros((len(at), 3), np.float32)
    for k, (n_, c_, o_, _) in enumerate(at):
        con = np.array([x[c_], x[o_], x[n_]])                # C-O-N
        cn = np.array([x[c_], x[n_]])                        # C-N
        amide_centroid = con.sum(0) / float(len(con))
        bond_centroid = cn.sum(0) / float(len(cn))
        cog = con - amide_centroid
        u, s_, vh = np.linalg.svd(cog)
        v = vh.conj().transpose()
        a, b, c = v[:, -1]
        ctr[k], nrm[k] = bond_centroid, np.array([a, b, c])
    return ctr, nrm


def ring_residues(xyz, res_id, ring_center):
    """interactions.py:1453-1492: atoms within 3.0 A of the ring centre (Bio.PDB.kdtrees: float64 sum of squares <= r*r),
    nearest by np.linalg.norm(atom.coord - centre) with a strict '<' (first of equals wins; brute force in packed atom
    order here, KD-tree order in the reference), its residue; -1 / -1.0 when no atom qualifies."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    ctr = np.asarray(ring_center, np.float64).reshape(-1, 3)
    res, dist = np.full(len(ctr), -1, np.int32), np.full(len(ctr), -1.0)
    xd = x.astype(np.float64)
    for r, c in enumerate(ctr):
        d = xd - c
        near = np.nonzero(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= 9.0)[0]
        closest = (None, None)
        for a in near:
            distance = np.linalg.norm(x[a] - c)
            if closest[1] is None or distance < closest[1]:
                closest = (a, distance)
        if closest[0] is not None:
            res[r], dist[r] = res_id[closest[0]], closest[1]
    return res, dist
