"""Structures built to sit on the seams of the slab sharding (arpeggio_amd/sharding.py, csrc/arp_shard.h, the ownership rule of
k_search and the ring / amide loops), shared by the CPU test that pins the reference side and the GPU tests that run them
(tests/test_shard_seams.py), and the drivers both use.

Every case carries sentinel atoms at x = 0 and x = x_far, so that the cuts ``sharding._partition`` takes from
``np.linspace(xmin, xmax, world + 1)`` are exact in float32 and float64: 30 for two ranks, 20 / 40 for three, 15 / 30 / 45 for
four (x_far = 60).  ``Case.edges(world)`` asserts them bit for bit.  Atom types, flags and radii come from
``helpers.random_dense_pack``, so that real contact types occur; ids are the order of insertion."""
import ctypes

import numpy as np

from arpeggio_amd import sharding
from helpers import random_dense_pack, tiny_complex

X_FAR = 60.0
CUTS = {2: [30.0], 3: [20.0, 40.0], 4: [15.0, 30.0, 45.0]}
PARK = -40.0                      # y and z of the sentinels: out of everybody's reach
BAGS = ('atom_plane', 'plane_plane', 'group_group', 'group_plane')
BAG_KEYS = {  # (columns compared exactly, angle columns compared with helpers.deg_close): as tests/test_gpu_paths.py
    'plane_plane': (('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end')),
    'atom_plane': (('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',)),
    'group_group': (('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta')),
    'group_plane': (('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta')),
}
BAG_IDS = {  # the two id columns of a bag (the sort key, in this order) and what each counts
    'atom_atom': (('i', 'atom'), ('j', 'atom')), 'plane_plane': (('bgn', 'ring'), ('end', 'ring')),
    'atom_plane': (('ring', 'ring'), ('atom', 'atom')), 'group_group': (('bgn', 'amide'), ('end', 'amide')),
    'group_plane': (('amide', 'amide'), ('ring', 'ring')),
}
RAD_NONE = 0xFFFF


def rad_capacity():
    """Radius pairs the table of a record header holds (``rad_tab`` of arp_rec_header, include/arpeggio_hip.h)."""
    from arpeggio_amd import _capi
    return len(_capi.RecHeader().rad_tab) // 2


def f32_below(b):
    """Largest float32 <= b."""
    v = np.float32(b)
    return v if float(v) <= b else np.nextafter(v, np.float32(-np.inf))


def face_bounds(edges, cutoff=5.0):
    """The float64 face bounds, computed as ``sharding._home_buffer_to_device`` does: [(cut index, side, b)], side -1 = the bound
    of the face the RIGHT slab of the cut sends to the left (x <= cut + halo), +1 = the one the left slab sends (x >= cut - halo)."""
    halo = sharding.halo_width(cutoff)
    out = []
    for k in range(1, len(edges) - 1):
        out.append((k, +1, edges[k] - halo))
        out.append((k, -1, edges[k] + halo))
    return out


class Case:
    def __init__(self, name, pc, worlds, cutoff=5.0, sel=None, cuts=None, tags=None):
        self.name, self.pc, self.worlds, self.cutoff, self.sel = name, pc, tuple(worlds), cutoff, sel
        self.cuts = cuts or CUTS                      # world -> the cuts this case is built for
        self.tags = tags or {}
        for w in self.worlds:
            self.edges(w)

    def edges(self, world):
        x = self.pc.xyz[:, 0]
        e = sharding.slab_edges(float(x.min()), float(x.max()), world)
        want = np.array(self.cuts[world], np.float64)
        assert np.array_equal(e[1:-1].view(np.uint64), want.view(np.uint64)), (self.name, world, e[1:-1], want)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want), 'cuts must be exact in float32'
        return e

    def owners(self, world):
        e = self.edges(world)
        pc = self.pc
        return (sharding.owner_of(pc.xyz[:, 0], e), sharding.owner_of(pc.ring_center[:, 0], e), sharding.owner_of(pc.amide_center[:, 0], e))

    def __repr__(self):
        return self.name


class Slab:
    """Atoms, bonds, hydrogens, rings and amides in the order they are added (= global ids)."""

    def __init__(self, seed):
        d = random_dense_pack(seed, n=96, box=14.0)
        self.donor = d
        self.rng = np.random.default_rng(seed)
        self.xyz, self.tm, self.fl, self.vdw, self.cov, self.res = [], [], [], [], [], []
        self.bonds, self.h, self.nres = [], {}, 0
        self.rc, self.rn, self.rr, self.ac, self.an, self.ar = [], [], [], [], [], []

    def new_res(self):
        self.nres += 1
        return self.nres - 1

    def atom(self, x, y, z, res=None, h=0, inert=False, rad=None, alone=False):
        """alone: no hydrogen / water / metal flag and a residue that is no sequence neighbour of the previous atom's, so that a
        designed pair is neither skipped nor dropped."""
        i = len(self.xyz)
        if alone:
            self.new_res()
        k = i % self.donor.n_atoms
        p = np.array([x, y, z], np.float32)
        self.xyz.append(p)
        self.tm.append(0 if inert else int(self.donor.type_mask[k]))
        self.fl.append(0 if inert or alone else int(self.donor.flags[k]))
        self.vdw.append(float(self.donor.vdw[k]) if rad is None else rad[0])
        self.cov.append(float(self.donor.cov[k]) if rad is None else rad[1])
        self.res.append(self.new_res() if res is None else res)
        if h:
            q = 2.0 * np.pi * (np.arange(h) / h) + 0.37 * i
            self.h[i] = (p.astype(np.float64) + np.stack([0.3 * np.ones(h), 0.95 * np.cos(q), 0.95 * np.sin(q)], axis=1)).tolist()
        return i

    def sentinel(self, x):
        return self.atom(x, PARK, PARK, inert=True)

    def bond(self, i, j):
        self.bonds.append((i, j))

    def unit(self):
        """A normal: one in four anywhere, the others within some 25 degrees of the x axis — the amide loops keep a pair only when
        the normals and the line between the centres agree within 30 degrees, and the cuts are planes of constant x."""
        v = self.rng.standard_normal(3)
        if self.rng.random() >= 0.25:
            v = np.array([1.0, 0.0, 0.0]) + 0.2 * v
        return v / np.linalg.norm(v)

    def ring(self, x, y, z, res, normal=None):
        self.rc.append([x, y, z]); self.rn.append(self.unit() if normal is None else normal); self.rr.append(res)
        return len(self.rc) - 1

    def amide(self, x, y, z, res, normal=None):
        self.ac.append([x, y, z]); self.an.append(self.unit() if normal is None else normal); self.ar.append(res)
        return len(self.ac) - 1

    def soup(self, cut, n, y0=0.0, half=4.5, span=8.0, n_rings=0, n_amides=0):
        """A dense random clump around a cut: residues of three atoms, bonds between close atoms, hydrogens; rings and amides
        among them whose residues are the clump's."""
        rng = self.rng
        first = len(self.xyz)
        res = None
        for k in range(n):
            if k % 3 == 0:
                res = self.new_res()
            self.atom(cut + rng.uniform(-half, half), y0 + rng.uniform(0, span), rng.uniform(0, span), res=res, h=int(rng.integers(0, 3)))
        ids = np.arange(first, first + n)
        x = np.array(self.xyz, np.float64)[ids]
        d = np.linalg.norm(x[:, None] - x[None], axis=2)
        for a, b in zip(*np.nonzero(np.triu(d < 2.2, 1))):
            self.bond(int(ids[a]), int(ids[b]))
        for _ in range(n_rings):
            self.ring(cut + rng.uniform(-half, half), y0 + rng.uniform(0, span), rng.uniform(0, span), int(self.res[int(rng.choice(ids))]))
        for _ in range(n_amides):
            self.amide(cut + rng.uniform(-half, half), y0 + rng.uniform(0, span), rng.uniform(0, span), int(self.res[int(rng.choice(ids))]))
        return ids

    def build(self):
        from arpeggio_amd.core import config
        n, nres = len(self.xyz), self.nres
        rk = np.arange(nres)
        res_flags = np.choose(rk % 3, [config.R_POLYPEPTIDE | config.R_HAS_SEQ, config.R_HAS_SEQ, 0]).astype(np.uint8)
        res_prev, res_next = np.full(nres, -1, np.int32), np.full(nres, -1, np.int32)
        even = rk[(rk % 2 == 0) & (rk + 1 < nres)]
        res_next[even], res_prev[even + 1] = even + 1, even
        tm = np.array(self.tm, np.uint16)
        bonded = np.zeros(n, bool)
        for i, j in self.bonds:
            bonded[i] = bonded[j] = True
        tm[~bonded] &= np.uint16(~config.ATOM_TYPE_BIT['xbond donor'] & 0xFFFF)       # a donor without a neighbour makes the reference raise
        rings = (np.array(self.rc, np.float64).reshape(-1, 3), np.array(self.rn, np.float64).reshape(-1, 3), np.array(self.rr, np.int32))
        amides = (np.array(self.ac, np.float32).reshape(-1, 3), np.array(self.an, np.float32).reshape(-1, 3), np.array(self.ar, np.int32))
        return tiny_complex(np.array(self.xyz, np.float32), vdw=np.array(self.vdw), cov=np.array(self.cov), type_mask=tm,
                            flags=np.array(self.fl, np.uint16), res_id=np.array(self.res, np.int32), res_flags=res_flags, res_prev=res_prev,
                            res_next=res_next, bonds=self.bonds, h=self.h, rings=rings, amides=amides)


# ---- A1: the 4 096-element chunk seam of k_scan_segments -------------------------------------------------------------------------
SCAN_COUNTS = (1, 2, 4095, 4096, 4097, 8192, 8193)
FACES = ('all', 'none', 'two')
IN_FACE_X, FILLER_X = 27.0, (6.0, 9.0, 12.0, 15.0, 18.0)


def _picked(n, face, first=0):
    """Indices of a list of n that a 'two' face holds: 4 095 and 4 096 where the list has them, else its ends (``first``: the lowest
    index that can be moved into the face — the sentinel, home atom 0, cannot)."""
    if face != 'two':
        return set()
    s = {k for k in (4095, 4096) if k < n}
    return s or {k for k in (first, n - 1) if first <= k < n}


def scan_case(n_home, face, n_rings=0, n_amides=0, many_radii=False):
    """World 2; rank 0 owns n_home atoms (the sentinel at x = 0 is home index 0), n_rings rings and n_amides amides.  Hydrogen
    counts cycle 0..3 and bond counts 0..2 over the home indices, so that the three atom scans carry different sums across
    element 4 096.  face: what of rank 0's lists its right face holds — 'all' (cut with x in (-inf, inf)), 'none', or 'two' (the
    items at home indices 4 095 and 4 096 alone).  Filler atoms lie on a 3.2 A lattice in five sheets left of the face."""
    b = Slab(700 + n_home % 97)
    cap = rad_capacity()
    near = _picked(n_home, face, first=1)
    for k in range(n_home):
        rad = (1.2 + 0.002 * (k % (cap + 90)), 0.3 + 0.001 * (k % (cap + 90))) if many_radii else None
        if k == 0:
            b.atom(0.0, PARK, PARK, inert=True, rad=rad)
            continue
        q = k // 5
        x = IN_FACE_X if k in near else FILLER_X[k % 5]
        b.atom(x, 3.2 * (q % 41), 3.2 * (q // 41), res=b.new_res() if k % 3 == 1 else b.nres - 1, h=k % 4, rad=rad)
    for t in range(0, n_home // 3 + 1, 2):                         # degrees 0, 1, 2, 0, 1, 2, ...
        for i, j in ((3 * t + 1, 3 * t + 2), (3 * t + 2, 3 * t + 5), (3 * t + 4, 3 * t + 5)):
            if j < n_home:
                b.bond(i, j)
    for k in range(9):                                              # rank 1: a few atoms beside the cut, then its sentinel
        b.atom(31.0 + 0.5 * k, 3.2 * k, 1.0 + 0.4 * k, h=k % 3, rad=(1.9, 0.9 + 0.01 * k) if many_radii else None)
    b.sentinel(X_FAR)
    for n, add in ((n_rings, b.ring), (n_amides, b.amide)):
        pick = _picked(n, face)
        for k in range(n):
            add(IN_FACE_X if k in pick else 10.0 + (k % 3), 4.0 * (k % 64) + 1.0, -12.0 - 4.0 * (k // 64), k % max(b.nres, 1))
    for k in range(2):
        b.ring(32.0 + k, 5.0, 3.0, b.nres - 2)
        b.amide(33.0 - k, 9.0, 2.0, b.nres - 3)
    bounds = {(0, +1): (-np.inf, np.inf)} if face == 'all' else None
    name = f'scan_{n_home}_{face}_{n_rings}r_{n_amides}m' + ('_radii' if many_radii else '')
    return Case(name, b.build(), (2,), tags=dict(bounds=bounds, n_home=n_home, face=face, many_radii=many_radii))


def scan_cases():
    """(n_home, face, rings, amides): ring / amide counts 0, 1 and 65 spread over the cases, then the long ring and amide lists and
    the radius case."""
    out, groups = [], ((0, 0), (1, 65), (65, 1), (1, 1), (65, 65), (0, 65), (65, 0))
    for k, n in enumerate(SCAN_COUNTS):
        for f, face in enumerate(FACES):
            nr, nm = groups[(k + 2 * f) % len(groups)]
            out.append((n, face, nr, nm, False))
    out += [(40, 'two', 4097, 3, False), (40, 'all', 2, 4098, False), (700, 'two', 1, 1, True)]
    return out


# ---- A2: items on the face bounds and on the cuts ------------------------------------------------------------------------------
def face_case(world, exact=False):
    """At every face bound b: atoms (and amide centres) at the largest float32 <= b, one step below it and at the smallest float32
    > b; ring centres at b and one float64 step to either side; at every cut: atoms on it and one float32 step to either side, a
    ring and an amide on it.  The bounds the halo gives, ``cut +- halo_width()``, are no float32 numbers, so no atom can sit ON one:
    with ``exact`` the faces are cut with the largest float32 <= b instead (tags['bounds']), and the atoms and amide centres there,
    and a fourth ring centre, sit on the bound itself.  tags: (id, cut index, side, the bound in force)."""
    b = Slab(800 + world)
    b.sentinel(0.0)
    edges = sharding.slab_edges(0.0, X_FAR, world)
    tags = dict(bound_atoms=[], bound_rings=[], bound_amides=[], cut_atoms=[], bounds={} if exact else None, on_bound=0)
    y = 0.0
    for k, side, bd in face_bounds(edges):
        lo32 = f32_below(bd)
        if exact:
            bd = float(lo32)
            tags['bounds'][(k - 1, +1) if side > 0 else (k, -1)] = (bd, np.inf) if side > 0 else (-np.inf, bd)
        for x in (np.nextafter(lo32, np.float32(-np.inf)), lo32, np.nextafter(lo32, np.float32(np.inf))):
            res = b.new_res()
            i = b.atom(x, y, 1.0, res=res, h=2)
            j = b.atom(x, y + 1.4, 2.0, res=res, h=1)
            b.bond(i, j)
            b.atom(float(x) + side * 2.5, y + 2.0, 4.0, h=1)                   # company on the inner side of the bound
            tags['bound_atoms'] += [(i, k, side, bd), (j, k, side, bd)]
            tags['bound_amides'].append((b.amide(x, y + 3.0, 2.5, res), k, side, bd))
            tags['on_bound'] += int(float(x) == bd)
            y += 3.3
        for q, x in enumerate((bd, np.nextafter(bd, -np.inf), np.nextafter(bd, np.inf))):
            tags['bound_rings'].append((b.ring(x, y - 6.0 + 1.7 * q, 3.0 + q, b.nres - 1), k, side, bd))
    for k in range(1, world):
        cut = np.float32(edges[k])
        for x in (cut, np.nextafter(cut, np.float32(-np.inf)), np.nextafter(cut, np.float32(np.inf))):
            tags['cut_atoms'].append((b.atom(x, y, 1.5, h=1), k, float(x)))
            y += 2.9
        b.ring(float(cut), y - 4.0, 4.0, b.nres - 1)
        b.amide(cut, y - 2.0, 4.5, b.nres - 2)
    b.sentinel(X_FAR)
    return Case(f'faces_w{world}' + ('_exact' if exact else ''), b.build(), (world,), tags=tags)


# ---- A3: merges that interleave ------------------------------------------------------------------------------------------------
def merge_case(kind):
    """World 3.  'interleave': ids cycle left slab / middle / right slab, all inside the halos of the middle rank, so that its three
    sorted lists interleave element by element (atoms, rings and amides alike); bonds inside a list, across a cut, and to atoms
    beyond the halo; hydrogens on halo atoms; halogen-bond donors whose single-bond neighbour is beyond the halo.
    'empty_home': nothing in the middle slab, atoms within the halo of both its cuts.  'one_halo': the right halo of the middle
    rank is empty."""
    b = Slab(900 + len(kind))
    T = _types()
    b.sentinel(0.0)
    xs = {'interleave': (17.0, 23.0, 43.0), 'empty_home': (16.5, None, 42.5), 'one_halo': (17.0, 23.0, None)}[kind]
    tri = []
    for k in range(40):
        row = []
        for s, x in enumerate(xs):
            if x is None:
                continue
            dx = 2.5 * np.sin(0.7 * k + s) if kind != 'empty_home' else 1.2 * np.sin(0.7 * k + s)
            row.append(b.atom(x + dx + (14.0 if s == 1 and k % 2 else 0.0), 2.1 * (k % 8), 2.3 * (k // 8) + 0.4 * s, h=(k + s) % 4))
        tri.append(row)
        for s, x in enumerate(xs):
            if x is not None and k % 2 == 0:
                b.ring(x + 0.05 * k, 2.0 * (k % 8), 2.0 * (k // 8) + 0.5, b.nres - 1 - s % len(row))
            if x is not None and k % 3 == 0:
                b.amide(x - 0.05 * k, 2.0 * (k % 8) + 1.0, 2.0 * (k // 8), b.nres - 1 - s % len(row))
    for k in range(0, 39):
        if k % 4 == 0:
            for s in range(len(tri[k])):
                b.bond(tri[k][s], tri[k + 1][s])                    # partner in the same list
        if k % 4 == 1 and len(tri[k]) > 1:
            b.bond(tri[k][0], tri[k][1])                            # partner in another list
            b.bond(tri[k + 1][-1], tri[k + 1][-2])
    far = []
    for k in range(6):                                              # beyond every halo of the middle rank: bonded partners that must vanish
        far.append(b.atom(9.0, 3.0 * k, 2.0, h=1))
        b.bond(far[-1], tri[3 * k + 2][0])
        if xs[1] is not None:
            b.bond(far[-1], tri[3 * k + 2][1])
    # halogen-bond donors of the middle slab whose single-bond neighbour (their first bond) lies beyond the left halo: the angle
    # neighbour - donor - acceptor (180 and 90 degrees: a halogen bond and none) can only come from the coordinates in the record
    tags = dict(xbond=[])
    if xs[1] is not None:
        for k, (ax, ay) in enumerate(((3.3, 0.0), (0.0, 3.3))):
            y = 30.0 + 8.0 * k
            nb = b.atom(13.5, y, 20.0, inert=True)
            d = b.atom(20.5, y, 20.0, inert=True)
            a = b.atom(20.5 + ax, y + ay, 20.0, inert=True)
            b.bond(nb, d)
            b.tm[d], b.tm[a] = T['xbond donor'], T['xbond acceptor']
            tags['xbond'].append((nb, d, a))
    b.sentinel(X_FAR)
    return Case(f'merge_{kind}', b.build(), (3,), tags=tags)


def _types():
    from arpeggio_amd.core import config
    return config.ATOM_TYPE_BIT


# ---- B: ownership at the cuts ----------------------------------------------------------------------------------------------------
def _thirds(pc):
    return (pc.res_id % 3 == 0).astype(np.uint8)


def case_thin():
    """1: a dense soup thinner than two halos around the cut of two ranks: both shards hold every atom of it."""
    d = random_dense_pack(61, n=260, box=11.0)
    rng = np.random.default_rng(61)
    b = Slab(61)
    b.sentinel(0.0)
    b.nres += d.n_residues
    off = np.array([24.5, 0.0, 0.0])
    for i in range(d.n_atoms):
        b.xyz.append((d.xyz[i].astype(np.float64) + off).astype(np.float32))
        b.tm.append(int(d.type_mask[i])); b.fl.append(int(d.flags[i])); b.vdw.append(float(d.vdw[i])); b.cov.append(float(d.cov[i]))
        b.res.append(1 + int(d.res_id[i]))
        if d.h_off[i + 1] > d.h_off[i]:
            b.h[i + 1] = (d.h_xyz[d.h_off[i]:d.h_off[i + 1]] + off).tolist()
    for i in range(d.n_atoms):
        for j in d.bond_idx[d.bond_off[i]:d.bond_off[i + 1]]:
            if i < j:
                b.bond(i + 1, int(j) + 1)
    for k in range(30):
        p = rng.random(3) * 11.0 + off
        b.ring(p[0], p[1], p[2], int(rng.integers(1, b.nres)))
        p = rng.random(3) * 11.0 + off
        b.amide(p[0], p[1], p[2], int(rng.integers(1, b.nres)))
    b.sentinel(X_FAR)
    pc = b.build()
    assert pc.xyz[1:-1, 0].min() >= 30.0 - sharding.halo_width() and pc.xyz[1:-1, 0].max() <= 30.0 + sharding.halo_width()
    return Case('thin', pc, (2,), sel=_thirds(pc))


def case_on_cut():
    """2: pairs on the cuts of two, three and four ranks: both atoms at x = cut, the lower id left and the higher right, and the
    mirror image; a soup around each cut for company."""
    b = Slab(62)
    b.sentinel(0.0)
    tags = dict(pairs=[])
    for n, cut in enumerate((15.0, 20.0, 30.0, 40.0, 45.0)):
        y = 11.0 * n
        tags['pairs'].append((b.atom(cut, y, 0.0, h=1, alone=True), b.atom(cut, y + 3.1, 0.0, alone=True)))
        tags['pairs'].append((b.atom(cut - 1.5, y, 4.0, alone=True), b.atom(cut + 1.5, y, 4.0, h=2, alone=True)))
        hi = b.atom(cut + 1.5, y, 8.0, alone=True)
        tags['pairs'].append((hi, b.atom(cut - 1.5, y, 8.0, alone=True)))
        b.soup(cut, 18, y0=y, n_rings=2, n_amides=2)
    b.sentinel(X_FAR)
    pc = b.build()
    return Case('on_cut', pc, (2, 3, 4), sel=_thirds(pc), tags=tags)


def case_cutoff6():
    """3: cutoff 6.0 (below the halo): an atom at cut - 6.0 and a partner on the cut with equal y and z: the distance sits on the
    inclusive float64 test of the search, and the atom is inside the face."""
    b = Slab(63)
    b.sentinel(0.0)
    tags = dict(pairs=[])
    for n, cut in enumerate((20.0, 30.0, 40.0)):
        y = 12.0 * n
        assert float(np.float32(cut - 6.0)) == cut - 6.0
        tags['pairs'].append((b.atom(cut - 6.0, y, 0.0, h=1, alone=True), b.atom(cut, y, 0.0, alone=True)))
        on = b.atom(cut, y + 5.0, 9.0, alone=True)
        tags['pairs'].append((on, b.atom(cut - 6.0, y + 5.0, 9.0, alone=True)))
        b.soup(cut, 15, y0=y, n_rings=1, n_amides=1)
    b.sentinel(X_FAR)
    pc = b.build()
    return Case('cutoff6', pc, (2, 3), cutoff=6.0, sel=_thirds(pc), tags=tags)


def case_reach():
    """4: selection reach across the cut of two ranks.  'plain': S selected on rank 0 at cut - 6.0, M unselected on the cut (rank 1),
    in selection_plus only because of S, T further right in contact with M (and in selection_plus by a selected atom of its own).
    'mirror': the same reflected.  'beyond' (both ways): M's selector lies beyond the halo of the rank that owns M's partner, so
    that M's bit can only arrive through the exchange."""
    b = Slab(64)
    b.sentinel(0.0)
    sel, tags = [], dict(trios=[])

    def trio(name, xs, y, order=(0, 1, 2, 3)):
        ids = [None] * 4                              # S, M, T, and the selected atom that brings T into selection_plus
        for k in order:
            ids[k] = b.atom(xs[k], y, 5.0, alone=True)
        sel.extend([ids[0], ids[3]])
        tags['trios'].append((name, ids[0], ids[1], ids[2]))

    trio('plain', (24.0, 30.0, 33.0, 38.5), 0.0)
    trio('mirror', (35.5, 29.5, 26.5, 21.0), 10.0)
    trio('beyond', (37.0, 31.0, 28.0, 23.0), 20.0)                          # S beyond rank 0's halo; T (rank 0) - M (rank 1), M first
    trio('beyond_t_first', (37.0, 31.0, 28.0, 23.0), 30.0, (2, 3, 0, 1))    # the same with T's id below M's
    trio('beyond_mirror', (23.0, 29.0, 32.0, 37.0), 40.0)                   # S beyond rank 1's halo; M (rank 0) - T (rank 1)
    trio('beyond_mirror_t_first', (23.0, 29.0, 32.0, 37.0), 50.0, (2, 3, 0, 1))
    b.soup(30.0, 24, y0=60.0, n_rings=2, n_amides=2)
    b.sentinel(X_FAR)
    pc = b.build()
    s = np.zeros(pc.n_atoms, np.uint8)
    s[sel] = 1
    s[pc.res_id == pc.res_id[-2]] = 1                           # and one residue of the soup
    return Case('reach', pc, (2,), sel=s, tags=tags)


def case_res_sets():
    """5: a residue with atoms on both sides of the cut whose only selected atom lies further than the halo from it; a ring and an
    amide of that residue owned by the other rank: their set membership arrives only through the reduction of the residue sets."""
    b = Slab(65)
    b.sentinel(0.0)
    sel = []
    for k, (far_x, near_x, sign) in enumerate(((10.0, 32.0, 1.0), (50.0, 28.0, -1.0))):
        y = 14.0 * k
        res = b.new_res()
        sel.append(b.atom(far_x, y, 3.0, res=res))
        b.atom(near_x, y, 3.0, res=res)
        b.ring(near_x + sign, y + 1.0, 4.0, res)
        b.ring(near_x + 2 * sign, y + 3.5, 5.0, res)
        b.amide(near_x + sign, y + 2.0, 2.0, res)
        b.amide(near_x + 2 * sign, y + 4.0, 1.0, res)
        other = b.soup(near_x + 1.5 * sign, 12, y0=y, half=2.0, span=6.0, n_rings=2, n_amides=2)
        sel.append(int(other[0]))
    b.sentinel(X_FAR)
    pc = b.build()
    s = np.zeros(pc.n_atoms, np.uint8)
    s[sel] = 1
    return Case('res_sets', pc, (2,), sel=s)


def case_planes():
    """6: ring-ring, amide-amide and amide-ring pairs with their centres on opposite sides of a cut, the lower id on the left and on
    the right; a ring centre on the cut; atoms beside rings owned by the other rank; rings whose residue lies across the cut."""
    b = Slab(66)
    T = _types()
    b.sentinel(0.0)
    for n, cut in enumerate((20.0, 30.0, 40.0)):
        y = 13.0 * n
        left = [b.atom(cut - 2.0, y + 2.0 * k, 2.0 + k, h=k % 2) for k in range(3)]
        right = [b.atom(cut + 2.0, y + 2.0 * k, 3.0 + k, h=(k + 1) % 2) for k in range(3)]
        rl, rr = b.res[left[0]], b.res[right[0]]
        for i in (left[0], right[0]):                                                # atoms a ring across the cut has a contact with
            b.tm[i] = (b.tm[i] | T['hbond donor'] | T['pos ionisable']) & ~T['aromatic']
            b.fl[i] = 0
        b.ring(cut - 1.5, y, 1.0, rr); b.ring(cut + 1.5, y, 2.0, rl)             # lower id left; residues across the cut
        b.ring(cut + 1.2, y + 4.0, 1.0, rr); b.ring(cut - 1.2, y + 4.0, 2.0, rl)    # lower id right
        b.ring(cut, y + 2.0, 4.0, b.res[left[1]])                                   # on the cut
        b.amide(cut - 1.5, y + 1.0, 3.0, rl); b.amide(cut + 1.5, y + 1.0, 4.0, rr)
        b.amide(cut + 1.2, y + 3.0, 5.0, rr); b.amide(cut - 1.2, y + 3.0, 4.0, rl)
        b.soup(cut, 15, y0=y, half=3.0, span=6.0, n_rings=4, n_amides=4)
    b.sentinel(X_FAR)
    pc = b.build()
    return Case('planes', pc, (2, 3), sel=_thirds(pc))


NARROW_INNER = 6.0 + 5.0 / 4096.0           # the inner slab of three: about 1e-3 A wider than the halo, a dyadic number


def case_narrow3():
    """7: three ranks whose inner slab is only just wider than the halo: the atoms of the middle slab sit in both neighbours' halos."""
    assert 5e-4 < NARROW_INNER - sharding.halo_width() < 2e-3
    x_far = 3.0 * NARROW_INNER
    assert float(np.float32(x_far)) == x_far
    b = Slab(67)
    b.sentinel(0.0)
    b.soup(x_far / 2.0, 150, half=x_far / 2.0 - 0.01, span=9.0, n_rings=24, n_amides=24)
    b.sentinel(x_far)
    pc = b.build()
    return Case('narrow3', pc, (3,), sel=_thirds(pc), cuts={3: [NARROW_INNER, 2.0 * NARROW_INNER]})


def ownership_cases():
    inter = merge_case('interleave')                  # and the interleaved merge of A3, for what a pass makes of it
    inter.sel = _thirds(inter.pc)
    return [case_thin(), case_on_cut(), case_cutoff6(), case_reach(), case_res_sets(), case_planes(), case_narrow3(), inter]


# ---- the reference: the oracle on the whole structure ---------------------------------------------------------------------------
def _sorted_bag(name, cols):
    (k1, _), (k2, _) = BAG_IDS[name]
    o = np.lexsort((cols[k2], cols[k1]))
    return {k: np.asarray(v)[o] for k, v in cols.items() if isinstance(v, np.ndarray) and np.asarray(v).shape[:1] == o.shape}


def oracle_bags(oc, cutoff, comp=0.1, seq=False):
    aa = oc.atom_contacts(cutoff, comp, seq, use_grid=False)
    assert aa.get('err', 0) == 0
    out = {'atom_atom': {k: aa[k] for k in ('i', 'j', 'dist', 'sift', 'ctype')}, 'plane_plane': oc.plane_plane(),
           'atom_plane': oc.atom_plane(), 'group_group': oc.group_group(), 'group_plane': oc.group_plane()}
    return {k: _sorted_bag(k, v) for k, v in out.items()}


def oracle_reference(case, whole):
    """The five bags of the unsharded structure, each sorted by its id columns, and the oracle complex (its selection masks)."""
    import oracle
    oc = oracle.OracleComplex(case.pc)
    oc.make_selection(None if whole else case.sel, use_grid=False)
    return oracle_bags(oc, case.cutoff), oc


def to_global(bags, sh):
    """Local ids of one rank's bags -> global ids (sh: a Shard or a DeviceShard)."""
    maps = {'atom': sh.global_id, 'ring': sh.ring_gid, 'amide': sh.amide_gid}
    out = {}
    for name, cols in bags.items():
        cols = dict(cols)
        for key, what in BAG_IDS[name]:
            cols[key] = np.asarray(maps[what])[cols[key]].astype(np.int32)
        out[name] = cols
    return out


def union(per_rank):
    """The ranks' bags concatenated — nothing removed — and sorted by their id columns."""
    out = {}
    for name in per_rank[0]:
        keys = [k for k, v in per_rank[0][name].items() if isinstance(v, np.ndarray)]
        out[name] = _sorted_bag(name, {k: np.concatenate([p[name][k] for p in per_rank]) for k in keys})
    return out


def owned_by(case, world, exp, rank):
    """The records of ``exp`` (global ids) that ``rank`` must emit — no other rank: a pair belongs to the rank that owns its bgn
    atom (the lower id), the lower ring of a ring pair, the bgn amide of an amide pair, the ring of an atom-ring pair and the amide of
    an amide-ring pair."""
    a_own, r_own, m_own = case.owners(world)
    key = {'atom_atom': lambda c: a_own[c['i']], 'plane_plane': lambda c: r_own[np.minimum(c['bgn'], c['end'])],
           'atom_plane': lambda c: r_own[c['ring']], 'group_group': lambda c: m_own[c['bgn']], 'group_plane': lambda c: m_own[c['amide']]}
    return {name: {k: v[key[name](cols) == rank] for k, v in cols.items()} for name, cols in exp.items()}


def assert_ranks_and_union_equal(case, world, per_rank, exp, where):
    """Every rank's records are the oracle's records that rank owns; and their concatenation is the oracle's list."""
    for rank, mine in enumerate(per_rank):
        assert_union_equals(union([mine]), owned_by(case, world, exp, rank), where + (f'rank {rank}',))
    assert_union_equals(union(per_rank), exp, where)


def assert_union_equals(got, exp, where):
    """Ids, distance, SIFt and contact type to the bit, angles within the suite's 1e-4 degrees, and the same length: a record
    emitted twice or not at all fails."""
    from helpers import assert_planes_equal
    a, e = got['atom_atom'], exp['atom_atom']
    assert len(a['i']) == len(e['i']), (where, 'atom_atom', len(a['i']), len(e['i']))
    for k in ('i', 'j', 'sift', 'ctype'):
        assert np.array_equal(a[k], e[k]), (where, 'atom_atom', k)
    assert np.array_equal(a['dist'].view(np.uint32), e['dist'].view(np.uint32)), (where, 'atom_atom dist')
    for bag in BAGS:
        exact, angles = BAG_KEYS[bag]
        assert len(got[bag][exact[0]]) == len(exp[bag][exact[0]]), (where, bag, len(got[bag][exact[0]]), len(exp[bag][exact[0]]))
        try:
            assert_planes_equal(got[bag], exp[bag], exact, angles)
        except AssertionError as err:
            raise AssertionError(f'{where} {bag}: {err}') from None


# ---- the same on the CPU: host shards, the oracle per shard, the ownership rule ----------------------------------------------
def _with_ghost_neighbours(sh, masks):
    """The shard's single-bond neighbours are inline coordinates; the oracle wants an index: inert ghost atoms are appended
    (as tests/test_sharding.py does)."""
    from arpeggio_amd.core.packed import PackedComplex
    pc = sh.pc
    n = pc.n_atoms
    need = np.nonzero(sh.sb_has)[0]
    g = need.size
    sb = pc.sb_nbr.copy()
    sb[need] = n + np.arange(g)
    pc2 = PackedComplex(
        xyz=np.concatenate([pc.xyz, sh.sb_xyz[need]]), vdw=np.concatenate([pc.vdw, np.ones(g)]), cov=np.concatenate([pc.cov, np.ones(g)]),
        type_mask=np.concatenate([pc.type_mask, np.zeros(g, np.uint16)]), flags=np.concatenate([pc.flags, np.zeros(g, np.uint16)]),
        res_id=np.concatenate([pc.res_id, pc.n_residues + np.arange(g)]), res_flags=np.concatenate([pc.res_flags, np.zeros(g, np.uint8)]),
        res_prev=np.concatenate([pc.res_prev, np.full(g, -1)]), res_next=np.concatenate([pc.res_next, np.full(g, -1)]),
        bond_off=np.concatenate([pc.bond_off, np.full(g, pc.bond_off[-1])]), bond_idx=pc.bond_idx,
        h_off=np.concatenate([pc.h_off, np.full(g, pc.h_off[-1])]), h_xyz=pc.h_xyz, sb_nbr=np.concatenate([sb, np.full(g, -1)]),
        ring_center=pc.ring_center, ring_normal=pc.ring_normal, ring_res=pc.ring_res,
        amide_center=pc.amide_center, amide_normal=pc.amide_normal, amide_res=pc.amide_res)
    z = np.zeros(g, np.uint8)
    return pc2, np.concatenate([masks['sel'], z]), np.concatenate([masks['plus'], z])


def shard_bags_cpu(sh, masks, cutoff):
    """The oracle on one shard with the given masks, then the ownership rule: the bgn atom, the lower ring, the bgn amide, the
    ring of an atom-ring pair and the amide of an amide-ring pair must be home.  Global ids."""
    import oracle
    pc2, sel, plus = _with_ghost_neighbours(sh, masks)
    oc = oracle.OracleComplex(pc2, in_sel=sel, in_plus=plus)
    oc.ring_sel[:] = masks['ring_sel']; oc.ring_plus[:] = masks['ring_plus']
    oc.amide_sel[:] = masks['amide_sel']; oc.amide_plus[:] = masks['amide_plus']
    bags = oracle_bags(oc, cutoff)
    keep = {'atom_atom': sh.is_home[bags['atom_atom']['i']] == 1,
            'plane_plane': sh.ring_home[np.minimum(bags['plane_plane']['bgn'], bags['plane_plane']['end'])] == 1,
            'atom_plane': sh.ring_home[bags['atom_plane']['ring']] == 1,
            'group_group': sh.amide_home[bags['group_group']['bgn']] == 1,
            'group_plane': sh.amide_home[bags['group_plane']['amide']] == 1}
    return to_global({name: {k: v[keep[name]] for k, v in cols.items()} for name, cols in bags.items()}, sh)


def combine_on_host(shards, local_plus):
    """What the two exchanges of a pass do, in NumPy: halo atoms take their selection_plus bit from their owner, the residue sets
    (made from each rank's home atoms) are OR-ed.  Returns (masks per rank, residue sets per rank before the merge)."""
    world = len(shards)
    plus = [np.asarray(p, np.uint8).copy() for p in local_plus]
    for r, sh in enumerate(shards):
        for side in (-1, +1):
            nb = r + side
            if 0 <= nb < world:
                ids = shards[nb].send_right if side == -1 else shards[nb].send_left
                src = sharding._lookup(shards[nb].global_id, ids)
                dst = np.nonzero(sh.origin == side)[0]
                assert len(src) == len(dst)
                plus[r][dst] = local_plus[nb][src]
    sets = []
    for sh, p in zip(shards, plus):
        nres = sh.n_res_global
        res = np.zeros(2 * nres, np.uint8)
        hm = sh.is_home == 1
        res[sh.pc.res_id[hm & (sh.sel == 1)]] = 1
        res[nres + sh.pc.res_id[hm & (p == 1)]] = 1
        sets.append(res)
    merged = np.maximum.reduce(sets)
    masks = []
    for sh, p in zip(shards, plus):
        nres = sh.n_res_global
        pick = lambda r, m: np.where(r >= 0, m[np.maximum(r, 0)], 0).astype(np.uint8)      # noqa: E731
        masks.append(dict(sel=sh.sel, plus=p, ring_sel=pick(sh.pc.ring_res, merged[:nres]), ring_plus=pick(sh.pc.ring_res, merged[nres:]),
                          amide_sel=pick(sh.pc.amide_res, merged[:nres]), amide_plus=pick(sh.pc.amide_res, merged[nres:])))
    return masks, sets


def cpu_union(case, world, whole):
    """Host shards, the oracle per shard (local expansion, the two exchanges in NumPy), the ownership rule.  Returns dict(union, shards,
    masks, sets = the residue sets before the merge, local_plus = each shard's own expansion)."""
    import oracle
    sel = None if whole else case.sel
    shards = [sharding.make_shard_local(case.pc, r, world, sel, cutoff=case.cutoff) for r in range(world)]
    if whole:
        one = lambda v: (np.asarray(v) >= 0).astype(np.uint8)                               # noqa: E731
        masks = [dict(sel=np.ones(sh.pc.n_atoms, np.uint8), plus=np.ones(sh.pc.n_atoms, np.uint8), ring_sel=one(sh.pc.ring_res),
                      ring_plus=one(sh.pc.ring_res), amide_sel=one(sh.pc.amide_res), amide_plus=one(sh.pc.amide_res)) for sh in shards]
        sets = local = None
    else:
        local = [oracle.OracleComplex(sh.pc).make_selection(sh.sel, use_grid=False) for sh in shards]
        masks, sets = combine_on_host(shards, local)
    per_rank = [shard_bags_cpu(sh, m, case.cutoff) for sh, m in zip(shards, masks)]
    return dict(per_rank=per_rank, union=union(per_rank), shards=shards, masks=masks, sets=sets, local_plus=local)


def crossing(case, world, bags):
    """Per bag: how many records join items owned by different ranks, split by whether the first id column's item lies left or right."""
    a_own, r_own, m_own = case.owners(world)
    own = {'atom': a_own, 'ring': r_own, 'amide': m_own}
    out = {}
    for name, cols in bags.items():
        (k1, w1), (k2, w2) = BAG_IDS[name]
        o1, o2 = own[w1][cols[k1]], own[w2][cols[k2]]
        out[name] = (int((o1 < o2).sum()), int((o1 > o2).sum()))
    return out


# ---- shards on the device: one context per rank on one GPU ----------------------------------------------------------------------
def host_shards(case, world, sel, bounds=None):
    """``sharding.make_shard_local`` — or, with ``bounds`` {(rank, side): (x_lo, x_hi)}, the same assembly (``pack_records`` /
    ``assemble_shard``) with those faces cut by the given inclusive bounds instead of the halo's."""
    if not bounds:
        return [sharding.make_shard_local(case.pc, r, world, sel, cutoff=case.cutoff) for r in range(world)]
    pc = case.pc
    halo = sharding.halo_width(case.cutoff)
    edges, a_own, r_own, m_own = sharding._partition(pc, world, halo)

    def face(rank, side):
        if (rank, side) not in bounds:
            return sharding._face_sets(pc, edges, a_own, r_own, m_own, rank, side, halo)
        lo, hi = bounds[(rank, side)]
        inside = lambda x: (np.asarray(x, np.float64) >= lo) & (np.asarray(x, np.float64) <= hi)      # noqa: E731
        return (np.nonzero((a_own == rank) & inside(pc.xyz[:, 0]))[0], np.nonzero((r_own == rank) & inside(pc.ring_center[:, 0]))[0],
                np.nonzero((m_own == rank) & inside(pc.amide_center[:, 0]))[0])

    out = []
    for rank in range(world):
        home = sharding.pack_records(pc, np.nonzero(a_own == rank)[0], np.nonzero(r_own == rank)[0], np.nonzero(m_own == rank)[0], sel)
        halos, sends = {}, {}
        for side, nb in ((-1, rank - 1), (+1, rank + 1)):
            if 0 <= nb < world:
                halos[side] = sharding.pack_records(pc, *face(nb, -side), sel)
                sends[side] = face(rank, side)[0]
        sh = sharding.assemble_shard(home, halos, pc.n_residues, rank, world)
        sh.send_left, sh.send_right, sh.halo = sends.get(-1), sends.get(+1), halo
        out.append(sh)
    return out


def device_shards(capi, case, world, sel, whole, bounds=None):
    """One context per rank on device 0; the face buffers a rank cuts out are handed to its neighbours' contexts as device
    pointers (what RCCL delivers).  ``bounds`` as for ``host_shards``: those faces are cut again with the given bounds."""
    pc = case.pc
    ctxs = [capi.Context(0) for _ in range(world)]
    step1 = []
    for r, c in enumerate(ctxs):
        faces, book = sharding.shard_home_to_device(c, pc, r, world, sel, case.cutoff)
        for (rank, side), (lo, hi) in (bounds or {}).items():
            if rank == r:
                faces[side] = c.shard_pack_face(0 if side < 0 else 1, lo, hi)
                a_own = case.owners(world)[0]
                ids = np.nonzero(a_own == r)[0]
                hx = pc.xyz[ids, 0].astype(np.float64)
                book['sends'][side] = ids[(hx >= lo) & (hx <= hi)]
        step1.append((faces, book))
    shards = []
    for r, c in enumerate(ctxs):
        received = {}
        if r > 0:
            received[-1] = step1[r - 1][0][+1]
        if r + 1 < world:
            received[+1] = step1[r + 1][0][-1]
        shards.append(sharding.finish_shard_on_device(c, received, step1[r][1], whole_structure=whole))
    return ctxs, shards


def expected_rad_idx(blob):
    """Per atom: the index of the first entry in use of the blob's ``rad_tab`` whose two doubles equal the atom's {vdw, cov} bit for
    bit, 0xFFFF where there is none (``blob``: ``_capi.unpack_blob`` of the resident structure)."""
    n_rad = int(blob['header'].n_rad)
    tab = np.ascontiguousarray(blob['rad_tab'][:n_rad]).view(np.uint64).reshape(-1, 2)
    rad = np.ascontiguousarray(blob['rad']).view(np.uint64).reshape(-1, 2)
    if n_rad == 0 or len(rad) == 0:
        return np.full(len(rad), RAD_NONE, np.uint16)
    eq = (rad[:, None, :] == tab[None, :, :]).all(axis=2)
    return np.where(eq.any(axis=1), eq.argmax(axis=1), RAD_NONE).astype(np.uint16)


BLOB_ARRAYS = ('type_mask', 'flags', 'res_id', 'res_flags', 'res_prev', 'res_next', 'bond_off', 'bond_idx', 'h_off', 'h_xyz', 'ring_center',
               'ring_normal', 'ring_res', 'amide_center', 'amide_normal', 'amide_res')


def assert_device_shard_equals_host(capi, c, ds, hs, where):
    """Id maps, origins, send lists and every resident array of a device-assembled shard against the host-assembled one."""
    for k in ('global_id', 'origin', 'is_home', 'sel', 'ring_gid', 'ring_home', 'amide_gid', 'amide_home'):
        assert np.array_equal(getattr(ds, k), getattr(hs, k)), (where, k)
    for k in ('send_left', 'send_right'):
        x, y = getattr(ds, k), getattr(hs, k)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (where, k)
    got = capi.unpack_blob(c.get_blob())
    pc = hs.pc
    assert np.array_equal(got['xyz'], pc.xyz), (where, 'xyz')
    assert np.array_equal(got['rad'][:, 0], pc.vdw) and np.array_equal(got['rad'][:, 1], pc.cov), (where, 'rad')
    for k in BLOB_ARRAYS:
        assert np.array_equal(got[k], getattr(pc, k)), (where, k)
    assert np.all(got['sb_nbr'] == -1), (where, 'sb_nbr')
    assert np.array_equal(got['rad_idx'], expected_rad_idx(got)), (where, 'rad_idx')
    return got


def assert_pass_equal(c, ds, ref, hs, whole, cutoff, where):
    """The pass over the device-assembled shard against the pass over the host-assembled one uploaded into ``ref`` (this is where
    the single-bond-neighbour coordinates of the records show): every column of every bag, bit for bit."""
    sharding.upload_shard(ref, hs, whole_structure=whole)
    if whole:
        n_dev, n_host = sharding.run_shard_whole_structure(c, cutoff, sh=ds), sharding.run_shard_whole_structure(ref, cutoff, sh=hs)
    else:
        n_dev, n_host = c.run_launch(cutoff), ref.run_launch(cutoff)
    assert dict(n_dev) == dict(n_host), (where, n_dev, n_host)
    a, b = c.atom_contacts_fetch(n_dev['atom_atom']), ref.atom_contacts_fetch(n_host['atom_atom'])
    for k in a:
        assert np.array_equal(a[k], b[k]), (where, 'atom_atom', k)
    for bag in BAGS:
        x, y = c.fetch_bag(bag), ref.fetch_bag(bag)
        for k in x:
            assert np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == 'f'), (where, bag, k)
    return n_dev


# ---- the three-stage pass between contexts on one GPU -----------------------------------------------------------------------------
def _hip():
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    return hip


def staged_exchange(ctxs, shards, names, *stage_args):
    """arp_run_stage 0 / 1 / 2 on every context (each holding its shard), and between the stages what ``sharding.DeviceExchange``
    does over RCCL: every shard's halo atoms take their selection_plus bit from the owner's buffer, the residue sets are OR-ed over
    the shards — here with plain hipMemcpy on the contexts' device buffers (arp_device_buffer).  ``shards``: Shard or DeviceShard.
    Returns (atom contacts per rank, unsorted; {bag: [per rank]}; the residue sets per rank before the merge)."""
    hip = _hip()
    world = len(ctxs)

    def read(c, which):
        ptr, nb = c.device_buffer(which)
        out = np.empty(nb, np.uint8)
        assert hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), nb, 2) == 0      # device -> host
        return out

    def write(c, which, arr):
        ptr, nb = c.device_buffer(which)
        arr = np.ascontiguousarray(arr, np.uint8)
        assert arr.size == nb
        assert hip.hipMemcpy(ctypes.c_void_p(ptr), arr.ctypes.data_as(ctypes.c_void_p), nb, 1) == 0      # host -> device

    for c in ctxs:
        c.run_stage(0, *stage_args)
    assert hip.hipDeviceSynchronize() == 0
    plus = [read(c, c.BUF_PLUS) for c in ctxs]
    new_plus = [p.copy() for p in plus]
    for r, sh in enumerate(shards):
        for side in (-1, +1):
            nb = r + side
            if 0 <= nb < world:
                ids = shards[nb].send_right if side == -1 else shards[nb].send_left      # what the neighbour sends towards r
                src = sharding._lookup(shards[nb].global_id, ids)
                dst = np.nonzero(sh.origin == side)[0]
                assert len(src) == len(dst)
                new_plus[r][dst] = plus[nb][src]
    for c, p_ in zip(ctxs, new_plus):
        write(c, c.BUF_PLUS, p_)
    for c in ctxs:
        c.run_stage(1, *stage_args)
    assert hip.hipDeviceSynchronize() == 0
    sets = [read(c, c.BUF_RES_SETS) for c in ctxs]
    merged = np.maximum.reduce(sets)
    for c in ctxs:
        write(c, c.BUF_RES_SETS, merged)
    parts, bags = [], {k: [] for k in names}
    for c in ctxs:
        k = c.run_stage(2, *stage_args)
        parts.append(c.atom_contacts_fetch(k['atom_atom'], sort=False))
        for b in names:
            bags[b].append(c.fetch_bag(b))
    return parts, bags, sets


def gpu_union(capi, case, world, whole):
    """Device-assembled shards of the case, one flow of the pass, the ranks' records concatenated (a context that holds a shard
    reports global ids).
    Returns (the bags per rank, residue sets before the merge or None)."""
    ctxs, dss = device_shards(capi, case, world, None if whole else case.sel, whole)
    try:
        sets = None
        if whole:
            per_rank = []
            for c, ds in zip(ctxs, dss):
                n = sharding.run_shard_whole_structure(c, case.cutoff, sh=ds)
                bags = {'atom_atom': c.atom_contacts_fetch(n['atom_atom'])}
                bags.update({b: c.fetch_bag(b) for b in BAGS})
                per_rank.append({k: {f: v for f, v in cols.items() if f in _columns(k)} for k, cols in bags.items()})
        else:
            for ds in dss:
                sharding._check_radius(ds, case.cutoff)
            parts, bags, sets = staged_exchange(ctxs, dss, BAGS, case.cutoff, 0.1, False)
            per_rank = []
            for r, ds in enumerate(dss):
                mine = {'atom_atom': parts[r]}
                mine.update({b: bags[b][r] for b in BAGS})
                per_rank.append({k: {f: v for f, v in cols.items() if f in _columns(k)} for k, cols in mine.items()})
        return per_rank, sets
    finally:
        for c in ctxs:
            c.close()


def _columns(name):
    return ('i', 'j', 'dist', 'sift', 'ctype') if name == 'atom_atom' else BAG_KEYS[name][0] + BAG_KEYS[name][1]
