"""Two independent restatements must agree: oracle/ref_py.py (real NumPy calls, the reference's idiom) and
oracle/ref_c.c (explicit arithmetic model).  Agreement to the last bit re-validates the model of NumPy's
float32 / float64 dot products and NEP-50 comparisons on this machine.  CPU only."""
import numpy as np
import pytest

import oracle
from oracle.ref_py import RefPy
from helpers import known_answer_packs, random_dense_pack


def _same(a, b, name=''):
    assert len(a['i']) == len(b['i']), name
    for k in ('i', 'j', 'sift', 'ctype'):
        assert np.array_equal(a[k], b[k]), (name, k)
    assert np.array_equal(a['dist'].view(np.uint32), b['dist'].view(np.uint32)), name


def test_known_answer_packs_both_orientations():
    for name, pc in known_answer_packs():
        oc = oracle.OracleComplex(pc)
        rp = RefPy(pc)
        for b in range(pc.n_atoms):
            for e in range(pc.n_atoms):
                if b == e:
                    continue
                ok, d, s, ct, err = oc.pair_contact(b, e)
                try:
                    r = rp.pair(b, e)
                except AttributeError:
                    assert err == -4, name
                    continue
                assert err == 0, name
                assert (r is not None) == ok, (name, b, e)
                if ok:
                    assert (np.float32(r[0]).view(np.uint32), r[1], r[2]) == (np.float32(d).view(np.uint32), s, ct), (name, b, e)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_dense_soup_full_loop(seed):
    pc = random_dense_pack(seed, n=260, box=12.0)
    rng = np.random.default_rng(seed)
    sel = (rng.random(pc.n_atoms) < 0.4).astype(np.uint8)
    oc = oracle.OracleComplex(pc)
    plus = oc.make_selection(sel, use_grid=False)
    rp = RefPy(pc, sel, plus)
    for seq_adj, comp in ((False, 0.1), (True, 0.33)):
        _same(rp.atom_contacts(5.0, comp, seq_adj), oc.atom_contacts(5.0, comp, seq_adj, use_grid=False), f'seed{seed}')


# ---- the four ring / amide loops --------------------------------------------------------------------------------------------------------
PLANE_BAGS = (('plane_plane', ('bgn', 'end', 'type1', 'type2', 'ctype'), ('dihedral', 'theta_bgn', 'theta_end')),
              ('atom_plane', ('atom', 'ring', 'mask', 'ctype'), ('theta',)),
              ('group_group', ('bgn', 'end', 'ctype'), ('dihedral', 'theta')),
              ('group_plane', ('amide', 'ring', 'ctype'), ('dihedral', 'theta')))


def _same_planes(rp, oc, name):
    """Ids, classes, masks and contact types exactly, distances to the last bit, reported angles by deg_close (NumPy's arccos and
    glibc's acos differ in the last place; a decision that differs shows as a different record)."""
    from helpers import deg_close
    n = 0
    for bag, exact, angles in PLANE_BAGS:
        a, b = getattr(rp, bag)(), getattr(oc, bag)()
        for k in exact:
            assert np.array_equal(a[k], b[k]), (name, bag, k)
        assert a['dist'].dtype == b['dist'].dtype and a['dist'].tobytes() == b['dist'].tobytes(), (name, bag)
        for k in angles:
            assert a[k].dtype == b[k].dtype and deg_close(a[k], b[k]), (name, bag, k)
        n += len(a['dist'])
    return n


def test_ring_and_amide_loops_on_random_sets():
    """All 40 random ring / amide sets of tests/test_gpu_edge_cases.py (whole and partial selections, coincident centres, zero normals,
    rings without a residue).  In the sets of the 4 A and 9 A boxes every item is within 6 A of nearly every other, hundreds of
    thousands of pairs at the ~60 us a pair costs ref_py (the whole test took 51 s): there both restatements get the first 70 rings and
    70 amides of the set only, the other sets whole."""
    from helpers import random_ring_and_amide_sets
    records = 0
    for case, pc, sel in random_ring_and_amide_sets():
        if np.ptp(pc.ring_center, axis=0).max() < 10.0 or np.ptp(pc.amide_center, axis=0).max() < 10.0:
            pc.ring_center, pc.ring_normal, pc.ring_res = pc.ring_center[:70], pc.ring_normal[:70], pc.ring_res[:70]
            pc.amide_center, pc.amide_normal, pc.amide_res = pc.amide_center[:70], pc.amide_normal[:70], pc.amide_res[:70]
            pc.amide_atoms = pc.amide_atoms[:70]
        oc = oracle.OracleComplex(pc)
        plus = oc.make_selection(sel, use_grid=False)
        records += _same_planes(RefPy(pc, sel, plus), oc, f'case{case}')
    assert records > 10_000, records


def test_ring_and_amide_loops_on_the_golden_plane_fixture(golden_dir):
    import os
    from helpers import planes_only_complex
    g = np.load(os.path.join(golden_dir, 'planes_input.npz'))
    pc = planes_only_complex(g['ring_center'], g['ring_normal'], g['ring_res'], g['amide_center'], g['amide_normal'], g['amide_res'], g['nres'])
    oc = oracle.OracleComplex(pc)
    oc.ring_sel[:] = g['ring_sel']; oc.ring_plus[:] = g['ring_plus']
    oc.amide_sel[:] = g['amide_sel']; oc.amide_plus[:] = g['amide_plus']
    rp = RefPy(pc)
    rp.ring_sel, rp.ring_plus = g['ring_sel'].astype(bool).tolist(), g['ring_plus'].astype(bool).tolist()
    rp.amide_sel, rp.amide_plus = g['amide_sel'].astype(bool).tolist(), g['amide_plus'].astype(bool).tolist()
    assert _same_planes(rp, oc, 'golden planes') > 500
