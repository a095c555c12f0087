"""Batches built to sit on the seams of the batch grid's placement (csrc/arp_batchgrid.h), shared by the CPU tests of the
layout and the GPU tests that run them (tests/test_batch_layout.py).  Every builder returns ``(pcs, boxes)``: the members and
the float64 [B, 6] boxes the batch is declared with — ``batch.concat_complexes``' own, except where a case says otherwise."""
import numpy as np

from arpeggio_amd import batch, synth
from helpers import planes_only_complex, tiny_complex

EDGE = lambda r: r * (1.0 + 1e-6)      # noqa: E731  the cell edge a radius asks for, before any growth


def own_boxes(pcs):
    return batch.concat_complexes(pcs)[1]['boxes'].copy()


def adversarial_members():
    """About 40 small members, under 5 k atoms: the shapes a placement or a binning can get wrong.  Returns (pcs, boxes, tags):
    tags[name] = member index (or indices) of the special ones."""
    pcs, tags = [], {}

    def add(name, pc):
        tags.setdefault(name, []).append(len(pcs))
        pcs.append(pc)

    add('one_atom', tiny_complex([[3.0, -2.0, 7.0]]))
    rng = np.random.default_rng(31)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)      # noqa: E731
    add('planes_only', planes_only_complex(rng.random((9, 3)) * 14.0, unit(rng.standard_normal((9, 3))), rng.integers(0, 6, 9).astype(np.int32),
                                           (rng.random((7, 3)) * 14.0).astype(np.float32), unit(rng.standard_normal((7, 3))).astype(np.float32),
                                           rng.integers(0, 6, 7).astype(np.int32), 6))
    a = 4.99 / np.sqrt(3.0)
    add('corners', tiny_complex([[0.0, 0.0, 0.0], [a, a, a]]))                       # both atoms are corners of their box
    add('flat', synth.make_synthetic(70, seed=32, box=(28, 28, 0.8), n_rings=2, n_amides=2))
    add('needle', synth.make_synthetic(60, seed=33, box=(90, 0.9, 0.9), origin=(-40, 5, 5)))
    add('multiple', synth.make_synthetic(90, seed=34, box=(14.9, 14.9, 5.9), n_rings=2, n_amides=2))
    twin = synth.make_synthetic(110, seed=35, box=(16, 16, 16), n_rings=3, n_amides=3)
    for _ in range(3):
        add('identical', twin)                                                          # the same world coordinates, three times
    add('box_larger', synth.make_synthetic(100, seed=36, box=(15, 15, 15), origin=(-5, -5, -5), n_rings=2, n_amides=2))
    add('box_smaller', synth.make_synthetic(160, seed=37, box=(24, 24, 24), n_rings=3, n_amides=3))
    shapes = [(12, 12, 12), (30, 10, 10), (10, 26, 10), (10, 10, 33), (20, 20, 6), (6, 22, 22), (17, 17, 17), (9, 9, 9)]
    for k in range(29):
        bx = shapes[k % len(shapes)]
        n = int(0.045 * bx[0] * bx[1] * bx[2])
        add('filler', synth.make_synthetic(n, seed=100 + k, box=bx, origin=(3.0 * (k % 4), -2.0 * (k % 3), 1.5 * (k % 5)),
                                           n_rings=k % 3, n_amides=(k + 1) % 3))
    boxes = own_boxes(pcs)
    # an extent that is an exact multiple of the cell edge, on a different axis for each radius a pass asks for
    m = tags['multiple'][0]
    boxes[m, :3] = 0.0                                                                   # (hi - lo is then the multiple itself)
    boxes[m, 3:] = np.array([3 * EDGE(5.0), 2 * EDGE(7.5), 1 * EDGE(6.0)])
    lg = tags['box_larger'][0]
    boxes[lg, :3] -= 7.0
    boxes[lg, 3:] += 11.0
    sm = tags['box_smaller'][0]                                                          # the middle third: most atoms lie outside
    lo, hi = boxes[sm, :3].copy(), boxes[sm, 3:].copy()
    boxes[sm, :3], boxes[sm, 3:] = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
    return pcs, boxes, tags


def far_clusters_member(gap=25_000.0, n=40, seed=5):
    """One member of two clusters ``gap`` apart along x: floor(gap / 5.000005) + 1 >= 4096 cells at a 5 A cutoff."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, 3)) * 8.0
    b = rng.random((n, 3)) * 8.0 + [gap, 0.0, 0.0]
    return tiny_complex(np.concatenate([a, b]).astype(np.float32), res_id=np.arange(2 * n) // 4)


def axis_limit_batch():
    pcs = [synth.make_synthetic(150, seed=41, box=(16, 16, 16), n_rings=3, n_amides=3), far_clusters_member(),
           synth.make_synthetic(120, seed=42, box=(20, 12, 12), n_rings=2, n_amides=2)]
    return pcs, own_boxes(pcs)


def needle_member(axis, length=15_000.0, n=24, seed=6):
    """Atoms in three clumps — both ends and the middle — of a needle ``length`` long and 2 A thick along ``axis``."""
    rng = np.random.default_rng(seed + axis)
    x = rng.random((3 * n, 3)) * 2.0
    x[:, axis] = np.concatenate([rng.random(n) * 6.0, length / 2 + rng.random(n) * 6.0, length - rng.random(n) * 6.0])
    x[0, axis], x[-1, axis] = 0.0, length
    return tiny_complex(x.astype(np.float32), res_id=np.arange(3 * n) // 3)


def three_needles_batch():
    """x, y and z needles of 3000 cells at 5 A: each is far below 4096 cells, their common grid would be ~3000^3."""
    pcs = [needle_member(0), needle_member(1), needle_member(2)]
    return pcs, own_boxes(pcs)


def eviction_batch():
    pcs = [synth.proteinlike(n_res=40, seed=21, n_waters=40, id='e0'), synth.proteinlike(n_res=30, seed=22, n_waters=30, id='e1'),
           synth.proteinlike(n_res=50, seed=23, n_waters=30, id='e2')]
    return pcs, own_boxes(pcs)


QUERY_SHIFTS = ([0.0, 0.0, 0.0], [4.0, 3.0, -2.0], [300.0, -40.0, 25.0])


def overlapping_members():
    """Two members whose boxes overlap in world coordinates and one 300 A away; all of one topology (the models of
    test 3d are the same three coordinate sets).  Returns (pc, xyz [3, n, 3], h_xyz [3, nh, 3], the three members)."""
    import dataclasses
    pc = synth.proteinlike(n_res=40, seed=24, n_waters=30, id='q')
    xyz, h_xyz, pcs = [], [], []
    for shift in QUERY_SHIFTS:
        xyz.append((pc.xyz.astype(np.float64) + shift).astype(np.float32))
        h_xyz.append(pc.h_xyz + shift)
        pcs.append(dataclasses.replace(pc, xyz=xyz[-1], h_xyz=h_xyz[-1], ring_center=pc.ring_center + shift,
                                       amide_center=(pc.amide_center.astype(np.float64) + shift).astype(np.float32)))
    return pc, np.stack(xyz), np.stack(h_xyz), pcs


# ---- directed layouts (boxes only) --------------------------------------------------------------------------------------
def cube_boxes(B, cells, r, origin=0.0):
    """B cubes of ``cells`` cells a side at radius r (extent half a cell short of the next count)."""
    ext = (cells - 0.5) * EDGE(r)
    lo = np.full((B, 3), origin) + np.arange(B)[:, None] * 0.25
    return np.concatenate([lo, lo + ext], axis=1)


def needle_boxes(length=15_000.0):
    z = np.zeros((3, 6))
    for a in range(3):
        z[a, 3:] = 2.0
        z[a, 3 + a] = length
    return z
