"""Time the library water bridges: everything fetched and joined on the host (A) against joined on the device (B).

    python tools/library_bridges_probe.py --reps 11 --out profiles/library_bridges.json

Case (that of tools/ligand_library_probe.py): synth.proteinlike(480, 2) as the receptor, 1 024 synthetic 'chain' ligands of 20 - 60
atoms (synth.ligands(seed=1)), 16 poses each (synth.library_poses_of about the receptor's centroid, shift 8 A), 5.0 A: T = 16 384
global poses.  Both routes start from a resident library result and a finished whole-receptor pass with everything selected (both
made outside the timed region, the device synchronised) and end with the eight columns and the three per-pose arrays in host
memory.  Route A is the only route there was: the full fetch of the library's records (``arp_library_contacts_fetch``) +
``fetch_packed()`` of the receptor's bags + the NumPy join of ``library_bridges.join``.  Route B: ``Context.library_water_bridges``
(the receptor's legs counted, compacted and sorted — wait 1 —, the table by water, ligand legs and rows counted — wait 2 —, the rows
written, the table over PCIe).  Before every repetition of B the result is voided by another mask's launch, so B never finds its
table waiting.  The tables are asserted equal on every repetition.  Masks: hbond | polar (the default of the public face) and
every bit.  Median of ``--reps`` after 2 warm-ups with smallest - largest; whole routes timed with the host clock, no kernel-level
times.  No time is a pass criterion.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, library_bridges, synth, water_bridges  # noqa: E402
from arpeggio_amd import ligand_library as ll  # noqa: E402

MASKS = {'hbond_polar': water_bridges.mask(('hbond', 'polar')), 'every_bit': water_bridges.SIFT_ALL}
KEYS = tuple(k for k, _ in library_bridges.COLUMNS + library_bridges.PER_POSE)


def same(a, b):
    return all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ligands', type=int, default=1024)
    ap.add_argument('--poses', type=int, default=16)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rec = synth.proteinlike(n_res=480, seed=2)
    ligs = synth.ligands(a.ligands, seed=1, sizes=(20, 60), kinds=('chain',))
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    poses = [synth.library_poses_of(rec, lig, centre, a.poses, seed=100 + l, shift=8.0) for l, lig in enumerate(ligs)]
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, poses)
    ctx = _capi.Context(0)
    ctx.set_sort_after_pass(False)
    ctx.set_complex(rec)
    ctx.run_launch(5.0, 0.1, False, 6.0)
    ctx.set_ligand_library(lib)
    ctx.library_summary(off, x, h, 5.0, 0.1, False)
    ctx.device_synchronize()
    T, k = ctx.library_info()['poses'], ctx.library_info()['records']
    state = dict(buf=None)

    def route_a(sa):
        ctx.device_synchronize()
        t = time.perf_counter()
        table = ctx._pose_records_fetch('arp_library_contacts_fetch', 'a', T, k)
        table['ligand_pose_off'] = off
        bags, state['buf'] = ctx.fetch_packed(state['buf'])
        out = library_bridges.join(table, bags['atom_atom'], rec.flags, lib, sa)
        return time.perf_counter() - t, out, table, bags

    def route_b(sa):
        ctx.library_water_bridges(sift_any=sa ^ 1)          # (another mask: the table below is made, not found)
        ctx.device_synchronize()
        t = time.perf_counter()
        out = ctx.library_water_bridges(sift_any=sa)
        return time.perf_counter() - t, out

    out = dict(case='proteinlike(480, 2) + synth.ligands(%d, seed=1, sizes=(20, 60), chain) x %d poses' % (a.ligands, a.poses),
               receptor_atoms=rec.n_atoms, poses=T, library_records=k, reps=a.reps,
               timing='host clock around whole routes; median of reps after 2 warm-ups; no kernel-level times', runs=[])
    for mname, sa in MASKS.items():
        for _ in range(2):
            route_a(sa)
            route_b(sa)
        tA, tB = [], []
        for _ in range(a.reps):
            da, ta, table, bags = route_a(sa)
            db, tb = route_b(sa)
            assert same(ta, tb), (mname, 'the tables differ')
            tA.append(da)
            tB.append(db)
        info = ctx.library_water_bridges_info()
        d2h_a = int(sum(np.asarray(table[c]).nbytes for c in ('i', 'a', 'dist', 'sift', 'ctype', 'pose_off', 'summary')) +
                    sum(np.asarray(v).nbytes for b in bags.values() if isinstance(b, dict) for v in b.values()))
        run = dict(mask=mname, sift_any=sa, rows=info['rows'], ligand_legs=info['ligand_legs'], receptor_legs=info['receptor_legs'],
                   receptor_waters=info['receptor_waters'], results_equal=True, d2h_bytes_a=d2h_a, d2h_bytes_b=int(sum(np.asarray(tb[c]).nbytes for c in KEYS)),
                   a_median_ms=1e3 * float(np.median(tA)), b_median_ms=1e3 * float(np.median(tB)),
                   a_min_max_ms=[1e3 * min(tA), 1e3 * max(tA)], b_min_max_ms=[1e3 * min(tB), 1e3 * max(tB)],
                   a_ms=[1e3 * v for v in tA], b_ms=[1e3 * v for v in tB])
        out['runs'].append(run)
        print(json.dumps({c: v for c, v in run.items() if c not in ('a_ms', 'b_ms')}), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
