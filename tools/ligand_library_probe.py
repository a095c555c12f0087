"""Time a ligand library on a resident receptor (Context.library_contacts, csrc/arp_library.h) beside the pose route run per ligand.

    python tools/ligand_library_probe.py --out profiles/ligand_library_probe.json

Case: synth.proteinlike(480, 2) (5.9 k atoms) as the receptor, a library of 1 024 synthetic 'chain' ligands of 20 - 60 atoms
(synth.ligands(seed=1)), 16 poses each (synth.library_poses_of about the receptor's centroid, shift 8 A), 5.0 A.  Every
repetition starts from a synchronised device with the receptor and the library resident and ends with its result in host memory:

    full      library_contacts: upload of the poses and their tables + launch (kernel, sort, columns) + fetch of records, offsets, summary
    summary   library_summary: the same launch, only the [T, 16] summary copied
    best      the same launch, then library_best: 20 bytes per ligand copied

and the parent's route (A) over the first ``--route-a-ligands`` ligands (default 32), per ligand: set_complex of the receptor with
the ligand appended, set_selection, poses_contacts on its 16 poses.  Its time per ligand is carried over to the whole library
(``route_a_carried_over_ms``: measured on the subset, NOT on 1 024 ligands).  The records of the two routes are compared on the
subset during the warm-up (``equal``).  Not timed apart: the upload, the kernel, the sort and the fetch inside a launch; packing
the library and set_ligand_library (once per library: ``set_library_ms``, one measurement).  Medians of ``reps`` repetitions in
one process after ``warmups`` warm-ups of each route, smallest and largest beside them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, synth  # noqa: E402
from arpeggio_amd import ligand_library as ll  # noqa: E402

PARAMS = (5.0, 0.1, False)
WEIGHTS = np.array([-8, 0, -2, 1, 0, 5, 2, 6, 6, 6, 2, 1, 2, 1, 1, 0], np.int64)


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), range_ms=[1e3 * min(ts), 1e3 * max(ts)], all_ms=[1e3 * v for v in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ligands', type=int, default=1024)
    ap.add_argument('--poses', type=int, default=16)
    ap.add_argument('--route-a-ligands', type=int, default=32)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rec = synth.proteinlike(n_res=480, seed=2)
    ligs = synth.ligands(a.ligands, seed=1, sizes=(20, 60), kinds=('chain',))
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    poses = [synth.library_poses_of(rec, lig, centre, a.poses, seed=100 + l, shift=8.0) for l, lig in enumerate(ligs)]
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, poses)
    ctx = _capi.Context(0)
    ctx.set_complex(rec)
    ctx.device_synchronize()
    t0 = time.perf_counter()
    ctx.set_ligand_library(lib)
    set_library = time.perf_counter() - t0

    def timed(fn):
        ctx.device_synchronize()
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    def best():
        ctx._library_launch(off, x, h, *PARAMS)      # (the launch alone: nothing of it is fetched)
        return ctx.library_best(WEIGHTS)
    routes = dict(full=lambda: ctx.library_contacts(off, x, h, *PARAMS), summary=lambda: ctx.library_summary(off, x, h, *PARAMS), best=best)
    last = {}
    for _ in range(a.warmups):
        for name, fn in routes.items():
            last[name] = timed(fn)[1]
    table = last['full']
    assert np.array_equal(last['summary'], table['summary'])
    assert all(np.array_equal(last['best'][k], v) for k, v in ll.best(table, WEIGHTS).items())
    times = {name: [] for name in routes}
    for _ in range(a.reps):
        for name, fn in routes.items():
            times[name].append(timed(fn)[0])
    # ---- route (A) on a subset
    sub = min(a.route_a_ligands, a.ligands)
    ref = _capi.Context(0)
    complexes = [ll.complex_of(rec, lig) for lig in ligs[:sub]]
    masks = [np.concatenate([np.zeros(rec.n_atoms, np.uint8), np.ones(lig.n_atoms, np.uint8)]) for lig in ligs[:sub]]

    def route_a():
        out = []
        for l in range(sub):
            ref.set_complex(complexes[l])
            ref.set_selection(masks[l])
            out.append(ref.poses_contacts(poses[l][0], poses[l][1], *PARAMS))
        return out

    def timed_a():
        ref.device_synchronize()
        t = time.perf_counter()
        r = route_a()
        return time.perf_counter() - t, r
    for _ in range(a.warmups):
        _, per = timed_a()
    parts = ll.split(table)
    equal = True
    for l in range(sub):
        o = per[l]['pose_off'].astype(np.int64)
        for p in range(a.poses):
            r = parts[l][p]
            equal &= np.array_equal(per[l]['i'][o[p]:o[p + 1]], r['i']) and np.array_equal(per[l]['j'][o[p]:o[p + 1]] - rec.n_atoms, r['a'])
            equal &= per[l]['dist'][o[p]:o[p + 1]].tobytes() == r['dist'].tobytes() and np.array_equal(per[l]['sift'][o[p]:o[p + 1]], r['sift'])
            equal &= np.array_equal(per[l]['ctype'][o[p]:o[p + 1]], r['ctype'])
    ta = [timed_a()[0] for _ in range(a.reps)]
    ref.close()
    k, T = len(table['i']), int(off[-1])
    out = dict(case='proteinlike(480, 2) + synth.ligands(%d, seed=1, sizes=(20, 60), chain) x %d poses' % (a.ligands, a.poses), receptor_atoms=rec.n_atoms,
               ligands=a.ligands, library_atoms=int(lib['atom_off'][-1]), library_hydrogen_rows=int(lib['h_off'][-1]), poses=T, params=list(PARAMS),
               reps=a.reps, warmups=a.warmups, records=k, records_per_pose=k / T, blocks=ctx.library_info()['blocks'],
               h2d_bytes=int(x.nbytes + h.nbytes + 4 * T + 8 * (3 * a.ligands + 1)), d2h_bytes_full=15 * k + 8 * (T + 1) + 64 * T, d2h_bytes_summary=64 * T,
               d2h_bytes_best=20 * a.ligands, set_library_ms=1e3 * set_library, full=stats(times['full']), summary=stats(times['summary']),
               best=stats(times['best']), full_per_pose_us=1e6 * float(np.median(times['full'])) / T,
               summary_per_pose_us=1e6 * float(np.median(times['summary'])) / T, best_per_pose_us=1e6 * float(np.median(times['best'])) / T,
               route_a_ligands=sub, route_a=stats(ta), route_a_per_ligand_ms=1e3 * float(np.median(ta)) / sub,
               route_a_carried_over_ms=1e3 * float(np.median(ta)) / sub * a.ligands,
               route_a_carried_over_note='measured on %d ligands, carried over to %d at the same time per ligand' % (sub, a.ligands), equal=bool(equal),
               not_timed_apart='upload, kernel, sort and fetch inside a launch; packing the library; set_ligand_library (one measurement)')
    ctx.close()
    print(json.dumps({k_: v for k_, v in out.items() if not isinstance(v, dict)}), flush=True)
    print(json.dumps({n: {q: out[n][q] for q in ('median_ms', 'range_ms')} for n in ('full', 'summary', 'best', 'route_a')}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
