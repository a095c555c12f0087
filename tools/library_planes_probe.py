"""Time the ring and amide contacts of a ligand library (Context.library_planes, csrc/arp_library_planes.h) beside the pose route
run per ligand.

    python tools/library_planes_probe.py --out profiles/library_planes_probe.json

Case (the protocol of tools/ligand_library_probe.py): synth.proteinlike(480, 2) (5.9 k atoms) as the receptor, a library of 1 024
ligands that mixes the ring-bearing kinds ('arylamide', 'biaryl', 'halo' with its ring; synth.ligands(seed=1, planes=True)), 16
poses each (synth.library_poses_of about the receptor's centroid, shift 8 A).  Every repetition starts from a synchronised device
with the receptor, the library and its plane table resident and ends with its result in host memory:

    full      library_planes: upload of the poses and their tables + launch (kernel, offsets, sort, columns) + fetch of the four tables,
              their offsets and the summary
    summary   library_planes_summary: the same launch, only the [T, 16] summary copied

and route (A) over the first ``--route-a-ligands`` ligands (default 32), per ligand: set_complex of the receptor with the ligand
appended (its home 1 000 A away along x), set_selection, set_plane_atoms, poses_planes on its 16 poses.  Its time per ligand is
carried over to the whole library (``route_a_carried_over_ms``: measured on the subset, NOT on 1 024 ligands).  The records of the
two routes are compared on the subset during the warm-up (``equal``).  Not timed apart: the upload, the kernel, the sort and the
fetch inside a launch; packing the library, set_ligand_library and set_ligand_library_planes (once per library:
``set_planes_ms``, one measurement).  Medians of ``reps`` repetitions in one process after ``warmups`` warm-ups of each route,
smallest and largest beside them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, poses as _poses, synth  # noqa: E402
from arpeggio_amd import ligand_library as ll  # noqa: E402

KINDS = ('arylamide', 'biaryl', 'halo')


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), range_ms=[1e3 * min(ts), 1e3 * max(ts)], all_ms=[1e3 * v for v in ts])


def table_bytes(table, T):
    """Bytes the four tables, their offsets and the summary hold."""
    b = 64 * T
    for name in _poses.PLANE_TABLES:
        b += 8 * (T + 1) + sum(np.dtype(dt).itemsize for _, dt in _poses.plane_columns(name)) * len(table[name]['ctype'])
    return int(b)


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
    ligs = synth.ligands(a.ligands, seed=1, kinds=KINDS, planes=True)
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    ps = [synth.library_poses_of(rec, lig, centre, a.poses, seed=100 + l, shift=8.0) for l, lig in enumerate(ligs)]
    lib = ll.pack(ligs)
    off, x, _ = ll.flatten_poses(lib, ps)
    ctx = _capi.Context(0)
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    ctx.device_synchronize()
    t0 = time.perf_counter()
    ctx.set_ligand_library_planes(lib)
    set_planes = time.perf_counter() - t0

    def timed(c, fn):
        c.device_synchronize()
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r
    routes = dict(full=lambda: ctx.library_planes(off, x), summary=lambda: ctx.library_planes_summary(off, x))
    last = {}
    for _ in range(a.warmups):
        for name, fn in routes.items():
            last[name] = timed(ctx, fn)[1]
    table = last['full']
    assert np.array_equal(last['summary'], table['summary'])
    times = {name: [] for name in routes}
    for _ in range(a.reps):
        for name, fn in routes.items():
            times[name].append(timed(ctx, fn)[0])
    info = ctx.library_planes_info()
    # ---- route (A) on a subset
    sub = min(a.route_a_ligands, a.ligands)
    ref = _capi.Context(0)
    away = np.array([1000.0, 0.0, 0.0])
    complexes = [ll.complex_of(rec, lig, lig.xyz + away.astype(np.float32), lig.h_xyz + away) for lig in ligs[:sub]]
    masks = [np.concatenate([np.zeros(rec.n_atoms, np.uint8), np.ones(lig.n_atoms, np.uint8)]) for lig in ligs[:sub]]

    def route_a():
        out = []
        for l in range(sub):
            ref.set_complex(complexes[l])
            ref.set_selection(masks[l])
            ref.set_plane_atoms(complexes[l])
            out.append(ref.poses_planes(ps[l][0]))
        return out
    for _ in range(a.warmups):
        _, per = timed(ref, route_a)
    parts = ll.split_planes(table)
    equal = True
    for l in range(sub):
        for p, bags in enumerate(_poses.split_planes(per[l])):
            for name in _poses.PLANE_TABLES:
                equal &= all(bags[name][c].tobytes() == parts[l][p][name][c].tobytes() for c, _ in _poses.plane_columns(name))
    ta = [timed(ref, route_a)[0] for _ in range(a.reps)]
    ref.close()
    T = int(off[-1])
    records = {name: len(table[name]['ctype']) for name in _poses.PLANE_TABLES}
    out = dict(case='proteinlike(480, 2) + synth.ligands(%d, seed=1, kinds=%s, planes=True) x %d poses' % (a.ligands, '/'.join(KINDS), a.poses),
               receptor_atoms=rec.n_atoms, receptor_rings=rec.n_rings, receptor_amides=rec.n_amides, ligands=a.ligands, library_atoms=int(lib['atom_off'][-1]),
               library_rings=int(lib['ring_off'][-1]), library_amides=int(lib['amide_off'][-1]), poses=T, reps=a.reps, warmups=a.warmups, records=records,
               records_per_pose=sum(records.values()) / T, blocks=info['blocks'], kernel_launches_per_call=1,
               h2d_bytes=int(x.nbytes + 4 * T + 8 * (2 * a.ligands + 1)), d2h_bytes_full=table_bytes(table, T), d2h_bytes_summary=64 * T,
               set_planes_ms=1e3 * set_planes, full=stats(times['full']), summary=stats(times['summary']),
               full_per_pose_us=1e6 * float(np.median(times['full'])) / T, summary_per_pose_us=1e6 * float(np.median(times['summary'])) / T,
               route_a_ligands=sub, route_a=stats(ta), route_a_per_ligand_ms=1e3 * float(np.median(ta)) / sub,
               route_a_per_pose_us=1e6 * float(np.median(ta)) / (sub * a.poses), route_a_carried_over_ms=1e3 * float(np.median(ta)) / sub * a.ligands,
               route_a_carried_over_note='measured on %d ligands, carried over to %d at the same time per ligand: NOT measured' % (sub, a.ligands),
               equal=bool(equal),
               not_timed_apart='upload, kernel, sort and fetch inside a launch; packing the library; set_ligand_library / set_ligand_library_planes (one measurement)')
    ctx.close()
    print(json.dumps({k_: v for k_, v in out.items() if not isinstance(v, dict)}), flush=True)
    print(json.dumps(dict(records=records, **{n: {q: out[n][q] for q in ('median_ms', 'range_ms')} for n in ('full', 'summary', 'route_a')})), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
