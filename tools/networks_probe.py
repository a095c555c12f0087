"""Time the interaction networks of a pass: components made on the host from the fetched atom-atom bag (A) against on the
device (B).

    python tools/networks_probe.py --reps 21 --out profiles/networks_probe.json

Both routes start from a resident structure and end with the labels and the component table in host memory; each repetition is
timed from a synchronised device.  Route A: pass + ``fetch_packed`` (sort on the device, every record over PCIe) +
``networks.components`` in NumPy.  Route B: pass + ``Context.networks`` (only the labels and the table are copied).  The two
results are compared on the first repetition.  The repetitions alternate A, B, pass alone; medians of each, and each median
minus that of the pass alone.  Whole routes by the host clock only: no kernel-level time is taken, and no time is a pass
criterion of the tests.  Cases: those of tools/persistence_probe.py (models) with the all-records masks, and
``synth.config3(100_000)`` (one structure) with the all-records masks — one giant component — and with hbond | polar — many
small ones.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, contact_filter, networks, synth  # noqa: E402

HP = contact_filter.masks(('hbond', 'polar'))[0]
ALL = contact_filter.SIFT_ALL
# name -> (structure, models (0: one structure), cutoff, sift_any)
CASES = {'F8': (lambda: synth.proteinlike(n_res=480, seed=2), 8, 5.0, ALL), 'F64': (lambda: synth.proteinlike(n_res=480, seed=2), 64, 5.0, ALL),
         'F256': (lambda: synth.proteinlike(n_res=480, seed=2), 256, 5.0, ALL),
         'hub': (lambda: synth.proteinlike(n_res=40, seed=21, n_waters=20), 256, 7.5, ALL),
         'config3_100k_all': (lambda: synth.config3(100_000), 0, 5.0, ALL),
         'config3_100k_hbond_polar': (lambda: synth.config3(100_000), 0, 5.0, HP)}


def same(a, b):
    return np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) and a[1][k].dtype == b[1][k].dtype for k in a[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = dict(reps=a.reps, runs=[])
    for name in a.cases:
        make, F, cutoff, sift_any = CASES[name]
        pc = make()
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(True)
        if F:
            xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
            ctx.set_topology(pc)
            ctx.set_models(xyz, h_xyz)
        else:
            ctx.set_complex(pc)
        nodes = pc.n_atoms * max(F, 1)

        def timed(work):
            ctx.device_synchronize()
            t = time.perf_counter()
            r = work()
            return time.perf_counter() - t, r

        def route_a():
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            bags, _ = ctx.fetch_packed()
            return networks.components(bags['atom_atom'], nodes, sift_any)

        def route_b():
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            return ctx.networks(sift_any)

        def pass_only():
            ctx.run_launch(cutoff, 0.1, False, 6.0)

        for _ in range(2):
            ra, rb = timed(route_a)[1], timed(route_b)[1]
            timed(pass_only)
        records = int(ctx.run_launch(cutoff, 0.1, False, 6.0)['atom_atom'])
        tA, tB, tO = [], [], []
        for _ in range(a.reps):      # (alternating: what shares the host shares it with all three)
            tA.append(timed(route_a)[0])
            tB.append(timed(route_b)[0])
            tO.append(timed(pass_only)[0])
        ma, mb, mo = (1e3 * float(np.median(x)) for x in (tA, tB, tO))
        label, table = rb
        run = dict(case=name, atoms=pc.n_atoms, models=F, nodes=nodes, cutoff=cutoff, sift_any=sift_any, records=records,
                   edges=int(table['n_edges'].astype(np.int64).sum()), components=len(table['root']),
                   largest_nodes=int(table['n_nodes'].max()) if len(table['root']) else 0, untouched=int((label < 0).sum()),
                   results_equal=bool(same(ra, rb)), d2h_bytes_a=15 * records,
                   d2h_bytes_b=int(label.nbytes + sum(np.asarray(v).nbytes for v in table.values())),
                   a_median_ms=ma, b_median_ms=mb, pass_only_median_ms=mo, a_minus_pass_ms=ma - mo, b_minus_pass_ms=mb - mo,
                   a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB], pass_only_ms=[1e3 * x for x in tO])
        out['runs'].append(run)
        print(json.dumps({k: v for k, v in run.items() if not k.endswith('_ms') or 'median' in k or 'minus' in k}), flush=True)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
