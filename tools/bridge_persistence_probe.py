"""Time water-bridge persistence over the resident models: the bridge table fetched and folded on the host (A) against folded
on the device (B).

    python tools/bridge_persistence_probe.py --reps 21 --out profiles/bridge_persistence.json

Both routes start from a finished pass over F resident models with NO sort enqueued (``set_sort_after_pass(False)``, a
synchronised device) and end with the fourteen columns of the persistence table in host memory.  Route A is the only route
there was before the device fold: ``Context.water_bridges`` (the join on the device, B rows over PCIe),
``water_bridges.split_models``, ``bridge_persistence.fold`` of every model and ``bridge_persistence.merge`` of the F tables,
left to right.  Route B: ``Context.models_water_bridge_persistence`` (the same join, its rows re-keyed and sorted, ONE more wait
for U, one wave per row, U rows over PCIe).  Every repetition runs a pass of its own first, outside the timed region, so neither
route finds a made table waiting.  The two tables are asserted equal on every repetition, ``dist_sum`` to the bit.  Cases: the
532-atom protein-like structure with 20 waters in 64 models, and synth.config3(20 000) in 16 models; whole structures, 5.0 A.
Masks: hbond | polar (the default of the public face) and every bit but proximal; both levels.  Whole routes are timed with the
host clock; no kernel-level times are taken here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, bridge_persistence, synth, water_bridges  # noqa: E402
from arpeggio_amd.core import config  # noqa: E402

CASES = {'proteinlike40_F64': lambda: (synth.proteinlike(n_res=40, seed=21, n_waters=20), 64),
         'config3_20k_F16': lambda: (synth.config3(20000), 16)}
MASKS = {'hbond_polar': water_bridges.mask(('hbond', 'polar')),
         'all_but_proximal': water_bridges.SIFT_ALL & ~(1 << config.SIFT_NAMES.index('proximal'))}
LEVELS = {'atom': 0, 'residue': bridge_persistence.BY_RESIDUE}


def _nbytes(t):
    return int(sum(np.asarray(v).nbytes for v in t.values()))


def same(a, b):
    return list(a) == list(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = dict(reps=a.reps, timing='host clock around whole routes; no kernel-level times', runs=[])
    for name in a.cases:
        pc, F = CASES[name]()
        xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
        n = pc.n_atoms
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(False)
        ctx.set_topology(pc)
        ctx.set_models(xyz, h_xyz)

        def finished_pass():
            ctx.run_launch(5.0, 0.1, False, 6.0)
            ctx.device_synchronize()

        def route_a(sa, level):
            finished_pass()
            t = time.perf_counter()
            bridges = ctx.water_bridges(sa)
            res = pc.res_id if level == 'residue' else None
            table = bridge_persistence.empty(level)
            for f, part in enumerate(water_bridges.split_models(bridges, n)):
                table = bridge_persistence.merge(table, bridge_persistence.fold(part, n, res), f)
            return time.perf_counter() - t, table, bridges

        def route_b(sa, level):
            finished_pass()
            t = time.perf_counter()
            table = ctx.models_water_bridge_persistence(sa, LEVELS[level])
            return time.perf_counter() - t, table

        for mname, sa in MASKS.items():
            for level in LEVELS:
                for _ in range(2):
                    route_a(sa, level)
                    route_b(sa, level)
                tA, tB = [], []
                for _ in range(a.reps):
                    da, ta, bridges = route_a(sa, level)
                    db, tb = route_b(sa, level)
                    assert same(ta, tb), (name, mname, level, 'the tables differ')
                    tA.append(da)
                    tB.append(db)
                ma, mb = (1e3 * float(np.median(x)) for x in (tA, tB))
                spread = lambda x: [1e3 * float(np.percentile(x, q)) for q in (25, 75)]
                run = dict(case=name, mask=mname, sift_any=sa, level=level, atoms_per_model=n, models=F, bridge_rows=len(bridges['water']),
                           rows=len(tb['n_models']), results_equal=True, d2h_bytes_a=_nbytes(bridges), d2h_bytes_b=_nbytes(tb),
                           a_median_ms=ma, b_median_ms=mb, a_quartiles_ms=spread(tA), b_quartiles_ms=spread(tB),
                           a_min_max_ms=[1e3 * min(tA), 1e3 * max(tA)], b_min_max_ms=[1e3 * min(tB), 1e3 * max(tB)],
                           a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB])
                out['runs'].append(run)
                print(json.dumps({k: v for k, v in run.items() if k not in ('a_ms', 'b_ms')}), flush=True)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
