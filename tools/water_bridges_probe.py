"""Time the water-mediated contacts of a pass: everything fetched and joined on the host (A) against joined on the device (B).

    python tools/water_bridges_probe.py --reps 21 --out profiles/water_bridges.json

Both routes start from a finished pass with NO sort enqueued (``set_sort_after_pass(False)``, a synchronised device) and end
with the nine columns of the bridge table in host memory.  Route A is the only route there was before the device join:
``fetch_packed()`` (the canonical sort of all k records on the device, all k over PCIe) + the NumPy join of
``water_bridges.join``.  Route B: ``Context.water_bridges`` (legs counted and compacted, ONE wait for L, their sort, the runs,
the pairs counted, a SECOND wait for B, the rows written, B rows over PCIe).  Every repetition runs a pass of its own first,
outside the timed region, so neither route finds a sorted bag or a made table waiting.  The results are asserted equal on every
repetition.  Cases: synth.proteinlike() (5.9 k atoms), synth.config3(100 000), and the batch of 64 protein-sized structures
bench.py --batch 64 times; whole structures, 5.0 A.  Masks: hbond | polar (the default of the public face) and every bit but
proximal.  Whole routes are timed with the host clock; no kernel-level times are taken here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, batch, synth, water_bridges  # noqa: E402
from arpeggio_amd.core import config  # noqa: E402


def _batch64():
    distinct = [synth.proteinlike(seed=2 + k, id=f'standin{k}') for k in range(8)]
    return batch.concat_complexes([distinct[k % 8] for k in range(64)])


CASES = {'proteinlike': lambda: (synth.proteinlike(), None), 'config3_100k': lambda: (synth.config3(100_000), None), 'batch64': _batch64}
MASKS = {'hbond_polar': water_bridges.mask(('hbond', 'polar')),
         'all_but_proximal': water_bridges.SIFT_ALL & ~(1 << config.SIFT_NAMES.index('proximal'))}


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
        pc, off = CASES[name]()
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(False)
        ctx.set_blob(_capi.pack_blob(pc))
        if off is not None:
            ctx.declare_batch(off)
        state = dict(buf=None)

        def finished_pass():
            ctx.run_launch(5.0, 0.1, False, 6.0)
            ctx.device_synchronize()

        def route_a(sa):
            finished_pass()
            t = time.perf_counter()
            bags, state['buf'] = ctx.fetch_packed(state['buf'])
            table = water_bridges.join(bags['atom_atom'], pc.flags, pc.res_id, sa)
            return time.perf_counter() - t, table, bags

        def route_b(sa):
            finished_pass()
            t = time.perf_counter()
            table = ctx.water_bridges(sa)
            return time.perf_counter() - t, table

        for mname, sa in MASKS.items():
            for _ in range(2):
                route_a(sa)
                route_b(sa)
            tA, tB = [], []
            for _ in range(a.reps):
                da, ta, bags = route_a(sa)
                db, tb = route_b(sa)
                assert same(ta, tb), (name, mname, 'the tables differ')
                tA.append(da)
                tB.append(db)
            ma, mb = (1e3 * float(np.median(x)) for x in (tA, tB))
            spread = lambda x: [1e3 * float(np.percentile(x, q)) for q in (25, 75)]
            d2h_a = int(sum(np.asarray(v).nbytes for b in bags.values() if isinstance(b, dict) for v in b.values()))
            run = dict(case=name, mask=mname, sift_any=sa, atoms=pc.n_atoms, records=len(bags['atom_atom']['j']), bridges=len(tb['water']),
                       results_equal=True, d2h_bytes_a=d2h_a, d2h_bytes_b=_nbytes(tb), a_median_ms=ma, b_median_ms=mb,
                       a_quartiles_ms=spread(tA), b_quartiles_ms=spread(tB), a_min_max_ms=[1e3 * min(tA), 1e3 * max(tA)],
                       b_min_max_ms=[1e3 * min(tB), 1e3 * max(tB)], a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB])
            out['runs'].append(run)
            print(json.dumps({k: v for k, v in run.items() if k not in ('a_ms', 'b_ms')}), flush=True)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
