"""Time the fetch of the atom-atom records a caller asks for: everything fetched and masked on the host (A) against filtered on
the device (B).

    python tools/filtered_fetch_probe.py --reps 21 --out profiles/filtered_fetch.json

Both routes start from a finished pass with NO sort enqueued (``set_sort_after_pass(False)``, a synchronised device) and end
with the kept records' five columns and the four ring / amide bags in host memory.  Route A is the only route there was before
the device filter: ``fetch_packed()`` (the canonical sort of all k records on the device, all k over PCIe) + the NumPy mask of
``contact_filter.apply``.  Route B: ``fetch_packed_filtered`` (count, scan, ONE wait for k', write, the sort of k' records, k'
over PCIe).  Every repetition runs a pass of its own first, outside the timed region, so neither route finds a sorted or
filtered result waiting.  The results are asserted equal on every repetition.  Cases: synth.proteinlike() (5.9 k atoms),
synth.config3(100 000), and the batch of 64 protein-sized structures bench.py --batch 64 times; whole structures, 5.0 A.
Filters: ``contact_filter.SPECIFIC`` (every bit but proximal) and the feature bits only (0x7FE0).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, batch, contact_filter, synth  # noqa: E402


def _batch64():
    distinct = [synth.proteinlike(seed=2 + k, id=f'standin{k}') for k in range(8)]
    return batch.concat_complexes([distinct[k % 8] for k in range(64)])


CASES = {'proteinlike': lambda: (synth.proteinlike(), None), 'config3_100k': lambda: (synth.config3(100_000), None), 'batch64': _batch64}
FILTERS = {'specific': contact_filter.SPECIFIC, 'feature_bits': (0x7FE0, 0x7F)}
AA = ('i', 'j', 'dist', 'sift', 'ctype')


def _nbytes(bags):
    return int(sum(np.asarray(v).nbytes for b in bags.values() if isinstance(b, dict) for v in b.values()))


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = dict(reps=a.reps, runs=[])
    for name in a.cases:
        pc, off = CASES[name]()
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(False)
        ctx.set_blob(_capi.pack_blob(pc))
        if off is not None:
            ctx.declare_batch(off)
        state = dict(buf_a=None, buf_b=None)

        def finished_pass():
            ctx.run_launch(5.0, 0.1, False, 6.0)
            ctx.device_synchronize()

        def route_a(sa, cm):
            finished_pass()
            t = time.perf_counter()
            bags, state['buf_a'] = ctx.fetch_packed(state['buf_a'])
            kept = contact_filter.apply(bags['atom_atom'], sa, cm)
            return time.perf_counter() - t, kept, bags

        def route_b(sa, cm):
            finished_pass()
            t = time.perf_counter()
            bags, state['buf_b'] = ctx.fetch_packed_filtered(sa, cm, state['buf_b'])
            return time.perf_counter() - t, bags['atom_atom'], bags

        for fname, (sa, cm) in FILTERS.items():
            for _ in range(2):
                route_a(sa, cm)
                route_b(sa, cm)
            tA, tB = [], []
            for _ in range(a.reps):
                da, ka, ba = route_a(sa, cm)
                db, kb, bb = route_b(sa, cm)
                assert same(ka, {k: kb[k] for k in AA}), (name, fname, 'the kept records differ')
                assert all(same(ba[p], bb[p]) for p in ('plane_plane', 'atom_plane', 'group_group', 'group_plane')), (name, fname, 'ring / amide bags')
                tA.append(da)
                tB.append(db)
            ma, mb = (1e3 * float(np.median(x)) for x in (tA, tB))
            spread = lambda x: [1e3 * float(np.percentile(x, q)) for q in (25, 75)]
            run = dict(case=name, filter=fname, sift_any=sa, ctype_mask=cm, atoms=pc.n_atoms, records=int(bb['atom_atom_total']), kept=len(kb['j']),
                       results_equal=True, d2h_bytes_a=_nbytes(ba), d2h_bytes_b=_nbytes(bb), a_median_ms=ma, b_median_ms=mb,
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
