"""Time the contact-lifetimes table of an ensemble: reduced on the host from fetched records (A) against on the device (B),
beside the persistence table made by the same library in the same session.

    python tools/lifetimes_probe.py --reps 21 --out profiles/lifetimes_probe.json

Both routes start from resident models and end with the table in host memory; each repetition is timed from a synchronised
device.  Route A: pass + ``run_models`` (sort on the device, every record over PCIe, ``split_models``) + a NumPy reduction
(one lexsort by (pair, model), interval heads by a difference, np.add.reduceat / np.maximum.reduceat over the intervals of a
pair).  Route B: pass + ``models_lifetimes`` (only the table is copied).  The two tables are compared on the first repetition.
The yardstick of route B is the persistence table on the same case — same sort, same record count, a heavier reduce —, timed
TWICE per repetition (``persist_minus_pass_ms``, ``persist_again_minus_pass_ms``): what two runs of the same thing differ by
in this session is the spread against which ``b_minus_pass_ms`` is read.  Cases: those of tools/persistence_probe.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, synth, tables  # noqa: E402

CASES = {'F8': (lambda: synth.proteinlike(n_res=480, seed=2), 8, 5.0), 'F64': (lambda: synth.proteinlike(n_res=480, seed=2), 64, 5.0),
         'F256': (lambda: synth.proteinlike(n_res=480, seed=2), 256, 5.0),
         'hub': (lambda: synth.proteinlike(n_res=40, seed=21, n_waters=20), 256, 7.5)}


def host_table(per_model, n, gap):
    """The table from per-model atom-atom bags (every record takes part), vectorised."""
    F = len(per_model)
    key = np.concatenate([b['i'].astype(np.int64) * n + b['j'] for b in per_model])
    f = np.repeat(np.arange(F, dtype=np.int64), [len(b['i']) for b in per_model])
    o = np.lexsort((f, key))
    key, f = key[o], f[o]
    k = len(key)
    if k == 0:
        return tables.empty(tables.LIFETIMES)
    new_row = np.ones(k, bool)
    new_row[1:] = key[1:] != key[:-1]
    head = new_row.copy()
    head[1:] |= (f[1:] - f[:-1]) > gap + 1
    rs = np.nonzero(new_row)[0]                      # first record of every row
    hs = np.nonzero(head)[0]                         # first record of every interval
    ends = np.append(hs[1:], k) - 1                  # its last record
    span = f[ends] - f[hs] + 1
    first_iv = np.searchsorted(hs, rs)               # first interval of every row
    last_iv = np.append(first_iv[1:], len(hs)) - 1
    longest = np.maximum.reduceat(span, first_iv)
    row_of_iv = np.repeat(np.arange(len(rs)), np.diff(np.append(first_iv, len(hs))))
    is_best = span == longest[row_of_iv]
    best_iv = np.minimum.reduceat(np.where(is_best, np.arange(len(hs)), len(hs)), first_iv)      # the earliest on a tie
    cols = dict(a=key[rs] // n, b=key[rs] % n, n_models=np.diff(np.append(rs, k)), first=f[rs], last=f[np.append(rs[1:], k) - 1],
                n_intervals=last_iv - first_iv + 1, longest=longest, longest_start=f[hs][best_iv], head=span[first_iv],
                tail=span[last_iv], span_sum=np.add.reduceat(span, first_iv))
    return {name: cols[name].astype(dt) for name, dt in tables.LIFETIMES.columns}


def same(a, b):
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--gap', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = dict(reps=a.reps, gap=a.gap, runs=[])
    for name in a.cases:
        make, F, cutoff = CASES[name]
        pc = make()
        n = pc.n_atoms
        xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(True)
        ctx.set_topology(pc)
        ctx.set_models(xyz, h_xyz)

        def timed(work):
            ctx.device_synchronize()
            t = time.perf_counter()
            r = work()
            return time.perf_counter() - t, r

        def route_a():
            return host_table([m['atom_atom'] for m in ctx.run_models(cutoff, 0.1, False, 6.0)], n, a.gap)

        def route_b():
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            return ctx.models_lifetimes(a.gap)

        def persist():
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            return ctx.models_persistence()

        def pass_only():
            ctx.run_launch(cutoff, 0.1, False, 6.0)

        for _ in range(2):
            ta, tb, tp = timed(route_a)[1], timed(route_b)[1], timed(persist)[1]
            timed(pass_only)
        records = int(ta['n_models'].astype(np.int64).sum())
        tA, tB, tP1, tP2, tO = [], [], [], [], []
        for _ in range(a.reps):      # (alternating: what shares the host shares it with all five)
            tA.append(timed(route_a)[0])
            tP1.append(timed(persist)[0])
            tB.append(timed(route_b)[0])
            tP2.append(timed(persist)[0])
            tO.append(timed(pass_only)[0])
        ma, mb, mp1, mp2, mo = (1e3 * float(np.median(x)) for x in (tA, tB, tP1, tP2, tO))
        run = dict(case=name, atoms=n, models=F, cutoff=cutoff, gap=a.gap, records=records, rows=len(ta['a']),
                   intervals=int(ta['n_intervals'].astype(np.int64).sum()), tables_equal=bool(same(ta, tb)),
                   d2h_bytes_a=15 * records, d2h_bytes_b=int(sum(np.asarray(v).nbytes for v in tb.values())),
                   d2h_bytes_persistence=int(sum(np.asarray(v).nbytes for v in tp.values())),
                   a_median_ms=ma, b_median_ms=mb, pass_only_median_ms=mo, a_minus_pass_ms=ma - mo, b_minus_pass_ms=mb - mo,
                   persist_minus_pass_ms=mp1 - mo, persist_again_minus_pass_ms=mp2 - mo,
                   a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB], persist_ms=[1e3 * x for x in tP1],
                   persist_again_ms=[1e3 * x for x in tP2], pass_only_ms=[1e3 * x for x in tO])
        out['runs'].append(run)
        print(json.dumps({k: v for k, v in run.items() if not k.endswith('_ms') or 'median' in k or 'minus' in k}), flush=True)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
