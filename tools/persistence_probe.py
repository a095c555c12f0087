"""Time the contact-persistence table of an ensemble: reduced on the host from fetched records (A) against on the device (B).

    python tools/persistence_probe.py --reps 21 --out profiles/models_persistence.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/persistence_probe.py --reps 5 --cases hub
    python tools/persistence_probe.py --kernel-stats DIR --out profiles/models_persistence.json      # adds the kernel times

Both routes start from resident models and end with the table in host memory; each repetition is timed from a synchronised
device.  Route A is what existed before the device reduction: pass + ``run_models`` (sort on the device, every record over
PCIe, ``split_models``) + a NumPy reduction (np.unique over (a, b), np.add.at / minimum.at / maximum.at; dist_sum by one
pass per model as the table's contract orders it).  Route B: pass + ``models_persistence`` (only the table is copied).  The
two tables are compared on the first repetition.  Cases: synth.proteinlike(480, 2) at F = 8, 64, 256 (5.0 A) and the hub case
synth.proteinlike(40, 21, 20) at F = 256, 7.5 A; models by synth.models_of(seed=4, jitter=0.3).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, synth  # noqa: E402

CASES = {'F8': (lambda: synth.proteinlike(n_res=480, seed=2), 8, 5.0), 'F64': (lambda: synth.proteinlike(n_res=480, seed=2), 64, 5.0),
         'F256': (lambda: synth.proteinlike(n_res=480, seed=2), 256, 5.0),
         'hub': (lambda: synth.proteinlike(n_res=40, seed=21, n_waters=20), 256, 7.5)}


def host_table(per_model, n):
    """The table from per-model atom-atom bags, vectorised where the contract allows it (everything but dist_sum)."""
    F = len(per_model)
    key = np.concatenate([b['i'].astype(np.int64) * n + b['j'] for b in per_model])
    f = np.repeat(np.arange(F, dtype=np.int32), [len(b['i']) for b in per_model])
    dist = np.concatenate([b['dist'] for b in per_model])
    sift = np.concatenate([b['sift'] for b in per_model])
    ct = np.concatenate([b['ctype'] for b in per_model])
    uk, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(uk)
    first, last = np.full(U, F, np.int32), np.full(U, -1, np.int32)
    np.minimum.at(first, inv, f)
    np.maximum.at(last, inv, f)
    dmin, dmax = np.full(U, np.inf, np.float32), np.full(U, -np.inf, np.float32)
    np.minimum.at(dmin, inv, dist)
    np.maximum.at(dmax, inv, dist)
    bits = np.stack([np.bincount(inv, weights=(sift >> k) & 1, minlength=U) for k in range(15)], axis=1).astype(np.uint16)
    cm = np.zeros(U, np.uint8)
    np.bitwise_or.at(cm, inv, (1 << ct.astype(np.int64)).astype(np.uint8))
    acc = np.zeros(U, np.float64)
    lo = 0
    for b in per_model:      # ascending model order; a model touches a row at most once
        hi = lo + len(b['i'])
        acc[inv[lo:hi]] += b['dist'].astype(np.float64)
        lo = hi
    return dict(a=(uk // n).astype(np.int32), b=(uk % n).astype(np.int32), n_models=np.bincount(inv, minlength=U).astype(np.uint16),
                first=first, last=last, dist_min=dmin, dist_max=dmax, dist_sum=acc, bit_count=bits, ctype_mask=cm)


def same(a, b):
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)


def kernel_stats(path):
    """Per-kernel totals of a rocprofv3 --kernel-trace --stats run (the *kernel_stats.csv under ``path``): the reduction's own
    kernels and the radix passes it launches."""
    out = {}
    for p in glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True):
        for row in csv.DictReader(open(p)):
            name = row.get('Name', '')
            if 'k_persist' in name or 'k_runs_' in name or 'k_sort_' in name:
                short = name.split('(')[0].split(' ')[-1]
                out[short] = dict(calls=int(row['Calls']), total_us=float(row['TotalDurationNs']) / 1e3, average_us=float(row['AverageNs']) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-stats', default=None, help='directory of a rocprofv3 --kernel-trace --stats run of this tool: merged into --out')
    a = ap.parse_args()
    if a.kernel_stats:
        doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        doc['kernel_stats'] = kernel_stats(a.kernel_stats)
        print(json.dumps(doc['kernel_stats']))
        if a.out:
            json.dump(doc, open(a.out, 'w'), indent=1)
        return
    out = dict(reps=a.reps, runs=[])
    for name in a.cases:
        make, F, cutoff = CASES[name]
        pc = make()
        n = pc.n_atoms
        xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(True)
        ctx.set_topology(pc)
        ctx.set_models(xyz, h_xyz)

        def route_a():
            ctx.device_synchronize()
            t = time.perf_counter()
            per = ctx.run_models(cutoff, 0.1, False, 6.0)
            tab = host_table([m['atom_atom'] for m in per], n)
            return time.perf_counter() - t, tab

        def route_b():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            tab = ctx.models_persistence()
            return time.perf_counter() - t, tab

        def pass_only():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            return time.perf_counter() - t

        for _ in range(2):
            _, ta = route_a()
            _, tb = route_b()
            pass_only()
        records = int(ta['n_models'].astype(np.int64).sum())
        rows = len(ta['a'])
        tA, tB, tP = [], [], []
        for _ in range(a.reps):
            tA.append(route_a()[0])
            tB.append(route_b()[0])
            tP.append(pass_only())
        ma, mb, mp = (1e3 * float(np.median(x)) for x in (tA, tB, tP))
        run = dict(case=name, atoms=n, models=F, cutoff=cutoff, records=records, rows=rows, tables_equal=bool(same(ta, tb)),
                   d2h_bytes_a=15 * records, d2h_bytes_b=int(sum(np.asarray(v).nbytes for v in tb.values())),
                   a_median_ms=ma, b_median_ms=mb, pass_only_median_ms=mp, a_minus_pass_ms=ma - mp, b_minus_pass_ms=mb - mp,
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
