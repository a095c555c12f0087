"""Time the residue contact-persistence table of an ensemble: folded on the host from the per-model residue tables (A) against
on the device (B).

    python tools/residue_persistence_probe.py --reps 21 --out profiles/residue_persistence.json

Both routes start from resident models and end with the table in host memory; each repetition is timed from a synchronised
device.  Route A is what existed before the device reduction: pass + ``residue_pairs`` (the per-model residue table of all F
models over PCIe, 93 B a row and model) + ``residue_pairs.split`` + a NumPy fold over the models.  Route B: pass +
``models_residue_persistence`` (only the table is copied; its size does not depend on F).  The two tables are compared on the
first repetition.  Cases: synth.proteinlike(480, 2) with F = 8, 64 and 256 models at 5.0 A, and the hub of the tests —
synth.proteinlike(40, 21, 20 waters) with F = 256 at 7.5 A; whole structures, jitter 0.3 A.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, residue_pairs, residue_persistence, synth  # noqa: E402

CASES = {'proteinlike480_F8': (lambda: synth.proteinlike(n_res=480, seed=2), 8, 5.0),
         'proteinlike480_F64': (lambda: synth.proteinlike(n_res=480, seed=2), 64, 5.0),
         'proteinlike480_F256': (lambda: synth.proteinlike(n_res=480, seed=2), 256, 5.0),
         'hub40_F256': (lambda: synth.proteinlike(n_res=40, seed=21, n_waters=20), 256, 7.5)}


def host_table(parts, nres):
    """The table from the F per-model residue tables (``residue_pairs.split``), vectorised: the models' rows one after the
    other are in ascending model order, and np.add.at adds in element order — the order dist_sum is defined in."""
    f = np.concatenate([np.full(len(t['res_a']), k, np.int32) for k, t in enumerate(parts)]) if parts else np.zeros(0, np.int32)
    cat = {k: np.concatenate([t[k] for t in parts]) for k, _ in residue_pairs.COLUMNS} if parts else residue_pairs.empty()
    uk, inv = np.unique(cat['res_a'].astype(np.int64) * nres + cat['res_b'], return_inverse=True)
    inv = inv.reshape(-1)
    U = len(uk)
    first, last = np.full(U, np.iinfo(np.int32).max, np.int32), np.full(U, -1, np.int32)
    np.minimum.at(first, inv, f)
    np.maximum.at(last, inv, f)
    has = cat['n_contacts'] > 0
    cls = np.zeros((U, 5), np.int64)
    np.add.at(cls[:, 0], inv, has)
    np.add.at(cls[:, 1:], inv, cat['plane_count'] > 0)
    bits = np.zeros((U, 15), np.int64)
    np.add.at(bits, inv, cat['bit_count'] > 0)
    n = np.zeros(U, np.int64)
    np.add.at(n, inv, cat['n_contacts'])
    dmin, dmax = np.full(U, np.inf, np.float32), np.full(U, -np.inf, np.float32)
    np.minimum.at(dmin, inv[has], cat['dist_min'][has])
    np.maximum.at(dmax, inv[has], cat['dist_min'][has])
    dsum = np.zeros(U, np.float64)
    np.add.at(dsum, inv[has], cat['dist_min'][has].astype(np.float64))
    cm = np.zeros(U, np.uint8)
    np.bitwise_or.at(cm, inv, cat['ctype_mask'])
    return dict(res_a=(uk // nres).astype(np.int32), res_b=(uk % nres).astype(np.int32), n_models=np.bincount(inv, minlength=U).astype(np.uint16),
                first=first, last=last, n_contacts=n.astype(np.uint32), class_models=cls.astype(np.uint16), bit_models=bits.astype(np.uint16),
                dist_min=dmin, dist_max=dmax, dist_sum=dsum, ctype_mask=cm)


def same(a, b):
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and
               np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k, _ in residue_persistence.COLUMNS)


def nbytes(t):
    return int(sum(np.asarray(v).nbytes for v in t.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = dict(reps=a.reps, runs=[])
    for name in a.cases:
        make, F, cutoff = CASES[name]
        pc = make()
        xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(True)
        ctx.set_topology(pc)
        ctx.set_models(xyz, h_xyz)
        nres = pc.n_residues
        offsets = np.arange(F + 1, dtype=np.int64) * nres
        state = dict(d2h=0)

        def route_a():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            big = ctx.residue_pairs()
            tab = host_table(residue_pairs.split(big, offsets), nres)
            dt = time.perf_counter() - t
            state['d2h'] = nbytes(big)
            return dt, tab

        def route_b():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            tab = ctx.models_residue_persistence()
            return time.perf_counter() - t, tab

        def pass_only():
            ctx.device_synchronize()
            t = time.perf_counter()
            counts = ctx.run_launch(cutoff, 0.1, False, 6.0)
            return time.perf_counter() - t, counts

        for _ in range(2):
            _, ta = route_a()
            _, tb = route_b()
            _, counts = pass_only()
        tA, tB, tP = [], [], []
        for _ in range(a.reps):
            tA.append(route_a()[0])
            tB.append(route_b()[0])
            tP.append(pass_only()[0])
        ma, mb, mp = (1e3 * float(np.median(x)) for x in (tA, tB, tP))
        run = dict(case=name, atoms=pc.n_atoms, residues=nres, models=F, cutoff=cutoff, records={k: int(v) for k, v in counts.items()},
                   rows=len(tb['res_a']), rows_per_model_table=state['d2h'] // 93, tables_equal=bool(same(ta, tb)),
                   d2h_bytes_a=state['d2h'], d2h_bytes_b=nbytes(tb), a_median_ms=ma, b_median_ms=mb, pass_only_median_ms=mp,
                   a_minus_pass_ms=ma - mp, b_minus_pass_ms=mb - mp, a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB])
        out['runs'].append(run)
        print(json.dumps({k: v for k, v in run.items() if k not in ('a_ms', 'b_ms')}), flush=True)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
