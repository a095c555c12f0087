"""Time the model-by-model matrix of shared interaction features of an ensemble: made on the host from fetched records (A)
against on the device (B).

    python tools/similarity_probe.py --reps 21 --out profiles/similarity_probe.json

Both routes start from resident models and end with ``inter`` uint32 [F, F] in host memory; each repetition is timed from a
synchronised device.  Route A is the only route without the device product: pass + ``run_models`` (sort on the device, every
record over PCIe, ``split_models``) + NumPy on the host (np.unique over (a, b) for the rows, one byte per (model, row, plane),
``B @ B.T`` in float32 over column blocks of 65 536 — exact: a block's counts stay below 2^24 — summed in int64).  Route B: pass
+ ``models_similarity`` (only the matrix is copied).  The two matrices are compared on the first repetition.  Planes: every
contact but bare proximity and 'atom_atom' (16 planes less one), every contact type.  Cases: synth.proteinlike(480, 2) at
F = 8, 64, 256 (5.0 A) and the hub case synth.proteinlike(40, 21, 20) at F = 256, 7.5 A; models by
synth.models_of(seed=4, jitter=0.3).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, similarity, synth  # noqa: E402

CASES = {'F8': (lambda: synth.proteinlike(n_res=480, seed=2), 8, 5.0), 'F64': (lambda: synth.proteinlike(n_res=480, seed=2), 64, 5.0),
         'F256': (lambda: synth.proteinlike(n_res=480, seed=2), 256, 5.0),
         'hub': (lambda: synth.proteinlike(n_res=40, seed=21, n_waters=20), 256, 7.5)}
PLANES = similarity.planes(None, ('atom_atom',))
BLOCK = 65536


def host_inter(per_model, n, planes):
    """``inter`` from per-model atom-atom bags: the bit matrix as bytes, then its Gram product block by block."""
    F = len(per_model)
    key = np.concatenate([b['i'].astype(np.int64) * n + b['j'] for b in per_model])
    f = np.repeat(np.arange(F, dtype=np.int64), [len(b['i']) for b in per_model])
    has = np.concatenate([b['sift'] for b in per_model]).astype(np.int64) & 0x7FFF | (1 << similarity.CLASS_PLANE)
    uk, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(uk)
    sel = [q for q in range(similarity.CLASS_PLANE + 1) if (planes >> q) & 1]
    B = np.zeros((F, len(sel) * U), np.uint8)
    for p, q in enumerate(sel):
        m = ((has >> q) & 1) != 0
        B[f[m], p * U + inv[m]] = 1
    inter = np.zeros((F, F), np.int64)
    for lo in range(0, B.shape[1], BLOCK):
        blk = B[:, lo:lo + BLOCK].astype(np.float32)
        inter += (blk @ blk.T).astype(np.int64)
    return inter.astype(np.uint32), U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = dict(reps=a.reps, planes=PLANES, runs=[])
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
            inter, _ = host_inter([m['atom_atom'] for m in per], n, PLANES)
            return time.perf_counter() - t, inter

        def route_b():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            inter = ctx.models_similarity(PLANES)
            return time.perf_counter() - t, inter

        def pass_only():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            return time.perf_counter() - t

        for _ in range(2):
            _, ia = route_a()
            _, ib = route_b()
            st = ctx.stats()      # (of the matrix just made: the next pass voids it)
            pass_only()
        tA, tB, tP = [], [], []
        for _ in range(a.reps):
            tA.append(route_a()[0])
            tB.append(route_b()[0])
            tP.append(pass_only())
        ma, mb, mp = (1e3 * float(np.median(x)) for x in (tA, tB, tP))
        run = dict(case=name, atoms=n, models=F, cutoff=cutoff, records=st['emitted'], rows=st['sim_rows'], words_per_model=st['sim_words'],
                   slices=st['sim_slices'], matrices_equal=bool(np.array_equal(ia, ib)), d2h_bytes_a=15 * st['emitted'], d2h_bytes_b=int(ib.nbytes),
                   a_median_ms=ma, b_median_ms=mb, pass_only_median_ms=mp, a_minus_pass_ms=ma - mp, b_minus_pass_ms=mb - mp,
                   a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB])
        out['runs'].append(run)
        print(json.dumps({k: v for k, v in run.items() if k not in ('a_ms', 'b_ms')}), flush=True)
        ctx.close()
        if a.out:      # (after every case: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
