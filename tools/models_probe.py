"""Time an ensemble of F models of one structure (arp_set_models) against the routes that existed before it.

    python tools/models_probe.py --models 20 64 --reps 7 --out profiles/models_probe.json

Route A (model mode): set_models (only the coordinates cross PCIe; topology kept on the device) + one pass + ONE fetch_packed +
the contiguous split into models.  Route B (a batch of F structures, the best route without model mode): batch.concat_complexes
on the host + set_blob of the concatenation + declare_batch + run_batch (bag-by-bag fetches, split by structure).  B's per-model
ring / amide geometry is computed BEFORE its timing starts (it would otherwise need F single uploads), which favours B.  Both
routes deliver the same per-model bags (checked on the first repetition).  A and B alternate within one process; each
repetition is timed from a synchronised device to the bags on the host.  Also: F separate single-structure runs (set_blob + pass +
fetch_packed per model), per model, for reference.  Structure: synth.proteinlike(480, 2), models by synth.models_of(jitter=0.3).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, batch, synth  # noqa: E402
from arpeggio_amd.core import EnsembleComplex  # noqa: E402


def _same(a, b):
    for name in a:
        for c in a[name]:
            x, y = np.asarray(a[name][c]), np.asarray(b[name][c])
            if x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', type=int, nargs='+', default=[20, 64])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pc = synth.proteinlike(n_res=480, seed=2)
    out = dict(structure='proteinlike(480, 2)', n_atoms=pc.n_atoms, n_rings=pc.n_rings, n_amides=pc.n_amides, reps=a.reps, runs=[])
    for F in a.models:
        xyz, h_xyz = synth.models_of(pc, F, seed=1, jitter=0.3)
        ens = EnsembleComplex((pc, xyz, h_xyz))
        ens.initialize()                                     # topology kept, models resident (route A's context)
        pcs = [ens.model_pack(k) for k in range(F)]          # route B's per-model geometry, outside its timing
        ctx_a = ens._ctx
        ctx_b = _capi.Context(0)
        ctx_b.set_sort_after_pass(True)
        ctx_s = _capi.Context(0)
        ctx_s.set_sort_after_pass(True)
        blobs = [_capi.pack_blob(q) for q in pcs]

        def route_a():
            ctx_a.device_synchronize()
            t = time.perf_counter()
            ctx_a.set_models(xyz, h_xyz)
            per = ctx_a.run_models(5.0, 0.1, False, 6.0)
            return time.perf_counter() - t, per

        def route_b():
            ctx_b.device_synchronize()
            t = time.perf_counter()
            big, off = batch.concat_complexes(pcs)
            ctx_b.set_blob(_capi.pack_blob(big))
            ctx_b.declare_batch(off)
            per = ctx_b.run_batch(5.0, 0.1, False, 6.0)
            return time.perf_counter() - t, per

        def singles():
            ctx_s.device_synchronize()
            t = time.perf_counter()
            for b in blobs:
                ctx_s.set_blob(b)
                ctx_s.run_launch(5.0, 0.1, False, 6.0)
                ctx_s.fetch_packed()
            return time.perf_counter() - t

        _, pa = route_a()                                    # warm-up + equality of the two routes
        _, pb = route_b()
        singles()
        equal = all(_same(pa[k], pb[k]) for k in range(F))
        ta, tb, ts = [], [], []
        for _ in range(a.reps):
            ta.append(route_a()[0])
            tb.append(route_b()[0])
            ts.append(singles())
        ma, mb = float(np.median(ta)), float(np.median(tb))
        spread_b = float(max(tb) - min(tb))
        run = dict(models=F, records=int(sum(len(pa[k]['atom_atom']['j']) for k in range(F))), routes_equal=bool(equal),
                   a_ms=[1e3 * x for x in ta], b_ms=[1e3 * x for x in tb], a_median_ms=1e3 * ma, b_median_ms=1e3 * mb,
                   b_spread_ms=1e3 * spread_b, condition_a_le_b_plus_spread=bool(ma <= mb + spread_b),
                   a_per_model_ms=1e3 * ma / F, singles_per_model_ms=1e3 * float(np.median(ts)) / F)
        out['runs'].append(run)
        print(json.dumps(run), flush=True)
        ctx_b.close()
        ctx_s.close()
        ens._ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
