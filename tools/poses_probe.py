"""Time the contacts of ligand poses on a resident receptor (Context.poses_contacts, csrc/arp_poses.h) beside the ensemble route.

    python tools/poses_probe.py --reps 11 --out profiles/poses_probe.json

Case: synth.proteinlike(480, 2), movable set RESNAME:HEM, poses by synth.poses_of(seed=4, shift=3.0, jitter=0.2), 5.0 A,
P = 64, 1024, 16384.  Every repetition starts from a synchronised device with the receptor and the selection resident and
ends with the result in host memory:

    full      poses_contacts: upload of the poses + launch (kernel, sort, columns) + fetch of records, offsets and summary
    summary   poses_summary: the same launch, only the [P, 16] summary copied

and, at P = 64 only (the route holds every pose as a whole model: 16384 of them are 97 M atom records),

    ensemble  set_models(as_models(...)) + run_models: upload of P whole models, their expansion, one pass, the packed fetch and
              its cut into models — the only way before the poses route; its per-pose cost is the baseline for larger P

The records of the two routes are compared on the warm-up (``equal``).  Medians of ``reps`` repetitions in one process after
``warmups`` warm-ups of each route; the ranges are in the JSON.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, poses, synth  # noqa: E402
from arpeggio_amd.core import utils  # noqa: E402

PARAMS = (5.0, 0.1, False)
ENSEMBLE_MAX = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', nargs='+', type=int, default=[64, 1024, 16384])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pc = synth.proteinlike(n_res=480, seed=2)
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    mask = np.zeros(pc.n_atoms, np.uint8)
    mask[idx] = 1
    out = dict(case='proteinlike(480, 2) RESNAME:HEM', atoms=pc.n_atoms, movable=int(len(idx)), params=list(PARAMS), reps=a.reps,
               warmups=a.warmups, runs=[])
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(mask)
    for P in a.poses:
        x, h = synth.poses_of(pc, idx, P, seed=4, shift=3.0, jitter=0.2)

        def full():
            ctx.device_synchronize()
            t = time.perf_counter()
            r = ctx.poses_contacts(x, h, *PARAMS)
            return time.perf_counter() - t, r

        def summary():
            ctx.device_synchronize()
            t = time.perf_counter()
            r = ctx.poses_summary(x, h, *PARAMS)
            return time.perf_counter() - t, r

        for _ in range(a.warmups):
            _, table = full()
            _, s = summary()
        assert np.array_equal(s, table['summary'])
        tf, ts = [], []
        for _ in range(a.reps):
            tf.append(full()[0])
            ts.append(summary()[0])
        k = len(table['i'])
        run = dict(poses=P, records=k, records_per_pose=k / P, h2d_bytes=int(x.nbytes + h.nbytes), d2h_bytes_full=15 * k + 8 * (P + 1) + 64 * P,
                   d2h_bytes_summary=64 * P, full_median_ms=1e3 * float(np.median(tf)), full_range_ms=[1e3 * min(tf), 1e3 * max(tf)],
                   full_per_pose_us=1e6 * float(np.median(tf)) / P, summary_median_ms=1e3 * float(np.median(ts)),
                   summary_range_ms=[1e3 * min(ts), 1e3 * max(ts)], summary_per_pose_us=1e6 * float(np.median(ts)) / P,
                   full_ms=[1e3 * v for v in tf], summary_ms=[1e3 * v for v in ts])
        if P <= ENSEMBLE_MAX:
            X, H = poses.as_models(pc, idx, x, h)
            ens = _capi.Context(0)
            ens.set_sort_after_pass(True)
            ens.set_topology(pc)

            def ensemble():
                ens.device_synchronize()
                t = time.perf_counter()
                ens.set_models(X, H)
                ens.set_selection(np.tile(mask, P))
                per = ens.run_models(*PARAMS, 6.0)
                return time.perf_counter() - t, per

            for _ in range(a.warmups):
                _, per = ensemble()
            rows = [poses.reference_rows(m['atom_atom'], mask) for m in per]
            same = all(np.array_equal(np.concatenate([r[c] for r in rows]).view(np.uint8), np.asarray(table[c]).view(np.uint8)) for c in poses.COLUMNS)
            te = [ensemble()[0] for _ in range(a.reps)]
            run.update(ensemble_median_ms=1e3 * float(np.median(te)), ensemble_range_ms=[1e3 * min(te), 1e3 * max(te)],
                       ensemble_per_pose_us=1e6 * float(np.median(te)) / P, ensemble_records=int(sum(len(m['atom_atom']['i']) for m in per)),
                       ensemble_h2d_bytes=int(X.nbytes + H.nbytes), equal=bool(same), ensemble_ms=[1e3 * v for v in te])
            ens.close()
        out['runs'].append(run)
        print(json.dumps({k_: v for k_, v in run.items() if not k_.endswith('_ms') or 'median' in k_}), flush=True)
        if a.out:      # (after every case: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(out, fh, indent=1)
    ctx.close()


if __name__ == '__main__':
    main()
