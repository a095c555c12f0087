"""Time the ring and amide contacts of ligand poses on a resident receptor (Context.poses_planes, csrc/arp_poses_planes.h) beside
the ensemble route.

    python tools/poses_planes_probe.py --reps 11 --out profiles/poses_planes_probe.json

Case and protocol are those of tools/poses_probe.py: synth.proteinlike(480, 2) with the planes the device makes for it resident,
movable set RESNAME:HEM, poses by synth.poses_of(seed=4, shift=3.0, jitter=0.2), P = 64, 1024, 16384.  Every repetition starts
from a synchronised device with the receptor, the selection and the plane atoms resident and ends with the result in host memory:

    full      poses_planes: upload of the poses + launch (kernel, sort, columns) + fetch of the four tables and the summary
    summary   poses_planes_summary: the same launch, only the [P, 16] summary copied
    both      poses_contacts (5.0 A) followed by poses_planes: all five bags of every pose

and, at P = 64 only,

    ensemble  set_models(as_models(...)) + run_models: the only way to these records without the poses route

The records of the two routes are compared on the warm-up (``equal``: the ensemble's bags cut to the rows with an affected
entity, every column as bytes).  Medians of ``reps`` repetitions in one process after ``warmups`` warm-ups of each route.
"""
import argparse
import copy
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


def home_pack(pc):
    """``pc`` with the planes the device makes for its coordinates (one model of its own topology)."""
    ctx = _capi.Context(0)
    ctx.set_topology(pc)
    ctx.set_models(pc.xyz[None], pc.h_xyz[None])
    pl = ctx.models_planes()
    ctx.close()
    q = copy.copy(pc)
    q.ring_center, q.ring_normal, q.ring_res = pl['ring_center'][0], pl['ring_normal'][0], pl['ring_res'][0].astype(np.int32)
    q.amide_center, q.amide_normal = pl['amide_center'][0], pl['amide_normal'][0]
    return q


def timed(ctx, fn):
    ctx.device_synchronize()
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def stats(name, ts, P):
    return {f'{name}_median_ms': 1e3 * float(np.median(ts)), f'{name}_range_ms': [1e3 * min(ts), 1e3 * max(ts)],
            f'{name}_per_pose_us': 1e6 * float(np.median(ts)) / P, f'{name}_ms': [1e3 * v for v in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', nargs='+', type=int, default=[64, 1024, 16384])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pc = home_pack(synth.proteinlike(n_res=480, seed=2))
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    mask = np.zeros(pc.n_atoms, np.uint8)
    mask[idx] = 1
    out = dict(case='proteinlike(480, 2) RESNAME:HEM', atoms=pc.n_atoms, rings=pc.n_rings, amides=pc.n_amides, movable=int(len(idx)),
               reps=a.reps, warmups=a.warmups, runs=[])
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(mask)
    ctx.set_plane_atoms(pc)
    for P in a.poses:
        x, h = synth.poses_of(pc, idx, P, seed=4, shift=3.0, jitter=0.2)
        full = lambda: timed(ctx, lambda: ctx.poses_planes(x))
        summary = lambda: timed(ctx, lambda: ctx.poses_planes_summary(x))
        both = lambda: timed(ctx, lambda: (ctx.poses_contacts(x, h, *PARAMS), ctx.poses_planes(x)))
        for _ in range(a.warmups):
            _, table = full()
            _, s = summary()
            both()
        assert np.array_equal(s, table['summary'])
        tf, ts, tb = [], [], []
        for _ in range(a.reps):
            tf.append(full()[0])
            ts.append(summary()[0])
            tb.append(both()[0])
        counts = {n: int(len(table[n]['ctype'])) for n in poses.PLANE_TABLES}
        run = dict(poses=P, records=counts, records_per_pose=sum(counts.values()) / P, h2d_bytes=int(x.nbytes), info=ctx.poses_planes_info(),
                   affected_rings_per_pose=float(table['summary'][:, 12].mean()))
        run.update(stats('full', tf, P))
        run.update(stats('summary', ts, P))
        run.update(stats('both', tb, P))
        if P <= ENSEMBLE_MAX:
            X, H = poses.as_models(pc, idx, x, h)
            ens = _capi.Context(0)
            ens.set_sort_after_pass(True)
            ens.set_topology(pc)

            def ensemble():
                ens.set_models(X, H)
                ens.set_selection(np.tile(mask, P))
                return ens.run_models(*PARAMS, 6.0)

            for _ in range(a.warmups):
                _, per = timed(ens, ensemble)
            want = poses.planes_from_rows([poses.plane_reference_rows(m, pc, idx, x[f]) for f, m in enumerate(per)], idx)
            same = all(np.asarray(table[n][c]).tobytes() == want[n][c].tobytes() for n in poses.PLANE_TABLES for c, _ in poses.plane_columns(n))
            te = [timed(ens, ensemble)[0] for _ in range(a.reps)]
            run.update(stats('ensemble', te, P))
            run.update(equal=bool(same), ensemble_h2d_bytes=int(X.nbytes + H.nbytes))
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
