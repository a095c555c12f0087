"""Time the pose shortlist (arp_poses_shortlist_launch, csrc/arp_poses_shortlist.h) beside the full fetch.

    python tools/pose_shortlist_probe.py --reps 11 --out profiles/pose_shortlist_probe.json

Case: that of tools/poses_probe.py — synth.proteinlike(480, 2), movable set RESNAME:HEM, poses by synth.poses_of(seed=4,
shift=3.0, jitter=0.2), (5.0, 0.1, False), P = 1024 and 16384 — and the best K = 100 poses by a weighted sum of summary slots.
Every repetition starts from a synchronised device with the receptor and the selection resident and ends with the chosen poses'
records in host memory:

    a  full      poses_contacts (launch and full fetch) + pose_shortlist.scores / order / take on the host: the only way before
    b  summary   poses_summary + poses_shortlist('summary', k=K) (launch and fetch)
    c  tanimoto  poses_summary + poses_fingerprints(n_refs=1) + poses_shortlist('tanimoto', ref=0, skip=1, k=K)

pose, score, pose_off and the five columns of a and b are asserted equal on the warm-up, before anything is timed.  The three
routes alternate (a, b, c, a, b, c, ...) in one process; medians of ``reps`` repetitions after ``warmups`` warm-ups, smallest and
largest are in the JSON.  The times are wall-clock times of one process on one device at one moment: they say how the routes
compare on this case, not what any of them costs elsewhere.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, pose_fingerprints as fp, pose_shortlist as sl, poses, synth  # noqa: E402
from arpeggio_amd.core import utils  # noqa: E402

PARAMS = (5.0, 0.1, False)
WEIGHTS = sl.weights(atom_atom={'hbond': 40, 'hydrophobic': 5, 'vdw': 3, 'weak_polar': 2, 'proximal': -1, 'vdw_clash': -60})


def nbytes(t, keys):
    return int(sum(np.asarray(t[k]).nbytes for k in keys))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', nargs='+', type=int, default=[1024, 16384])
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pc = synth.proteinlike(n_res=480, seed=2)
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    mask = np.zeros(pc.n_atoms, np.uint8)
    mask[idx] = 1
    out = dict(case='proteinlike(480, 2) RESNAME:HEM, best K by weighted summary slots (b) / by Tanimoto to pose 0 (c)', atoms=pc.n_atoms,
               movable=int(len(idx)), params=list(PARAMS), k=a.k, weights=WEIGHTS.tolist(), reps=a.reps, warmups=a.warmups, runs=[])
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(mask)
    planes = fp.planes()
    for P in a.poses:
        x, h = synth.poses_of(pc, idx, P, seed=4, shift=3.0, jitter=0.2)

        last = {}      # a route lets go of its previous result inside its own timed region: the price of freeing a full
        #                table's buffers (the runtime forgets pages it had pinned for the copy) is then the full route's own

        def route_a():
            ctx.device_synchronize()
            t = time.perf_counter()
            last.pop('a', None)
            table = ctx.poses_contacts(x, h, *PARAMS)
            score = sl.scores('summary', table['summary'], None, WEIGHTS)
            chosen = sl.order(score, 0, a.k)
            got = sl.take(table, chosen)
            got['score'] = np.array([score[p] for p in chosen.tolist()], np.int64)
            last['a'] = (got, table)
            return time.perf_counter() - t, got, table

        def route_b():
            ctx.device_synchronize()
            t = time.perf_counter()
            last.pop('b', None)
            ctx.poses_summary(x, h, *PARAMS)
            t1 = time.perf_counter()
            got = ctx.poses_shortlist('summary', weights=WEIGHTS, k=a.k)
            last['b'] = got
            return time.perf_counter() - t, got, time.perf_counter() - t1

        def route_c():
            ctx.device_synchronize()
            t = time.perf_counter()
            last.pop('c', None)
            ctx.poses_summary(x, h, *PARAMS)
            ctx.poses_fingerprints(planes, n_refs=1)
            got = ctx.poses_shortlist('tanimoto', ref=0, skip=1, k=a.k)
            last['c'] = got
            return time.perf_counter() - t, got

        for _ in range(a.warmups):
            _, ga, table = route_a()
            _, gb, _ = route_b()
            _, gc = route_c()
        for key in ('pose', 'score', 'pose_off', 'summary') + poses.COLUMNS:
            assert np.asarray(ga[key]).dtype == np.asarray(gb[key]).dtype and np.asarray(ga[key]).tobytes() == np.asarray(gb[key]).tobytes(), (P, key)
        t_a, t_b, t_c, t_s = [], [], [], []
        ga = gb = gc = None
        for _ in range(a.reps):
            t_a.append(route_a()[0])
            b = route_b()
            t_b.append(b[0])
            t_s.append(b[2])
            t_c.append(route_c()[0])
            del b
        gb, gc = last['b'], last['c']
        ms = lambda v: dict(median_ms=1e3 * float(np.median(v)), range_ms=[1e3 * min(v), 1e3 * max(v)], all_ms=[1e3 * u for u in v])  # noqa: E731
        run = dict(poses=P, records=int(len(table['i'])), chosen=int(len(gb['pose'])), chosen_records=int(len(gb['i'])),
                   chosen_records_tanimoto=int(len(gc['i'])), equal=True,
                   d2h_bytes_full=nbytes(table, ('pose_off', 'summary') + poses.COLUMNS),
                   d2h_bytes_shortlist=64 * P + nbytes(gb, ('pose', 'score', 'summary', 'pose_off') + poses.COLUMNS),
                   full=ms(t_a), summary=ms(t_b), shortlist_behind_the_summary=ms(t_s), tanimoto=ms(t_c),
                   ratio_full_to_summary=float(np.median(t_a) / np.median(t_b)))
        out['runs'].append(run)
        print(json.dumps({k: v for k, v in run.items()}, default=str)[:2000], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
