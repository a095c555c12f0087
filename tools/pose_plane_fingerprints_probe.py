"""Time the ring / amide class planes of the pose fingerprints made on the device (arp_poses_fingerprints_planes_launch,
csrc/arp_poses_fingerprints.h) beside the host route.

    python tools/pose_plane_fingerprints_probe.py --reps 11 --out profiles/pose_plane_fingerprints_probe.json

Case and protocol: those of tools/pose_fingerprints_probe.py — synth.proteinlike(480, 2), movable set RESNAME:HEM, poses by
synth.poses_of(seed=4, shift=3.0, jitter=0.2), (5.0, 0.1, False), P = 64, 1024, 16384, pose 0 the one reference (Q = 1) — with
the 14 class planes alone, residue level.  Every repetition starts from a synchronised device with the receptor, the selection
and the plane atoms resident and ends with the scores (count, shared count and Tanimoto to the reference, occupancy) in host
memory:

    A  host    poses_summary + poses_planes (the launch and the full fetch of the four tables) + poses.plane_fingerprints and
               NumPy: the only way before
    B  device  poses_summary + poses_planes_summary (the same two launches, only the [P, 16] summaries copied) +
               poses_fingerprints with the class planes + pose_fingerprints.tanimoto
               (``device_fingerprints_median_ms``: the part of it behind the two summaries)

ids, count, cross and occupancy of the two routes are asserted equal on the warm-up, before anything is timed.  Medians of
``reps`` repetitions in one process after ``warmups`` warm-ups of each route, each route's repetitions together (the reason is in
tools/pose_fingerprints_probe.py); smallest and largest are in the JSON.  The times are wall-clock times of one process on one
device at one moment: they say how the two routes compare on this case, not what either costs elsewhere.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, pose_fingerprints as fp, poses, synth  # noqa: E402
from arpeggio_amd.core import utils  # noqa: E402

PARAMS = (5.0, 0.1, False)
PLANES = fp.planes([], 'all')
NP = fp.N_ALL_PLANES - fp.N_PLANES


def host_scores(planes_table, pc, idx):
    feats = poses.plane_fingerprints(planes_table, pc, idx)
    ids = np.array(sorted({u for f in feats for u, _ in f}), np.int32)
    occ = np.zeros((len(ids), NP), np.uint32)
    for f in feats[1:]:
        for u, q in f:
            occ[np.searchsorted(ids, u), q - poses.CLASS_PLANE] += 1
    r = dict(ids=ids, count=np.array([len(f) for f in feats], np.uint32), cross=np.array([[len(f & feats[0])] for f in feats], np.uint32),
             occupancy=occ, n_refs=1)
    return r, fp.tanimoto(r)


def table_bytes(planes_table):
    return int(sum(np.asarray(v).nbytes for name in poses.PLANE_TABLES for v in planes_table[name].values()) + planes_table['summary'].nbytes)


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
    out = dict(case='proteinlike(480, 2) RESNAME:HEM, reference = pose 0, the 14 class planes, residue level', atoms=pc.n_atoms,
               residues=pc.n_residues, movable=int(len(idx)), params=list(PARAMS), reps=a.reps, warmups=a.warmups, runs=[])
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(mask)
    ctx.set_plane_atoms(pc)
    for P in a.poses:
        x, h = synth.poses_of(pc, idx, P, seed=4, shift=3.0, jitter=0.2)

        def route_a():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.poses_summary(x, h, *PARAMS)
            table = ctx.poses_planes(x)
            r, tani = host_scores(table, pc, idx)
            return time.perf_counter() - t, r, tani, table

        def route_b():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.poses_summary(x, h, *PARAMS)
            ctx.poses_planes_summary(x)
            t1 = time.perf_counter()
            r = ctx.poses_fingerprints(PLANES, n_refs=1)
            tani = fp.tanimoto(r)
            return time.perf_counter() - t, r, tani, time.perf_counter() - t1

        for _ in range(a.warmups):
            _, ra, ta, table = route_a()
            _, rb, tb, _ = route_b()
        for key in ('ids', 'count', 'cross', 'occupancy'):
            assert np.array_equal(ra[key], rb[key]), (P, key)
        assert np.array_equal(ta, tb), (P, 'tanimoto')
        info = ctx.poses_fingerprints_info()
        t_a, t_b, t_f = [], [], []
        for _ in range(a.reps):
            t_a.append(route_a()[0])
        for _ in range(a.reps):
            b = route_b()
            t_b.append(b[0])
            t_f.append(b[3])
        U = len(rb['ids'])
        run = dict(poses=P, records={name: int(len(table[name]['ctype'])) for name in poses.PLANE_TABLES}, nodes=U, features=int(rb['count'].sum()),
                   words_per_pose=info['words'], slices=info['slices'], equal=True,
                   d2h_bytes_host=64 * P + table_bytes(table), d2h_bytes_device=2 * 64 * P + 4 * U + 4 * P + 4 * P + 4 * U * NP,
                   host_median_ms=1e3 * float(np.median(t_a)), host_range_ms=[1e3 * min(t_a), 1e3 * max(t_a)],
                   device_median_ms=1e3 * float(np.median(t_b)), device_range_ms=[1e3 * min(t_b), 1e3 * max(t_b)],
                   device_fingerprints_median_ms=1e3 * float(np.median(t_f)), ratio=float(np.median(t_a) / np.median(t_b)))
        out['runs'].append(run)
        print(json.dumps(run), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
