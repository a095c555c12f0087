"""Time the pose fingerprints made on the device (Context.poses_fingerprints, csrc/arp_poses_fingerprints.h) beside the host route.

    python tools/pose_fingerprints_probe.py --reps 11 --out profiles/pose_fingerprints_probe.json

Case: that of tools/poses_probe.py — synth.proteinlike(480, 2), movable set RESNAME:HEM, poses by synth.poses_of(seed=4,
shift=3.0, jitter=0.2), (5.0, 0.1, False), P = 64, 1024, 16384 — with pose 0 as the one reference (Q = 1), all 15 planes, both
levels.  Every repetition starts from a synchronised device with the receptor and the selection resident and ends with the
scores (count, shared count and Tanimoto to the reference, occupancy) in host memory:

    A  host    poses_contacts (upload, launch, fetch of every record) + poses.fingerprints + NumPy: the only way before
    B  device  poses_summary (the same launch, only the [P, 16] summary copied) + poses_fingerprints + pose_fingerprints.tanimoto
               (``device_fingerprints_median_ms``: the part of it behind poses_summary, i.e. launch, fetch and Tanimoto)

ids, count, cross and occupancy of the two routes are asserted equal on the warm-up, before anything is timed.  Medians of
``reps`` repetitions in one process after ``warmups`` warm-ups of each route; smallest and largest are in the JSON.  The
repetitions of a route follow each other, first all of A, then all of B: alternated, the poses launch that followed route A's
16 ms of NumPy at P = 1024 took 12 - 30 ms instead of 0.3 ms — an effect of the host's work on the next launch (it showed with
poses_summary alone, without any fingerprint launch before it), which would have been booked on route B.  The times
are wall-clock times of one process on one device at one moment: they say how the two routes compare on this case, not what
either costs elsewhere.
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
PLANES = 0x7FFF


def host_scores(table, pc, level):
    bits, ids = poses.fingerprints(table, pc, level)
    flat = bits.reshape(len(bits), -1)
    count = flat.sum(axis=1).astype(np.uint32)
    cross = (flat & flat[:1]).sum(axis=1).astype(np.uint32)[:, None]
    r = dict(ids=ids.astype(np.int32), count=count, cross=cross, occupancy=bits[1:].sum(axis=0).astype(np.uint32), n_refs=1)
    return r, fp.tanimoto(r)


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
    out = dict(case='proteinlike(480, 2) RESNAME:HEM, reference = pose 0, all 15 planes', atoms=pc.n_atoms, residues=pc.n_residues,
               movable=int(len(idx)), params=list(PARAMS), reps=a.reps, warmups=a.warmups, runs=[])
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    ctx.set_selection(mask)
    for P in a.poses:
        x, h = synth.poses_of(pc, idx, P, seed=4, shift=3.0, jitter=0.2)
        for level in ('residue', 'atom'):
            def route_a():
                ctx.device_synchronize()
                t = time.perf_counter()
                table = ctx.poses_contacts(x, h, *PARAMS)
                r, tani = host_scores(table, pc, level)
                return time.perf_counter() - t, r, tani, len(table['i'])

            def route_b():
                ctx.device_synchronize()
                t = time.perf_counter()
                ctx.poses_summary(x, h, *PARAMS)
                t1 = time.perf_counter()
                r = ctx.poses_fingerprints(PLANES, by_residue=level == 'residue', n_refs=1)
                tani = fp.tanimoto(r)
                return time.perf_counter() - t, r, tani, time.perf_counter() - t1

            for _ in range(a.warmups):
                _, ra, ta, k = route_a()
                _, rb, tb, _ = route_b()
            for key in ('ids', 'count', 'cross', 'occupancy'):
                assert np.array_equal(ra[key], rb[key]), (P, level, key)
            assert np.array_equal(ta, tb), (P, level, 'tanimoto')
            info = ctx.poses_fingerprints_info()
            t_a, t_b, t_f = [], [], []
            for _ in range(a.reps):
                t_a.append(route_a()[0])
            for _ in range(a.reps):
                b = route_b()
                t_b.append(b[0])
                t_f.append(b[3])
            U, NP = len(rb['ids']), 15
            run = dict(poses=P, level=level, records=k, nodes=U, words_per_pose=info['words'], slices=info['slices'], equal=True,
                       d2h_bytes_host=15 * k + 8 * (P + 1) + 64 * P, d2h_bytes_device=64 * P + 4 * U + 4 * P + 4 * P + 4 * U * NP,
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
