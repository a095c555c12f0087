"""Time the library clusters (arp_library_clusters_launch, csrc/arp_library_clusters.h) beside the host route.

    python tools/library_clusters_probe.py --reps 11 --out profiles/library_clusters_probe.json

Case (that of tools/ligand_library_probe.py): synth.proteinlike(480, 2) as the receptor, 1 024 synthetic 'chain' ligands of 20 - 60
atoms (synth.ligands(seed=1)), 16 poses each, 5.0 A; fingerprints at residue level over every contact but bare proximity, no
reference.  Two clusterings: the K = 1 024 ligand shortlist by summary (each ligand by its best pose, in rank order), and all
T = 16 384 global poses.  ``max_clusters`` = 4 096, the cap.  The thresholds are the quartiles of a sample of pair values, and
2^32 (only equal fingerprints are similar: the most clusters this case can make).  Every repetition starts from a synchronised
device with the library result resident (and, for the shortlist case, the shortlist) and ends with the clustering's arrays in
host memory:

    host     library_fingerprints(bits=True) + library_clusters.leader over the order: the only way before
    device   library_fingerprints + library_clusters (launch and fetch)

The arrays of both routes are asserted equal for every threshold before anything is timed.  Each route's repetitions follow each
other (tools/pose_fingerprints_probe.py explains why).  Medians of ``reps`` repetitions after ``warmups`` warm-ups, smallest and
largest are in the JSON, with the bytes copied back, C, the rounds that elected a leader, the rounds enqueued, the launches and
the host waits of the device route.  A host repetition that takes longer than ``--slow`` seconds is repeated ``--slow-reps``
times only (``host_reps`` says how often).  The times are wall-clock times of one process on one device at one moment: they say
how the routes compare on this case, not what either of them costs elsewhere; nothing here is a pass criterion.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, synth  # noqa: E402
from arpeggio_amd import library_clusters as lcl  # noqa: E402
from arpeggio_amd import library_fingerprints as lfp  # noqa: E402
from arpeggio_amd import library_shortlist as lsl  # noqa: E402
from arpeggio_amd import ligand_library as ll  # noqa: E402

PARAMS = (5.0, 0.1, False)
ARRAYS = lcl.PER_POSITION + lcl.PER_CLUSTER
MAX_CLUSTERS = lcl.MAX_CLUSTERS


def nbytes(t, keys):
    return int(sum(np.asarray(t[k]).nbytes for k in keys))


def enqueued(rounds_run, M, max_clusters):
    """What arp_library_clusters_launch enqueues: (rounds, launches, host waits).  Groups of LIBCL_ROUNDS_PER_WAIT rounds until the
    word behind a group is the sentinel (no round is left to run) or min(max_clusters, ceil(M / 32)) rounds are out; one launch
    for the positions, two a round, one to finish; a wait behind every group but the last, and the last one."""
    total, per = min(max_clusters, -(-M // lcl.WINDOW)), _capi.LIBCL_ROUNDS_PER_WAIT
    done, waits = 0, 1
    while done < total:
        done = min(total, done + per)
        if done < total:
            waits += 1
            if rounds_run <= done:
                break
    return done, 2 + 2 * done, waits


def sample_pair_values(f, order, n, seed=9):
    rng = np.random.default_rng(seed)
    Q = int(f['n_refs'])
    count = np.asarray(f['count'])
    rows = np.ascontiguousarray(f['bits'], np.uint64).reshape(len(count), -1)
    a, b = rng.choice(order, n), rng.choice(order, n)
    keep = a != b
    return sorted(lcl.pair_q32(rows[Q + p], rows[Q + q], count[Q + p], count[Q + q]) for p, q in zip(a[keep].tolist(), b[keep].tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ligands', type=int, default=1024)
    ap.add_argument('--poses', type=int, default=16)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--slow', type=float, default=1.0)
    ap.add_argument('--slow-reps', type=int, default=3)
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rec = synth.proteinlike(n_res=480, seed=2)
    ligs = synth.ligands(a.ligands, seed=1, sizes=(20, 60), kinds=('chain',))
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    poses = [synth.library_poses_of(rec, lig, centre, a.poses, seed=100 + l, shift=8.0) for l, lig in enumerate(ligs)]
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, poses)
    T = int(off[-1])
    lig_of = lcl.ligands_of(off)
    planes = lfp.planes(None)
    w = lsl.weights(atom_atom={'records': 1})
    ctx = _capi.Context(0)
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    ctx.library_summary(off, x, h, *PARAMS)
    out = dict(case='proteinlike(480, 2) + synth.ligands(%d, seed=1, sizes=(20, 60), chain) x %d poses, residue level, no reference' % (a.ligands, a.poses),
               poses=T, params=list(PARAMS), max_clusters=MAX_CLUSTERS, reps=a.reps, warmups=a.warmups, window=lcl.WINDOW,
               rounds_per_wait=_capi.LIBCL_ROUNDS_PER_WAIT, runs=[])
    ms = lambda v: dict(median_ms=1e3 * float(np.median(v)), range_ms=[1e3 * min(v), 1e3 * max(v)])  # noqa: E731
    for name in ('shortlist', 'all'):
        if name == 'shortlist':
            short = ctx.library_shortlist('summary', unit='ligands', weights=w, k=a.ligands)
            order = short['pose'].astype(np.int64)
        else:
            order = np.arange(T, dtype=np.int64)
        M = len(order)
        f = ctx.library_fingerprints(None, planes, bits=True)
        values = sample_pair_values(f, order, a.sample)
        thresholds = sorted({values[int(q * (len(values) - 1))] for q in (0.25, 0.5, 0.75)} | {lcl.ONE_Q32})
        for thr in thresholds:
            def host():
                ctx.device_synchronize()
                t = time.perf_counter()
                fr = ctx.library_fingerprints(None, planes, bits=True)
                got = lcl.leader(fr, thr, order=order, ligand_of=lig_of, max_clusters=MAX_CLUSTERS)
                return time.perf_counter() - t, got, fr

            def device():
                ctx.device_synchronize()
                t = time.perf_counter()
                fr = ctx.library_fingerprints(None, planes)
                t1 = time.perf_counter()
                got = ctx.library_clusters(thr, source=name, max_clusters=MAX_CLUSTERS)
                return time.perf_counter() - t, got, fr, time.perf_counter() - t1

            once, gh, fh = host()
            _, gd, fd, _ = device()
            for key in ARRAYS:      # equal before anything is timed
                u, v = np.asarray(gh[key]), np.asarray(gd[key])
                assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (name, thr, key)
            assert gh['unassigned'] == gd['unassigned']
            info = ctx.library_clusters_info()
            host_reps = a.slow_reps if once > a.slow else a.reps
            for _ in range(max(a.warmups - 1, 0) if once <= a.slow else 0):
                host()
            t_h = [host()[0] for _ in range(host_reps)]
            for _ in range(max(a.warmups - 1, 0)):
                device()
            runs = [device() for _ in range(a.reps)]
            t_d, t_c = [r[0] for r in runs], [r[3] for r in runs]
            del runs
            C = int(len(gd['leader']))
            rounds, launches, waits = enqueued(info['rounds'], M, MAX_CLUSTERS)
            run = dict(source=name, positions=M, threshold_q32=int(thr), threshold=int(thr) / lcl.ONE_Q32, equal=True, clusters=C,
                       unassigned=int(gd['unassigned']), largest=int(gd['size'].max()), words=info['words'], rounds=info['rounds'],
                       rounds_enqueued=rounds, launches=launches, waits=waits, round_form_launches=C + 1,
                       d2h_bytes_host=nbytes(fh, ('ids', 'count', 'cross', 'occupancy', 'bits')),
                       d2h_bytes_device=nbytes(fd, ('ids', 'count', 'cross', 'occupancy')) + nbytes(gd, ARRAYS),
                       host_reps=host_reps, host=ms(t_h), device=ms(t_d), clusters_behind_the_fingerprint=ms(t_c),
                       ratio_host_to_device=float(np.median(t_h) / np.median(t_d)))
            out['runs'].append(run)
            print(json.dumps(run), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, 'w') as fh_:
            json.dump(out, fh_, indent=1)
            fh_.write('\n')


if __name__ == '__main__':
    main()
