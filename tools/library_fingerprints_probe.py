"""Time the library fingerprints (Context.library_fingerprints / library_fingerprints_best, csrc/arp_library_fingerprints.h) beside
the route a user had before them: every record copied to the host and folded in NumPy.

    python tools/library_fingerprints_probe.py --out profiles/library_fingerprints_probe.json

Case: that of tools/ligand_library_probe.py — synth.proteinlike(480, 2) as the receptor, 1 024 synthetic 'chain' ligands of 20 - 60
atoms, 16 poses each, 5.0 A.  The references are the first pose of each of the first ``--refs`` ligands, as feature lists made once
from the records (not timed).  Residue level, every contact but bare proximity, all entity kinds.  Every repetition starts from a
synchronised device with the receptor and the library resident and ends with its result in host memory:

    device   library_summary (launch, the [T, 16] summary copied) + library_fingerprints (ids, count, cross, occupancy copied) +
             library_fingerprints_best (the per-ligand table copied); the three calls are also timed one by one
    host     library_contacts (launch, every record copied) + ``host_fold`` below (NumPy: the same four arrays) +
             library_fingerprints.best on them; the fetch and the fold are also timed one by one

The two routes' results are compared for equality (``equal``); nothing else is asserted.  Not timed apart: the upload of the
poses, the contact kernel, the sort and the copies inside a call; the kernels inside the fingerprint launch; making the references.
Medians of ``reps`` repetitions in one process after ``warmups`` warm-ups of each route, smallest and largest beside them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, synth  # noqa: E402
from arpeggio_amd import library_fingerprints as lfp  # noqa: E402
from arpeggio_amd import ligand_library as ll  # noqa: E402

PARAMS = (5.0, 0.1, False)


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), range_ms=[1e3 * min(ts), 1e3 * max(ts)], all_ms=[1e3 * v for v in ts])


def host_fold(table, refs, res_id, n_nodes, planes, ctype_mask=0x7F):
    """The result of a launch from the records on the host, residue level: per selected plane the distinct (pose, node) pairs."""
    T = len(table['pose_off']) - 1
    Q = lfp.n_references(refs)
    sel = [b for b in range(15) if planes >> b & 1]
    pose = np.repeat(np.arange(T, dtype=np.int64), np.diff(table['pose_off'].astype(np.int64)))
    node = np.asarray(res_id, np.int64)[table['i']]
    sift = table['sift']
    ok = ((ctype_mask >> table['ctype'].astype(np.int64)) & 1) != 0
    count, cross = np.zeros(Q + T, np.int64), np.zeros((Q + T, Q), np.int64)
    occ = np.zeros((n_nodes, len(sel)), np.int64)
    # the references, plane by plane, as node masks
    has = np.zeros((Q, len(sel), n_nodes), bool)
    off = refs['ref_off']
    for q in range(Q):
        n, m = refs['ref_node'][off[q]:off[q + 1]], refs['ref_planes'][off[q]:off[q + 1]]
        for k, b in enumerate(sel):
            has[q, k, n[(m >> b) & 1 != 0]] = True
    count[:Q] = has.sum(axis=(1, 2))
    cross[:Q] = (has[:, None] & has[None, :]).sum(axis=(2, 3))
    for k, b in enumerate(sel):
        pick = ok & ((sift >> b) & 1 != 0)
        key = np.unique(pose[pick] * n_nodes + node[pick])
        p, u = key // n_nodes, key % n_nodes
        count[Q:] += np.bincount(p, minlength=T)
        occ[:, k] = np.bincount(u, minlength=n_nodes)
        for q in range(Q):
            cross[Q:, q] += np.bincount(p, weights=has[q, k, u], minlength=T).astype(np.int64)
    ids = np.nonzero(occ.any(axis=1) | has.any(axis=(0, 1)))[0]
    return dict(ids=ids.astype(np.int32), count=count.astype(np.uint32), cross=cross.astype(np.uint32), occupancy=occ[ids].astype(np.uint32),
                planes=planes, n_refs=Q, level='residue')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ligands', type=int, default=1024)
    ap.add_argument('--poses', type=int, default=16)
    ap.add_argument('--refs', type=int, default=4)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rec = synth.proteinlike(n_res=480, seed=2)
    ligs = synth.ligands(a.ligands, seed=1, sizes=(20, 60), kinds=('chain',))
    centre = rec.xyz.astype(np.float64).mean(axis=0)
    poses = [synth.library_poses_of(rec, lig, centre, a.poses, seed=100 + l, shift=8.0) for l, lig in enumerate(ligs)]
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, poses)
    planes = lfp.planes(None)
    ctx = _capi.Context(0)
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    table = ctx.library_contacts(off, x, h, *PARAMS)
    refs = lfp.references([lfp.reference_from_pose(table, int(off[l]), rec.res_id) for l in range(min(a.refs, a.ligands))], rec.n_residues)

    copied = [0, 0]      # bytes the last repetition of each route copied to the host: the arrays it returned

    def nbytes(d):
        return int(sum(v.nbytes for v in d.values() if isinstance(v, np.ndarray)))

    def clock(fn):
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    def device():
        ctx.device_synchronize()
        t0, summary = clock(lambda: ctx.library_summary(off, x, h, *PARAMS))
        t1, fp = clock(lambda: ctx.library_fingerprints(refs, planes))
        t2, best = clock(lambda: ctx.library_fingerprints_best())
        copied[0] = summary.nbytes + nbytes(fp) + nbytes(best)
        return (t0 + t1 + t2, t0, t1, t2), (fp, best)

    def host():
        ctx.device_synchronize()
        t0, tab = clock(lambda: ctx.library_contacts(off, x, h, *PARAMS))
        t1, fp = clock(lambda: host_fold(tab, refs, rec.res_id, rec.n_residues, planes))
        t2, best = clock(lambda: lfp.best(fp, off))
        copied[1] = nbytes({k_: v for k_, v in tab.items() if k_ != 'ligand_pose_off'})      # (that one is the argument, not a copy)
        return (t0 + t1 + t2, t0, t1, t2), (fp, best)
    for _ in range(a.warmups):
        _, (dfp, dbest) = device()
        info = ctx.library_fingerprints_info()      # (the host route's launch voids the fingerprint)
        _, (hfp, hbest) = host()
    equal = all(np.array_equal(dfp[k], hfp[k]) for k in ('ids', 'count', 'cross', 'occupancy')) and \
        all(np.array_equal(dbest[k], hbest[k]) for k in ('n_poses',) + lfp.BEST_KEYS)
    assert equal, 'the device route and the host fold differ'
    td, th = [], []
    for _ in range(a.reps):
        td.append(device()[0])
        th.append(host()[0])
    k, T, Q, U = len(table['i']), int(off[-1]), lfp.n_references(refs), len(dfp['ids'])
    col = lambda ts, c: [t[c] for t in ts]
    out = dict(case='proteinlike(480, 2) + synth.ligands(%d, seed=1, sizes=(20, 60), chain) x %d poses' % (a.ligands, a.poses), receptor_atoms=rec.n_atoms,
               receptor_residues=rec.n_residues, ligands=a.ligands, poses=T, params=list(PARAMS), records=k, level='residue', planes=planes,
               references=Q, reference_features=int(refs['ref_off'][-1]), nodes=U, words_per_row=info['words'], slices=info['slices'],
               reps=a.reps, warmups=a.warmups, equal=bool(equal),
               device=stats(col(td, 0)), device_summary=stats(col(td, 1)), device_fingerprints=stats(col(td, 2)), device_best=stats(col(td, 3)),
               host=stats(col(th, 0)), host_contacts_full_fetch=stats(col(th, 1)), host_fold=stats(col(th, 2)), host_best=stats(col(th, 3)),
               ratio_host_over_device=float(np.median(col(th, 0)) / np.median(col(td, 0))),
               d2h_bytes_device=copied[0], d2h_bytes_host=copied[1], h2d_bytes_references=nbytes(refs),
               not_timed_apart='upload, contact kernel, sort and copies inside a call; the kernels inside the fingerprint launch; making the references')
    ctx.close()
    print(json.dumps({k_: v for k_, v in out.items() if not isinstance(v, dict)}), flush=True)
    print(json.dumps({n: {q: v[q] for q in ('median_ms', 'range_ms')} for n, v in out.items() if isinstance(v, dict)}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
