"""Time the library shortlist (Context.library_shortlist, csrc/arp_library_shortlist.h) beside the full fetch it replaces.

    python tools/library_shortlist_probe.py --out profiles/library_shortlist_probe.json

Case (that of tools/ligand_library_probe.py): synth.proteinlike(480, 2) as the receptor, 1 024 synthetic 'chain' ligands of 20 - 60
atoms (synth.ligands(seed=1)), 16 poses each, 5.0 A; the K = 100 best ligands, each by its best pose.  Every repetition starts from
a synchronised device with the receptor and the library resident and ends with its result in host memory:

    summary   library_summary alone: the launch, the [T, 16] summary copied (the floor of every route below)
    a         library_contacts (every record of every pose copied) + the host mirror (library_shortlist.scores / order) + take:
              the only way to the same result without the shortlist
    b         library_summary + library_shortlist('summary', unit='ligands', k=K)
    c         library_summary + library_fingerprints (one reference) + library_shortlist('tanimoto', unit='ligands', k=K)

a = b is asserted on the warm-up, c against the host mirror over the fetched fingerprint.  The routes alternate within a
repetition.  Not timed apart: the upload, the kernel, the sort and the fetch inside a launch; inside (b) and (c) the shortlist's
launch and its fetch; inside (a) the fetch, the scores and the slicing (``a_host_ms`` times the host part once more, alone).
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
from arpeggio_amd import library_shortlist as lsl  # noqa: E402
from arpeggio_amd import ligand_library as ll  # noqa: E402

PARAMS = (5.0, 0.1, False)
WEIGHTS = lsl.weights(atom_atom={'clash': -8, 'vdw_clash': -2, 'vdw': 1, 'hbond': 5, 'weak_hbond': 2, 'xbond': 6, 'ionic': 6, 'metal_complex': 6,
                                 'aromatic': 2, 'hydrophobic': 1, 'carbonyl': 2, 'polar': 1, 'weak_polar': 1})
ALL_BUT_PROXIMAL = 0x7FFF & ~(1 << 4)


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), range_ms=[1e3 * min(ts), 1e3 * max(ts)], all_ms=[1e3 * v for v in ts])


def same(a, b, keys):
    return all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ligands', type=int, default=1024)
    ap.add_argument('--poses', type=int, default=16)
    ap.add_argument('--k', type=int, default=100)
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
    T, K = int(off[-1]), a.k
    ctx = _capi.Context(0)
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)

    def timed(fn):
        ctx.device_synchronize()
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    def host_part(table):
        score = lsl.scores('summary', table['summary'], None, WEIGHTS)
        chosen = lsl.order(score, table['ligand_pose_off'], 'ligands', K)
        out = lsl.take(table, chosen)
        out['score'] = np.array([score[t] for t in chosen.tolist()], np.int64)
        return out

    def route_a():
        return host_part(ctx.library_contacts(off, x, h, *PARAMS))

    def route_b():
        ctx.library_summary(off, x, h, *PARAMS)
        return ctx.library_shortlist('summary', unit='ligands', weights=WEIGHTS, k=K)

    # the reference of route (c): the interactions of the best pose of the best ligand of route (a)
    table = ctx.library_contacts(off, x, h, *PARAMS)
    first = host_part(table)
    refs = lfp.references([lfp.reference_from_pose(table, int(first['pose'][0]), rec.res_id, planes=ALL_BUT_PROXIMAL)])

    def route_c():
        ctx.library_summary(off, x, h, *PARAMS)
        ctx.library_fingerprints(refs, ALL_BUT_PROXIMAL)
        return ctx.library_shortlist('tanimoto', unit='ligands', ref=0, k=K)
    routes = dict(summary=lambda: ctx.library_summary(off, x, h, *PARAMS), a=route_a, b=route_b, c=route_c)
    last = {}
    for _ in range(a.warmups):
        for name, fn in routes.items():
            last[name] = timed(fn)[1]
    keys = ('ligand', 'pose', 'score', 'summary', 'pose_off') + ll.COLUMNS
    equal_ab = same(last['a'], last['b'], keys)
    assert equal_ab, 'routes (a) and (b) differ'
    fpr = ctx.library_fingerprints(refs, ALL_BUT_PROXIMAL)
    score_c = lsl.scores('tanimoto', count=fpr['count'], cross=fpr['cross'], n_refs=1, ref=0)
    want_c = lsl.take(table, lsl.order(score_c, off, 'ligands', K))
    equal_c = same(last['c'], want_c, ('ligand', 'pose', 'summary', 'pose_off') + ll.COLUMNS)
    assert equal_c, 'route (c) differs from the host mirror'
    times = {name: [] for name in routes}
    for _ in range(a.reps):
        for name, fn in routes.items():
            times[name].append(timed(fn)[0])
    host = [timed(lambda: host_part(table))[0] for _ in range(a.reps)]
    k, kb, kc = len(table['i']), len(last['b']['i']), len(last['c']['i'])
    per_entry = 4 + 4 + 8 + 64 + 8
    info = ctx.library_fingerprints_info()
    out = dict(case='proteinlike(480, 2) + synth.ligands(%d, seed=1, sizes=(20, 60), chain) x %d poses, K = %d ligands' % (a.ligands, a.poses, K),
               receptor_atoms=rec.n_atoms, ligands=a.ligands, poses=T, k=K, params=list(PARAMS), reps=a.reps, warmups=a.warmups, records=k,
               records_b=kb, records_c=kc, equal_a_b=bool(equal_ab), equal_c_mirror=bool(equal_c),
               d2h_bytes_summary=64 * T, d2h_bytes_a=15 * k + 8 * (T + 1) + 64 * T,
               d2h_bytes_b=64 * T + 15 * kb + per_entry * K + 8 + 64, d2h_bytes_c=64 * T + 8 + 15 * kc + per_entry * K + 8 + 64
               + 4 * (info['rows'] + info['rows'] * info['n_refs'] + info['nodes'] + info['nodes'] * info['planes']),
               d2h_note='(b), (c): the summary of library_summary, the launch words, the K entries and their records; (c) also what '
                        'Context.library_fingerprints copies (ids, count, cross, occupancy)',
               summary=stats(times['summary']), a=stats(times['a']), b=stats(times['b']), c=stats(times['c']), a_host_ms=stats(host),
               b_over_summary_ms=1e3 * float(np.median(times['b']) - np.median(times['summary'])),
               a_over_summary_ms=1e3 * float(np.median(times['a']) - np.median(times['summary'])),
               c_over_summary_ms=1e3 * float(np.median(times['c']) - np.median(times['summary'])),
               not_timed_apart='upload, kernel, sort and fetch inside a launch; the shortlist launch and its fetch; the fingerprint launch and its fetch '
                               'inside (c); packing the library and set_ligand_library')
    ctx.close()
    print(json.dumps({k_: v for k_, v in out.items() if not isinstance(v, dict)}), flush=True)
    print(json.dumps({n: {q: out[n][q] for q in ('median_ms', 'range_ms')} for n in ('summary', 'a', 'b', 'c', 'a_host_ms')}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
