"""Time the class planes of the library fingerprints (Context.library_fingerprints with a mask beyond bit 14,
csrc/arp_library_fingerprints.h) beside the host route over fully fetched ring / amide tables.

    python tools/library_plane_fingerprints_probe.py --out profiles/library_plane_fingerprints_probe.json

Case and protocol of tools/library_planes_probe.py: synth.proteinlike(480, 2) as the receptor, 1 024 ring-bearing ligands
('arylamide', 'biaryl', 'halo' with its ring) x 16 poses about the receptor's centroid, shift 8 A; the receptor, the library and its
plane table resident; every repetition starts from a synchronised device and ends with its result in host memory.  The planes are
the 14 class planes alone (neither route copies an atom-atom record), the references the ring / amide features of the first pose
of the first three ligands that have any.

    host     library_summary + library_planes with the full fetch of the four tables + ligand_library.plane_fingerprints and NumPy:
             ids, count, cross, occupancy and the best pose per ligand (library_fingerprints.best)
    device   library_summary + library_planes_summary + library_fingerprints + library_fingerprints_best

The arrays of the two routes are compared before anything is timed (``equal``; the probe stops when they differ).  Timed apart, with
both results resident: the fingerprint with its best table for the class planes alone, for all 29 planes, and for the 15 SIFt
bits through the old entry (what the new launches cost beside it).  Medians of ``reps`` repetitions in one process after
``warmups`` warm-ups of each route, smallest and largest beside them.
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
from library_planes_probe import KINDS, stats, table_bytes  # noqa: E402

ALL15, ALL29 = (1 << 15) - 1, (1 << 29) - 1
CLASSES = ALL29 & ~ALL15
PARAMS = (5.0, 0.1, False)


def host_result(feats, refs, lig_off):
    """ids, count, cross, occupancy and the best table of per-pose sets of (node, plane >= 15) and references as sets."""
    rows = refs + feats
    Q = len(refs)
    ids = np.array(sorted({u for f in rows for u, _ in f}), np.int32)
    col = {int(u): k for k, u in enumerate(ids.tolist())}
    occ = np.zeros((len(ids), 14), np.uint32)
    for f in feats:
        for u, b in f:
            occ[col[u], b - 15] += 1
    out = dict(ids=ids, count=np.array([len(f) for f in rows], np.uint32),
               cross=np.array([[len(f & r) for r in refs] for f in rows], np.uint32).reshape(len(rows), Q), occupancy=occ,
               planes=CLASSES, n_refs=Q, level='residue')
    out['best'] = lfp.best(out, lig_off)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ligands', type=int, default=1024)
    ap.add_argument('--poses', type=int, default=16)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rec0 = synth.proteinlike(n_res=480, seed=2)
    ligs = synth.ligands(a.ligands, seed=1, kinds=KINDS, planes=True)
    centre = rec0.xyz.astype(np.float64).mean(axis=0)
    ps = [synth.library_poses_of(rec0, lig, centre, a.poses, seed=100 + l, shift=8.0) for l, lig in enumerate(ligs)]
    lib = ll.pack(ligs)
    off, x, h = ll.flatten_poses(lib, ps)
    T = int(off[-1])
    # the host route names a ring's node by the resident ring_res: the receptor with the planes the device makes for it
    tmp = _capi.Context(0)
    tmp.set_topology(rec0)
    tmp.set_models(rec0.xyz[None], rec0.h_xyz[None])
    pl = tmp.models_planes()
    tmp.close()
    ctx = _capi.Context(0)
    rec = synth.proteinlike(n_res=480, seed=2)
    rec.ring_center, rec.ring_normal, rec.ring_res = pl['ring_center'][0], pl['ring_normal'][0], pl['ring_res'][0].astype(np.int32)
    rec.amide_center, rec.amide_normal = pl['amide_center'][0], pl['amide_normal'][0]
    ctx.set_complex(rec)
    ctx.set_ligand_library(lib)
    ctx.set_ligand_library_planes(lib)

    def timed(fn):
        ctx.device_synchronize()
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    # ---- the references, from a first full fetch
    table = ctx.library_planes(off, x)
    feats = ll.plane_fingerprints(table, rec)
    picks = [int(off[l]) for l in range(a.ligands) if off[l + 1] > off[l] and feats[int(off[l])]][:3]
    refs = [lfp.reference_from_plane_records(table, rec, t) for t in picks]
    ref_sets = [set(feats[t]) for t in picks]
    r29 = lfp.references(refs, rec.n_residues, classes=True)
    r15 = lfp.references([(n, m & ALL15) for n, m in refs], rec.n_residues)

    def host():
        ctx.library_summary(off, x, h, *PARAMS)
        t = ctx.library_planes(off, x)
        return host_result(ll.plane_fingerprints(t, rec), ref_sets, off)

    def fingerprint(r, planes):
        out = ctx.library_fingerprints(r, planes)
        out['best'] = ctx.library_fingerprints_best()
        return out

    def device():
        ctx.library_summary(off, x, h, *PARAMS)
        ctx.library_planes_summary(off, x)
        return fingerprint(r29, CLASSES)
    routes = dict(host=host, device=device, fingerprint_classes=lambda: fingerprint(r29, CLASSES), fingerprint_all29=lambda: fingerprint(r29, ALL29),
                  fingerprint_all15=lambda: fingerprint(r15, ALL15))
    last = {}
    for _ in range(a.warmups):
        for name, fn in routes.items():
            last[name] = timed(fn)[1]
    hst, dev = last['host'], last['device']
    equal = all(np.array_equal(hst[k], dev[k]) and hst[k].dtype == dev[k].dtype for k in ('ids', 'count', 'cross', 'occupancy'))
    equal = equal and all(np.array_equal(hst['best'][k], dev['best'][k]) for k in ('n_poses', 'best_pose', 'tanimoto_q32', 'shared', 'count'))
    assert equal, 'the host route and the device route differ'
    times = {name: [] for name in routes}
    for _ in range(a.reps):
        for name, fn in routes.items():
            times[name].append(timed(fn)[0])
    info = ctx.library_fingerprints_info()
    U, Q, L = len(dev['ids']), len(refs), a.ligands
    small = 4 * U + 4 * (Q + T) * (1 + Q) + 4 * U * 14 + L * (8 + Q * 20)
    out = dict(case='proteinlike(480, 2) + synth.ligands(%d, seed=1, kinds=%s, planes=True) x %d poses' % (a.ligands, '/'.join(KINDS), a.poses),
               receptor_atoms=rec.n_atoms, receptor_rings=rec.n_rings, receptor_amides=rec.n_amides, ligands=L, poses=T, references=Q,
               planes='the 14 class planes alone', reps=a.reps, warmups=a.warmups,
               records={name: len(table[name]['ctype']) for name in ('atom_plane', 'plane_plane', 'group_group', 'group_plane')},
               nodes=U, features=int(dev['count'][Q:].sum()), poses_with_features=int((dev['count'][Q:] > 0).sum()), words_per_row=info['words'],
               d2h_bytes_host=64 * T + table_bytes(table, T), d2h_bytes_device=2 * 64 * T + small, d2h_bytes_fingerprint=small,
               equal=bool(equal), **{name: stats(ts) for name, ts in times.items()})
    ctx.close()
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}), flush=True)
    print(json.dumps({n: {q: out[n][q] for q in ('median_ms', 'range_ms')} for n in routes}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
