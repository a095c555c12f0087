"""Time the contact coupling of an ensemble — which contacts form and break together —: made on the host from fetched records
(A) against on the device (B).

    python tools/coupling_probe.py --reps 21 --out profiles/coupling_probe.json

Both routes start from resident models and end with the two tables (features a, b, count; pairs u, v, n11) in host memory; each
repetition is timed from a synchronised device.  Route A is the only route without the device product: pass + ``run_models``
(sort on the device, every record over PCIe, ``split_models``) + NumPy on the host (np.unique over (a, b) for the rows, one
byte per (model, row), the band, then ``B.T @ B`` in float32 — exact: a count stays below 2^24 — over blocks of 2048 features
against the features from the block on, and the integer criterion in int64 on every block).  Route B: pass +
``models_coupling`` (only the two tables are copied).  The tables are compared on the first repetition.  Planes: every contact
but bare proximity and 'atom_atom', every contact type; the band 0.05 ... 0.95 of the models (``coupling.counts``); \\|phi\\| >=
0.7 (``coupling.phi2_q``: q = 502).  Cases: those of tools/similarity_probe.py — synth.proteinlike(480, 2) at F = 8, 64, 256
(5.0 A) and the hub case synth.proteinlike(40, 21, 20) at F = 256, 7.5 A; models by synth.models_of(seed=4, jitter=0.3).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, coupling, similarity, synth  # noqa: E402

CASES = {'F8': (lambda: synth.proteinlike(n_res=480, seed=2), 8, 5.0), 'F64': (lambda: synth.proteinlike(n_res=480, seed=2), 64, 5.0),
         'F256': (lambda: synth.proteinlike(n_res=480, seed=2), 256, 5.0),
         'hub': (lambda: synth.proteinlike(n_res=40, seed=21, n_waters=20), 256, 7.5)}
PLANES = similarity.planes(None, ('atom_atom',))
BLOCK = 2048
MAX_PAIRS = 1 << 24


def host_coupling(per_model, n, planes, lo, hi, q):
    """The two tables from per-model atom-atom bags."""
    F = len(per_model)
    key = np.concatenate([b['i'].astype(np.int64) * n + b['j'] for b in per_model])
    f = np.repeat(np.arange(F, dtype=np.int64), [len(b['i']) for b in per_model])
    has = np.concatenate([b['sift'] for b in per_model]).astype(np.int64) & 0x7FFF | (1 << similarity.CLASS_PLANE)
    on = (has & planes) != 0
    uk, inv = np.unique(key[on], return_inverse=True)
    P = np.zeros((F, len(uk)), np.uint8)
    P[f[on], inv.reshape(-1)] = 1
    cnt = P.sum(axis=0, dtype=np.int64)
    feat = np.nonzero((cnt >= lo) & (cnt <= hi))[0]
    K = len(feat)
    B = P[:, feat].astype(np.float32)
    nf = cnt[feat]
    var = nf * (F - nf)
    us, vs, ns = [], [], []
    for s in range(0, K, BLOCK):
        e = min(s + BLOCK, K)
        n11 = (B[:, s:e].T @ B[:, s:]).astype(np.int64)
        d = F * n11 - nf[s:e, None] * nf[None, s:]
        keep = 1024 * d * d >= q * (var[s:e, None] * var[None, s:])
        keep &= np.arange(s, e)[:, None] < np.arange(s, K)[None, :]
        u, v = np.nonzero(keep)
        us.append(u + s)
        vs.append(v + s)
        ns.append(n11[u, v])
    cat = lambda x, dt: (np.concatenate(x) if x else np.zeros(0, np.int64)).astype(dt)
    features = dict(a=(uk[feat] // n).astype(np.int32), b=(uk[feat] % n).astype(np.int32), count=nf.astype(np.uint32))
    return features, dict(u=cat(us, np.uint32), v=cat(vs, np.uint32), n11=cat(ns, np.uint32)), len(uk)


def equal(x, y):
    return all(np.array_equal(x[0][k], y[0][k]) for k in x[0]) and all(np.array_equal(x[1][k], y[1][k]) for k in x[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    q, effective = coupling.phi2_q(0.7)
    out = dict(reps=a.reps, planes=PLANES, phi2_q=q, min_abs_phi=effective, occupancy=[0.05, 0.95], runs=[])
    if a.out and os.path.exists(a.out):      # (cases measured by an earlier call of the same session stay)
        with open(a.out) as fh:
            out['runs'] = [r for r in json.load(fh).get('runs', []) if r['case'] not in a.cases]
    for name in a.cases:
        make, F, cutoff = CASES[name]
        pc = make()
        n = pc.n_atoms
        lo, hi = coupling.counts(0.05, 0.95, F)
        xyz, h_xyz = synth.models_of(pc, F, seed=4, jitter=0.3)
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(True)
        ctx.set_topology(pc)
        ctx.set_models(xyz, h_xyz)
        room = [MAX_PAIRS]

        def route_a():
            ctx.device_synchronize()
            t = time.perf_counter()
            per = ctx.run_models(cutoff, 0.1, False, 6.0)
            f, p, _ = host_coupling([m['atom_atom'] for m in per], n, PLANES, lo, hi, q)
            return time.perf_counter() - t, (f, p)

        def route_b():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            try:
                r = ctx.models_coupling(PLANES, min_count=lo, max_count=hi, phi2_q=q, max_pairs=room[0])
            except _capi.NativeLibraryError as e:      # (more kept pairs than expected: come back with their number — a warm-up's matter)
                if getattr(e, 'code', None) != _capi.ARP_E_CAPACITY or not getattr(e, 'n_pairs', 0):
                    raise
                room[0] = e.n_pairs
                r = ctx.models_coupling(PLANES, min_count=lo, max_count=hi, phi2_q=q, max_pairs=room[0])
            return time.perf_counter() - t, r

        def pass_only():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(cutoff, 0.1, False, 6.0)
            return time.perf_counter() - t

        for _ in range(2):
            _, ra = route_a()
            _, rb = route_b()
            st = ctx.stats()      # (of the result just made: the next pass voids it)
            pass_only()
        tA, tB, tP = [], [], []
        for _ in range(a.reps):
            tA.append(route_a()[0])
            tB.append(route_b()[0])
            tP.append(pass_only())
        ma, mb, mp = (1e3 * float(np.median(x)) for x in (tA, tB, tP))
        K, P = len(rb[0]['a']), len(rb[1]['u'])
        run = dict(case=name, atoms=n, models=F, cutoff=cutoff, min_count=lo, max_count=hi, records=st['emitted'], rows=st['couple_rows'],
                   features=K, pairs=P, max_pairs=room[0], feature_pairs=K * (K - 1) // 2, tile_pairs=st['couple_tile_pairs'], tables_equal=bool(equal(ra, rb)),
                   d2h_bytes_a=15 * st['emitted'], d2h_bytes_b=12 * (K + P),
                   a_median_ms=ma, a_range_ms=[1e3 * min(tA), 1e3 * max(tA)], b_median_ms=mb, b_range_ms=[1e3 * min(tB), 1e3 * max(tB)],
                   pass_only_median_ms=mp, a_minus_pass_ms=ma - mp, b_minus_pass_ms=mb - mp,
                   a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB])
        out['runs'].append(run)
        print(json.dumps({k: v for k, v in run.items() if k not in ('a_ms', 'b_ms')}), flush=True)
        ctx.close()
        if a.out:      # (after every case: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
