"""Time the residue-residue contact table of a pass: folded on the host from fetched bags (A) against on the device (B).

    python tools/residue_pairs_probe.py --reps 21 --out profiles/residue_pairs.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/residue_pairs_probe.py --reps 5
    python tools/residue_pairs_probe.py --kernel-stats DIR --out profiles/residue_pairs.json      # adds the kernel times

Both routes start from a resident structure and end with the table in host memory; each repetition is timed from a
synchronised device.  Route A is what existed before the device reduction: pass + ``fetch_packed`` (sort on the device, every
record of the five bags over PCIe) + a NumPy fold (np.unique over res_a * nres + res_b, np.bincount / minimum.at /
bitwise_or.at).  Route B: pass + ``residue_pairs`` (only the table is copied).  The two tables are compared on the first
repetition.  Cases: synth.proteinlike() (5.9 k atoms), synth.config3(100 000), and the batch of 64 protein-sized structures
bench.py --batch 64 times (eight distinct stand-ins, repeated); whole structures, 5.0 A.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from arpeggio_amd import _capi, batch, synth  # noqa: E402


def _batch64():
    distinct = [synth.proteinlike(seed=2 + k, id=f'standin{k}') for k in range(8)]
    return batch.concat_complexes([distinct[k % 8] for k in range(64)])


CASES = {'proteinlike': lambda: (synth.proteinlike(), None), 'config3_100k': lambda: (synth.config3(100_000), None), 'batch64': _batch64}

_PLANES = (('atom_plane', 'atom', 'ring', 'a', 'r'), ('plane_plane', 'bgn', 'end', 'r', 'r'), ('group_group', 'bgn', 'end', 'm', 'm'),
           ('group_plane', 'amide', 'ring', 'm', 'r'))


def host_table(bags, pc):
    """The table from the five fetched bags, vectorised."""
    tab = {'a': pc.res_id.astype(np.int64), 'r': pc.ring_res.astype(np.int64), 'm': pc.amide_res.astype(np.int64)}
    nres = max(pc.n_residues, 1)
    aa = bags['atom_atom']
    ra, rb = tab['a'][aa['i']], tab['a'][aa['j']]
    keys = [np.minimum(ra, rb) * nres + np.maximum(ra, rb)]
    for name, ka, kb, ta, tb in _PLANES:
        b = bags[name]
        ra, rb = tab[ta][b[ka]], tab[tb][b[kb]]
        keep = (ra >= 0) & (rb >= 0)
        keys.append(np.minimum(ra, rb)[keep] * nres + np.maximum(ra, rb)[keep])
    uk, inv = np.unique(np.concatenate(keys), return_inverse=True)
    inv = inv.reshape(-1)
    U, k = len(uk), len(keys[0])
    ia = inv[:k]
    dmin = np.full(U, np.inf, np.float32)
    np.minimum.at(dmin, ia, aa['dist'])
    sift = np.asarray(aa['sift'])
    bits = np.stack([np.bincount(ia, weights=(sift >> b) & 1, minlength=U) for b in range(15)], axis=1).astype(np.uint32)
    cm = np.zeros(U, np.uint8)
    np.bitwise_or.at(cm, ia, (1 << np.asarray(aa['ctype']).astype(np.int64)).astype(np.uint8))
    planes = np.zeros((U, 4), np.uint32)
    lo = k
    for m in range(4):
        hi = lo + len(keys[m + 1])
        planes[:, m] = np.bincount(inv[lo:hi], minlength=U)
        lo = hi
    return dict(res_a=(uk // nres).astype(np.int32), res_b=(uk % nres).astype(np.int32), n_contacts=np.bincount(ia, minlength=U).astype(np.uint32),
                dist_min=dmin, bit_count=bits, ctype_mask=cm, plane_count=planes)


def same(a, b):
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)


def kernel_stats(path):
    """Per-kernel totals of a rocprofv3 --kernel-trace --stats run (the *kernel_stats.csv under ``path``): the reduction's own
    kernels, the run detection it shares with the persistence table and the radix passes it launches."""
    out = {}
    for p in glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True):
        for row in csv.DictReader(open(p)):
            name = row.get('Name', '')
            if 'k_respair' in name or 'k_residue_rekey' in name or 'k_runs_' in name or 'k_sort_' in name:
                short = name.split('(')[0].split(' ')[-1]
                out[short] = dict(calls=int(row['Calls']), total_us=float(row['TotalDurationNs']) / 1e3, average_us=float(row['AverageNs']) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-stats', default=None, help='directory of a rocprofv3 --kernel-trace --stats run of this tool: merged into --out')
    a = ap.parse_args()
    if a.kernel_stats:
        doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        doc['kernel_stats'] = kernel_stats(a.kernel_stats)
        print(json.dumps(doc['kernel_stats']))
        if a.out:
            json.dump(doc, open(a.out, 'w'), indent=1)
        return
    out = dict(reps=a.reps, runs=[])
    for name in a.cases:
        pc, off = CASES[name]()
        ctx = _capi.Context(0)
        ctx.set_sort_after_pass(True)
        ctx.set_blob(_capi.pack_blob(pc))
        if off is not None:
            ctx.declare_batch(off)
        state = dict(buf=None, d2h=0)

        def route_a():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(5.0, 0.1, False, 6.0)
            bags, state['buf'] = ctx.fetch_packed(state['buf'])
            tab = host_table(bags, pc)
            dt = time.perf_counter() - t
            state['d2h'] = int(sum(np.asarray(v).nbytes for b in bags.values() for v in b.values()))
            return dt, tab

        def route_b():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(5.0, 0.1, False, 6.0)
            tab = ctx.residue_pairs()
            return time.perf_counter() - t, tab

        def pass_only():
            ctx.device_synchronize()
            t = time.perf_counter()
            ctx.run_launch(5.0, 0.1, False, 6.0)
            return time.perf_counter() - t

        for _ in range(2):
            _, ta = route_a()
            _, tb = route_b()
            pass_only()
        tA, tB, tP = [], [], []
        for _ in range(a.reps):
            tA.append(route_a()[0])
            tB.append(route_b()[0])
            tP.append(pass_only())
        ma, mb, mp = (1e3 * float(np.median(x)) for x in (tA, tB, tP))
        run = dict(case=name, atoms=pc.n_atoms, residues=pc.n_residues, records=int(ta['n_contacts'].sum()),
                   plane_records=ta['plane_count'].sum(axis=0).tolist(), rows=len(ta['res_a']), tables_equal=bool(same(ta, tb)),
                   d2h_bytes_a=state['d2h'], d2h_bytes_b=int(sum(np.asarray(v).nbytes for v in tb.values())),
                   a_median_ms=ma, b_median_ms=mb, pass_only_median_ms=mp, a_minus_pass_ms=ma - mp, b_minus_pass_ms=mb - mp,
                   a_ms=[1e3 * x for x in tA], b_ms=[1e3 * x for x in tB])
        out['runs'].append(run)
        print(json.dumps({k: v for k, v in run.items() if k not in ('a_ms', 'b_ms')}), flush=True)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
