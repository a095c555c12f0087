"""The kernel paths of a pass against the oracle, one dispatcher switch at a time.

enqueue_contacts and its neighbours (arpeggio_amd/csrc/arp_api.hip) pick between a dozen kernel variants by size, sparsity
and what earlier passes over the structure left in the context.  The switches behind those choices are ARP_* environment
variables read ONCE per process (function-local statics), so every configuration of the matrix below runs in a child process
of its own: the same corpus, the same sequence of passes per structure (the history is what several switches act on), every
pass's bags written to an .npz.  The parent compares each pass with the oracle: selection masks equal, atom-atom records bit
for bit, the four ring / amide bags as the parity tests do.

Values are only those the dispatcher reaches by itself at some size or state, or values inside the ranges the code clamps
to: this is a test of results, not of robustness to nonsense settings.

test_every_switch_is_covered (CPU) keeps the matrix complete: a new ARP_* switch in csrc/ fails it until it is added here or
exempted with the test that covers it."""
import ctypes as C
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'arpeggio_amd', 'csrc')
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# ---- the matrix: configuration -> environment of its child (what it forces | when production takes that path) -------------
CONFIGS = {
    'default': {},
    'search_tile_2': {'ARP_SEARCH_TILE': '2'},                                  # k_search<0,2> | >= 60 000 cells
    'search_tile_min_cells': {'ARP_SEARCH_TILE_MIN_CELLS': '1000'},             # the same by the size rule, smaller grids
    'balance_atoms': {'ARP_SEARCH_BALANCE': '1'},                               # runs of atoms on dense grids | sparse / clumped
    'balance_cells': {'ARP_SEARCH_BALANCE': '0'},                               # runs of cells on sparse / clumped | dense
    'hint_eager_cells': {'ARP_SEARCH_BALANCE': '0', 'ARP_SEARCH_BALANCE_HINT_EAGER': '1'},   # k_balance_blocks from pass 1
    'hint_eager_atoms': {'ARP_SEARCH_BALANCE': '1', 'ARP_SEARCH_BALANCE_HINT_EAGER': '1'},   # k_cell_weights + scan + k_balance_atoms
    'hint_zero_weights': {'ARP_SEARCH_BALANCE': '1', 'ARP_SEARCH_BALANCE_HINT_EAGER': '1', 'ARP_SEARCH_W_UNIT': '0',
                          'ARP_SEARCH_W_CHUNK': '0', 'ARP_SEARCH_W_TEST_X8': '0'},      # k_balance_atoms' W <= 0 branch
    'hint_off': {'ARP_SEARCH_BALANCE_HINT': '0'},                               # no hint at all
    'hint_cells_only': {'ARP_SEARCH_BALANCE_HINT_ATOMS': '0', 'ARP_SEARCH_BALANCE_HINT_EAGER': '1'},   # runs of atoms without a hint
    'cells_unweighted': {'ARP_SEARCH_BALANCE': '0', 'ARP_SEARCH_BALANCE_HINT_EAGER': '1', 'ARP_SEARCH_CELL_WEIGHT_X16': '0'},
    'atoms_per_block_8': {'ARP_SEARCH_BALANCE': '1', 'ARP_SEARCH_APB': '8'},     # thousands of blocks, cells shared by neighbours
    'search_blocks_8': {'ARP_SEARCH_BLOCKS': '8'},                              # few long runs
    'search_blocks_4096': {'ARP_SEARCH_BLOCKS': '4096'},                        # more blocks than tiles
    'search_cpw_1': {'ARP_SEARCH_CPW': '1'},
    'compact_1024': {'ARP_COMPACT_512_MAX_ROWS': '0'},                          # k_compact_atoms<1024> | > 150 k atoms
    'tiled_scan': {'ARP_CHAINED_SCAN': '0'},                                    # k_scan_tiles + k_scan_fix | > 128 tiles or > 2 x CUs
    'stream_out': {'ARP_STREAM_OUT_MB': '0'},                                   # k_sift<1,*> / k_sift_planes<1,*> | > 6.7 M contacts
    'sift_shares_off': {'ARP_SIFT_SHARES': '0'},
    'sift_ppb_64': {'ARP_SIFT_PPB': '64'},
    'sift_bpc_1': {'ARP_SIFT_BPC': '1'},
    'planes_aside': {'ARP_PLANES_MODE': '1'},                                   # k_planes beside the search | first pass after an upload
    'plane_ipw_1': {'ARP_PLANE_IPW': '1'},
    'plane_cpw_1': {'ARP_PLANE_CPW': '1'},
    'plane_chunk_factor_min': {'ARP_PLANE_CHUNK_FACTOR_X10': '1'},
    'deterministic': {'ARP_DETERMINISTIC': '1'},                                # k_cellsort, general centre grids | > 16 384 centres
    'sort_small_one_block': {'ARP_SORT_SMALL_BLOCKS': '1'},
    'publish_by_copy': {'ARP_INKERNEL_PUBLISH': '0'},                           # k_publish_counters | caller-owned stream
    'no_spin_wait': {'ARP_SPIN_WAIT': '0'},                                     # the runtime's wait | caller-owned stream
    'join_by_stream_wait': {'ARP_JOIN_SPIN_US': '0'},
    'grids_in_first_pass': {'ARP_GRIDS_WITH_UPLOAD': '0'},                      # upload side work moved into the first pass
    'upload_on_main_stream': {'ARP_UPLOAD_ASIDE': '0'},
    'lists_in_first_pass': {'ARP_LISTS_WITH_UPLOAD': '0'},
    'static_in_first_pass': {'ARP_STATIC_WITH_UPLOAD': '0'},
    'fetch_by_copy_engine': {'ARP_FETCH_DIRECT_MAX_KB': '0'},                   # packed fetch by the copy engine | bags > 1 MB
}

# ---- switches covered elsewhere (name -> (reason, test)) ----------------------------------------------------------------
EXEMPT = {
    'ARP_SIFT_SEG_BY_BLOCK': ('segment dealt by block index instead of XCD', 'test_gpu_edge_cases.py::test_sift_blocks_dealt_by_index_give_the_same_contacts'),
    'ARP_BAG_LISTS': ('ring / amide loops called alone, list or grid walk', 'test_gpu_edge_cases.py::test_each_ring_amide_loop_alone_from_its_list_and_by_its_grid_walk'),
    'ARP_SORT_SMALL': ('one-launch small sort against the radix passes', 'test_gpu_sort.py::test_small_bags_take_the_one_launch_path_and_agree_with_the_radix_passes'),
    'ARP_EXPORT_THREADS': ('JSON writer, read on every call', 'test_gpu_paths.py::test_json_export_is_the_same_file_for_any_thread_count_and_with_mmap'),
    'ARP_EXPORT_MMAP': ('JSON writer, read on every call', 'test_gpu_paths.py::test_json_export_is_the_same_file_for_any_thread_count_and_with_mmap'),
}

BAGS = ('atom_plane', 'plane_plane', 'group_group', 'group_plane')
BAG_KEYS = {  # (columns compared exactly, angle columns compared with deg_close)
    'plane_plane': (('bgn', 'end', 'type1', 'type2', 'ctype', 'dist'), ('dihedral', 'theta_bgn', 'theta_end')),
    'atom_plane': (('atom', 'ring', 'mask', 'ctype', 'dist'), ('theta',)),
    'group_group': (('bgn', 'end', 'ctype', 'dist'), ('dihedral', 'theta')),
    'group_plane': (('amide', 'ring', 'ctype', 'dist'), ('dihedral', 'theta')),
}
# every structure runs this sequence: (cutoff, vdw_comp, sequence-adjacent pairs, selection) — whole at 5 A three times (first
# pass, hint made, hint used), another cell edge, other per-pair parameters, a partial selection, whole again
SCHEDULE = ((5.0, 0.1, False, 'all'), (5.0, 0.1, False, 'all'), (5.0, 0.1, False, 'all'), (4.0, 0.1, False, 'all'),
            (5.0, 0.3, True, 'all'), (5.0, 0.1, False, 'part'), (5.0, 0.1, False, 'all'))
CHILD_TIMEOUT = 300
HIP_ERROR_EXIT = 3      # the child's exit status after a failed HIP call (ARP_E_HIP)
_FAULTED = []      # a child that ended by a signal or a timeout: nothing more is started on the GPU


def _sparse_clusters():
    """1 500 atoms in 50-atom clusters over a 260 A box: ~140 k contact cells (above SCAN_LDS_CELLS: the scanned grid builds)."""
    from helpers import random_dense_pack
    pc = random_dense_pack(41, n=1500, box=14.0)
    rng = np.random.default_rng(260)
    shift = (rng.random((pc.n_atoms // 50 + 1, 3)) * (260.0 - 14.0)).astype(np.float32)
    pc.xyz = (np.asarray(pc.xyz) * 0.35 + shift[np.arange(pc.n_atoms) // 50]).astype(np.float32)
    par = np.repeat(np.arange(pc.n_atoms), np.diff(pc.h_off))
    pc.h_xyz = (np.asarray(pc.h_xyz).reshape(-1, 3) * 0.35 + shift[par // 50]).reshape(-1, 3)
    pc.cluster = np.arange(pc.n_atoms) // 50
    return pc


def _planes_only(seed):
    """Rings and amides and no atoms (the centres and normals of a ring / amide soup)."""
    from arpeggio_amd import synth
    from helpers import planes_only_complex
    q = synth.make_synthetic(0, seed=seed, box=(25.0, 25.0, 25.0), n_rings=40, n_amides=30)
    return planes_only_complex(q.ring_center, q.ring_normal, q.ring_res, q.amide_center, q.amide_normal, q.amide_res, q.n_residues)


def corpus():
    """[(name, upload, structure or list of structures)]; upload: 'blob' (arp_set_blob), 'classic' (the setters), 'batch'."""
    from arpeggio_amd import synth
    from helpers import random_dense_pack, threshold_edge_pack
    return [
        ('dense', 'blob', synth.config3(20_000, seed=51)),                                             # nx = 16 / 19
        ('protein', 'classic', synth.proteinlike(n_res=150, n_waters=60, seed=52)),                      # a protein in its box
        ('chain', 'blob', synth.proteinlike(n_res=1200, n_waters=600, seed=53)),                         # clumped
        ('thin', 'classic', synth.make_synthetic(1000, seed=54, box=(3.5, 60.0, 60.0))),                # nx == 1 (no ring atoms outside the box)
        ('odd_nx', 'blob', synth.make_synthetic(2500, seed=55, box=(33.5, 30.0, 30.0), n_rings=30, n_amides=40)),   # nx = 7 / 9
        ('sparse', 'classic', _sparse_clusters()),                                                     # nx = 44 / 55
        ('dense_pack', 'blob', random_dense_pack(57, n=600)),                                           # a few very full cells
        ('thresholds', 'classic', threshold_edge_pack()),
        ('rings', 'blob', synth.config5(1500, 1500, seed=58, L=45.0)),
        ('planes_only', 'classic', _planes_only(59)),
        ('one_atom', 'blob', synth.make_synthetic(1, seed=60, box=(5.0, 5.0, 5.0))),
        ('batch', 'batch', [synth.proteinlike(n_res=60 + 20 * k, n_waters=20, seed=61 + k) for k in range(3)]
         + [synth.make_synthetic(1, seed=62, box=(5.0, 5.0, 5.0)),
            _planes_only(63)]),
    ]


def partial_selection(pc):
    """Every residue but each fifth: more than SMALL_SEL_MAX atoms where the structure has them (the expansion grid runs).
    The sparse clusters: every cluster but each fourth (1 100 atoms), so that selection_plus leaves whole clusters out."""
    if getattr(pc, 'cluster', None) is not None:
        return (pc.cluster % 4 != 0).astype(np.uint8)
    return (pc.res_id % 5 != 0).astype(np.uint8)


def grid_dims(xyz, radius):
    """(nx, ny, nz) of the grid make_grid_desc (arp_api.hip) lays over these atoms with cell edge `radius`."""
    x = np.asarray(xyz, np.float64)
    if not len(x):
        return (1, 1, 1)
    return tuple(int(v) for v in np.floor((x.max(axis=0) - x.min(axis=0)) / (radius * (1.0 + 1e-6))) + 1)


# ---- the child: one configuration, the whole corpus --------------------------------------------------------------------
def _run_child(corpus_path, out_path):
    from arpeggio_amd import _capi, batch
    items = pickle.load(open(corpus_path, 'rb'))
    out, meta = {}, {}
    buf = _capi.pinned_empty(1 << 20, np.uint8)
    shared = None      # every blob goes into ONE context: after the first, each upload follows a pass (arp_set_blob's static-ahead branch)
    for name, upload, pc in items:
        if upload == 'blob':
            if shared is None:
                shared = _capi.Context(0)
                shared.set_profiling(True)
            ctx = shared
        else:
            ctx = _capi.Context(0)
            ctx.set_profiling(True)
        if upload == 'batch':
            off = ctx.set_batch(pc)
            n_atoms = int(off['atom'][-1])
            part = np.concatenate([partial_selection(p) for p in pc])
        else:
            if upload == 'blob':
                ctx.set_blob(_capi.pack_blob(pc))
            else:
                ctx.set_complex(pc)
            n_atoms = pc.n_atoms
            part = partial_selection(pc)
        prev = 'all'
        for k, (cutoff, comp, seq, sel) in enumerate(SCHEDULE):
            if sel != prev:
                ctx.set_selection(part if sel == 'part' else np.ones(n_atoms, np.uint8))
                prev = sel
            ctx.kernel_times(reset=True)
            counts = ctx.run_launch(cutoff, comp, seq, 6.0)
            bags, buf = ctx.fetch_packed(buf)
            key = f'{name}/{k}'
            for bag, cols in bags.items():
                assert len(cols[next(iter(cols))]) == counts[bag], (key, bag)
                for col, v in cols.items():
                    out[f'{key}/{bag}/{col}'] = np.array(v)
            for m, v in ctx.make_selection_masks().items():
                out[f'{key}/mask/{m}'] = v
            meta[key] = dict(launches={s: t['launches'] for s, t in ctx.kernel_times().items()}, stats=ctx.stats())
        if ctx is not shared:
            ctx.close()
    if shared is not None:
        shared.close()
    np.savez(out_path, **out)
    with open(out_path + '.json', 'w') as f:
        json.dump(meta, f)


# ---- the parent: oracle expectations (once per structure, selection and parameters), comparison -------------------------
_ORACLE = {}


def _oracle_pass(pc, cutoff, comp, seq, sel):
    import oracle
    key = (id(pc), cutoff, comp, seq, sel)
    if key not in _ORACLE:
        oc = oracle.OracleComplex(pc)
        plus = oc.make_selection(None if sel == 'all' else partial_selection(pc))
        exp = {'mask': dict(plus=plus, ring_plus=oc.ring_plus.copy(), amide_plus=oc.amide_plus.copy())}
        aa = oc.atom_contacts(cutoff, comp, seq)
        assert aa.get('err', 0) == 0
        exp['atom_atom'] = {k: aa[k] for k in ('i', 'j', 'dist', 'sift', 'ctype')}
        pp = oc.plane_plane()
        o = np.lexsort((pp['end'], pp['bgn']))
        exp['plane_plane'] = {k: v[o] for k, v in pp.items()}
        exp['atom_plane'], exp['group_group'], exp['group_plane'] = oc.atom_plane(), oc.group_group(), oc.group_plane()
        _ORACLE[key] = (pc, exp)       # (the structure stays alive with its entry: its id is the key)
    return _ORACLE[key][1]


def _compare(got, exp, where, bad):
    from helpers import planes_differences
    a, e = got['atom_atom'], exp['atom_atom']
    if len(a['i']) != len(e['i']):
        bad.append(f'{where} atom_atom: {len(a["i"])} records, the oracle has {len(e["i"])}')
    else:
        for k in ('i', 'j', 'sift', 'ctype'):
            if not np.array_equal(a[k], e[k]):
                bad.append(f'{where} atom_atom.{k} differs')
        if not np.array_equal(a['dist'].view(np.uint32), e['dist'].view(np.uint32)):
            bad.append(f'{where} atom_atom.dist not bit-identical')
    for bag in BAGS:
        exact, angles = BAG_KEYS[bag]
        g, x = got[bag], exp[bag]
        if len(g[exact[0]]) != len(x[exact[0]]):
            bad.append(f'{where} {bag}: {len(g[exact[0]])} records, the oracle has {len(x[exact[0]])}')
            continue
        bad += [f'{where} {bag}.{k} differs' for k in planes_differences(g, x, exact, angles)]


def _check_child(npz, items):
    from arpeggio_amd import batch
    bad = []
    for name, upload, pc in items:
        for k, (cutoff, comp, seq, sel) in enumerate(SCHEDULE):
            pre = f'{name}/{k}/'
            got = {}
            for key in npz.files:
                if key.startswith(pre):
                    bag, col = key[len(pre):].split('/')
                    got.setdefault(bag, {})[col] = npz[key]
            where = f'{name} pass {k} (cutoff {cutoff}, comp {comp}, seq {seq}, {sel})'
            members = [(where, pc, got)]
            if upload == 'batch':
                _, off = batch.concat_complexes(pc)
                split = {'atom_atom': batch.split_atom_contacts(got['atom_atom'], off)}
                for bag in BAGS:
                    split[bag] = batch.split_bag(bag, got[bag], off)
                members = []
                for s, p in enumerate(pc):
                    m = {bag: split[bag][s] for bag in split}
                    a0, a1 = int(off['atom'][s]), int(off['atom'][s + 1])
                    r0, r1 = int(off['ring'][s]), int(off['ring'][s + 1])
                    m0, m1 = int(off['amide'][s]), int(off['amide'][s + 1])
                    m['mask'] = dict(plus=got['mask']['plus'][a0:a1], ring_plus=got['mask']['ring_plus'][r0:r1],
                                     amide_plus=got['mask']['amide_plus'][m0:m1])
                    members.append((f'{where} member {s}', p, m))
            for w, p, g in members:
                exp = _oracle_pass(p, cutoff, comp, seq, sel)
                for m in ('plus', 'ring_plus', 'amide_plus'):
                    if not np.array_equal(g['mask'][m], exp['mask'][m]):
                        bad.append(f'{w} selection mask {m} differs')
                _compare(g, exp, w, bad)
    return bad


@pytest.fixture(scope='module')
def corpus_file(tmp_path_factory):
    items = corpus()
    path = str(tmp_path_factory.mktemp('paths') / 'corpus.pkl')
    with open(path, 'wb') as f:
        pickle.dump(items, f)
    return path, items


def run_config(name, corpus_path, out_dir):
    """One configuration in a fresh child process; returns (npz, meta).  A child ended by a signal or a timeout stops the
    matrix: the later configurations fail without starting a process."""
    if _FAULTED:
        pytest.fail(f'not run: an earlier child faulted ({_FAULTED[0]})')
    out = os.path.join(out_dir, f'{name}.npz')
    env = {k: v for k, v in os.environ.items() if not k.startswith('ARP_') or k == 'ARP_LIB_PATH'}
    env.update(CONFIGS[name])
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), corpus_path, out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _FAULTED.append(f'{name}: timed out after {CHILD_TIMEOUT} s')
        pytest.fail(f'{name}: child timed out after {CHILD_TIMEOUT} s')
    if r.returncode < 0 or r.returncode in (134, 139, HIP_ERROR_EXIT):
        _FAULTED.append(f'{name}: exit status {r.returncode}')
        pytest.fail(f'{name}: child ended by a signal or a HIP error ({r.returncode})\n{r.stderr[-3000:]}')
    assert r.returncode == 0, f'{name}: child failed ({r.returncode})\n{r.stderr[-3000:]}'
    return np.load(out), json.load(open(out + '.json'))


def _assert_reach(name, meta, items):
    """What the library shows of the path a configuration took (kernel_times slots, grid size); the rest is in the kernel trace
    (profiles/gpu_paths.md)."""
    planes_later = [meta[f'rings/{k}']['launches']['planes'] for k in range(1, len(SCHEDULE))]
    if CONFIGS[name].get('ARP_PLANES_MODE') == '1':
        assert all(n >= 1 for n in planes_later), planes_later
    elif name == 'default':
        assert not any(planes_later), planes_later       # (merged into the per-pair launch: the switch above changes something)
    # the partial selection of the sparse structure adds the scanned build of its expansion grid (> SCAN_LDS_CELLS cells: the
    # chained scan, or k_scan_tiles + k_scan_fix); no whole-structure pass over it builds a scanned grid
    whole_scans = [meta[f'sparse/{k}']['launches']['scan'] for k, step in enumerate(SCHEDULE) if step[3] == 'all']
    assert meta['sparse/5']['launches']['scan'] >= 1 and not any(whole_scans), (meta['sparse/5'], whole_scans)
    assert meta['sparse/5']['stats']['cells'] > 36_864, meta['sparse/5']['stats']
    # the thin structure's contact grid is one column wide at both cell edges
    thin = dict((n, pc) for n, _, pc in items)['thin']
    for k in (0, 3):
        nx, ny, nz = grid_dims(thin.xyz, SCHEDULE[k][0])
        assert nx == 1 and meta[f'thin/{k}']['stats']['cells'] == ny * nz, (k, meta[f'thin/{k}']['stats'], (nx, ny, nz))
    # the contact grid of a whole-structure pass is kept for the next one with the same cutoff, and rebuilt for another one
    assert meta['dense/1']['launches']['bin'] == 0 and meta['dense/3']['launches']['bin'] >= 1, (meta['dense/1'], meta['dense/3'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CONFIGS))
def test_kernel_path_equals_the_oracle(name, corpus_file, tmp_path):
    corpus_path, items = corpus_file
    npz, meta = run_config(name, corpus_path, str(tmp_path))
    try:
        bad = _check_child(npz, items)
        total = {b: sum(len(npz[k]) for k in npz.files if k.split('/')[2] == b and k.endswith(('/i', '/atom', '/bgn', '/amide')))
                 for b in ('atom_atom',) + BAGS}
    finally:
        npz.close()
        os.remove(os.path.join(str(tmp_path), f'{name}.npz'))      # (~100 MB a configuration)
    assert not bad, f'{name} ({CONFIGS[name]}): {len(bad)} differences\n' + '\n'.join(bad[:40])
    _assert_reach(name, meta, items)
    # the corpus has work for every bag
    assert all(v > 0 for v in total.values()), total


# ---- a caller-owned stream (arp_use_stream) --------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime the library has loaded (its path from the process's mappings)."""
    from arpeggio_amd import _capi
    _capi.load()
    for line in open('/proc/self/maps'):
        if 'libamdhip64' in line:
            L = C.CDLL(line.split()[-1])
            L.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
            L.hipStreamDestroy.argtypes = [C.c_void_p]
            L.hipStreamSynchronize.argtypes = [C.c_void_p]
            return L
    raise RuntimeError('the HIP runtime is not loaded')


def _expect(pc, cutoff=5.0, comp=0.1, seq=False, sel=None):
    return _oracle_pass(pc, cutoff, comp, seq, 'all' if sel is None else 'part')


def _fetch_all(ctx, counts):
    got = {'atom_atom': ctx.atom_contacts_fetch(counts['atom_atom'])}
    for bag in BAGS:
        got[bag] = ctx.fetch_bag(bag)
    got['mask'] = ctx.make_selection_masks()
    return got


def _assert_oracle(got, exp, where):
    bad = []
    for m in ('plus', 'ring_plus', 'amide_plus') if 'mask' in got else ():
        if not np.array_equal(got['mask'][m], exp['mask'][m]):
            bad.append(f'{where} selection mask {m} differs')
    _compare(got, exp, where, bad)
    assert not bad, '\n'.join(bad)


@pytest.mark.gpu
def test_passes_on_a_caller_owned_stream():
    """arp_use_stream: every pass goes on the caller's stream — no forked lists, planes merged, an unpolled upload, the counters
    copied by k_publish_counters and waited for by the runtime, stages 0 / 1 unsynchronised.  run_launch, enqueue / wait, a
    blob upload, the packed fetch with the sort enqueued by the pass, the three stages, a batch, two contexts interleaved on the
    one stream: all against the oracle; then back to the context's own stream (the caller's is destroyed only after that)."""
    from arpeggio_amd import _capi, synth
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    rich = synth.make_synthetic(3000, seed=71, box=(40.0, 40.0, 40.0), n_rings=150, n_amides=200, id='rich')
    prot = synth.proteinlike(n_res=150, n_waters=60, seed=72)
    a, b = _capi.Context(0), _capi.Context(0)
    try:
        for c in (a, b):
            c.use_stream(stream.value)
            assert c.stream_handle() == stream.value
        # classic setters, run_launch (the first pass would fork the candidate lists on an own stream)
        a.set_complex(rich)
        for cutoff in (5.0, 5.0, 4.0):
            _assert_oracle(_fetch_all(a, a.run_launch(cutoff, 0.1, False, 6.0)), _expect(rich, cutoff), ('run_launch', cutoff))
        # enqueue / wait
        a.run_enqueue(5.0, 0.3, True, 6.0)
        _assert_oracle(_fetch_all(a, a.run_wait()), _expect(rich, 5.0, 0.3, True), 'enqueue / wait')
        # a blob upload (not polled on a caller's stream), a partial selection, the packed fetch behind the sort of the pass
        a.set_blob(_capi.pack_blob(prot))
        a.set_sort_after_pass(True)
        for sel in (None, partial_selection(prot), None):
            a.set_selection(np.ones(prot.n_atoms, np.uint8) if sel is None else sel)
            counts = a.run_launch(5.0, 0.1, False, 6.0)
            bags, _ = a.fetch_packed()
            assert all(len(bags[k][next(iter(bags[k]))]) == counts[k] for k in bags)
            bags = {k: {c: np.array(v) for c, v in cols.items()} for k, cols in bags.items()}
            bags['mask'] = a.make_selection_masks()
            _assert_oracle(bags, _expect(prot, sel=sel), ('blob + fetch_packed', sel is None))
        a.set_sort_after_pass(False)
        # the three stages of a pass
        a.set_complex(rich)
        for st in (0, 1):
            a.run_stage(st, 5.0, 0.1, False, 6.0)
        counts = a.run_stage(2, 5.0, 0.1, False, 6.0)
        _assert_oracle(_fetch_all(a, counts), _expect(rich), 'run_stage 0 -> 1 -> 2')
        # a batch
        pcs = [synth.proteinlike(n_res=60 + 30 * k, n_waters=20, seed=73 + k) for k in range(3)]
        b.set_batch(pcs)
        per = b.run_batch(5.0, 0.1, False, 6.0)
        for s, p in enumerate(pcs):
            _assert_oracle(per[s], _expect(p), ('batch member', s))      # (bags only: the matrix compares a batch's masks)
        # two contexts interleaved on the one stream
        a.set_complex(prot)
        b.set_complex(rich)
        for _ in range(2):
            a.run_enqueue(5.0, 0.1, False, 6.0)
            b.run_enqueue(4.0, 0.1, False, 6.0)
            ca, cb = a.run_wait(), b.run_wait()
            _assert_oracle(_fetch_all(a, ca), _expect(prot), 'interleaved a')
            _assert_oracle(_fetch_all(b, cb), _expect(rich, 4.0), 'interleaved b')
        # back to the own streams
        for c in (a, b):
            c.use_stream(0)
            assert c.stream_handle() not in (0, stream.value)
        _assert_oracle(_fetch_all(a, a.run_launch(5.0, 0.1, False, 6.0)), _expect(prot), 'own stream again')
        b.set_blob(_capi.pack_blob(rich))
        _assert_oracle(_fetch_all(b, b.run_launch(5.0, 0.1, False, 6.0)), _expect(rich), 'own stream, blob')
    finally:
        for c in (a, b):
            c.use_stream(0)
        a.close(); b.close()
        assert hip.hipStreamDestroy(stream) == 0


def test_corpus_reaches_the_edges_it_is_meant_to():
    """The corpus has what the matrix relies on (computed from the coordinates and the oracle, no GPU): a grid one column wide,
    odd columns, a grid above SCAN_LDS_CELLS whose partial selection runs the expansion grid (more than SMALL_SEL_MAX atoms)
    and leaves whole clusters out of selection_plus."""
    items = dict((n, pc) for n, _, pc in corpus())
    for r in (5.0, 4.0):
        assert grid_dims(items['thin'].xyz, r)[0] == 1, r
        assert grid_dims(items['odd_nx'].xyz, r)[0] % 2 == 1, r
        nx, ny, nz = grid_dims(items['sparse'].xyz, r)
        assert nx * ny * nz > 36_864, r
    sparse = items['sparse']
    sel = partial_selection(sparse)
    assert 1024 < int(sel.sum()) < sparse.n_atoms
    plus = _oracle_pass(sparse, 5.0, 0.1, False, 'part')['mask']['plus']
    assert np.array_equal(plus[sel == 1], np.ones(int(sel.sum()), np.uint8)) and int(plus.sum()) < sparse.n_atoms - 200, int(plus.sum())


# ---- CPU: the registry of switches, the JSON writer's two variables ------------------------------------------------------
def _switches_in_source():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, f)
        if os.path.isfile(path) and f.endswith(('.hip', '.h', '.cpp', '.c')):
            names |= set(re.findall(r'(?:env_int|getenv)\(\s*"(ARP_[A-Z0-9_]+)"', open(path, encoding='utf-8').read()))
    return names


def test_every_switch_is_covered():
    """Every ARP_* switch of csrc/ (env_int / getenv) is set by a configuration of the matrix or exempted with the test that
    covers it; neither list names a switch the source no longer has."""
    found = _switches_in_source()
    in_matrix = {k for env in CONFIGS.values() for k in env}
    assert len(found) >= 36, sorted(found)
    missing = sorted(found - in_matrix - set(EXEMPT))
    assert not missing, f'switches without a test (add a configuration to CONFIGS or an entry to EXEMPT): {missing}'
    stale = sorted((in_matrix | set(EXEMPT)) - found)
    assert not stale, f'switches the source no longer reads: {stale}'
    assert not in_matrix & set(EXEMPT), sorted(in_matrix & set(EXEMPT))
    for name, (reason, test) in EXEMPT.items():
        mod, fn = test.split('::')
        assert reason and fn in open(os.path.join(ROOT, 'tests', mod), encoding='utf-8').read(), (name, test)


def test_json_export_is_the_same_file_for_any_thread_count_and_with_mmap(tmp_path, monkeypatch):
    """arp_write_contacts_json renders the records in blocks of 8 192 (arp_json.h: BLOCK), shares the blocks between
    ARP_EXPORT_THREADS threads and writes each at its offset by pwrite or, with ARP_EXPORT_MMAP=1, through a shared mapping (both
    read on every call).  The file is the same byte for byte for any of these, and it is json.dumps of the Python exporter's
    records — for no records, fewer records than threads, exactly one block, and several blocks with a partial last one."""
    from arpeggio_amd import synth
    from arpeggio_amd.core import export
    pc = synth.proteinlike(n_res=40, n_waters=10).ensure_labels()
    rng = np.random.default_rng(8)
    n = 3 * 8192 + 1001
    i = rng.integers(0, pc.n_atoms - 1, n).astype(np.int32)
    aa = dict(i=i, j=(i + 1 + rng.integers(0, 5, n)).clip(max=pc.n_atoms - 1).astype(np.int32),
              dist=(rng.random(n) * 6).astype(np.float32), sift=rng.integers(0, 1 << 15, n).astype(np.uint16),
              ctype=rng.integers(0, 6, n).astype(np.uint8))
    gg = dict(bgn=np.array([0], np.int32), end=np.array([2], np.int32), dist=np.array([4.29], np.float32), ctype=np.array([6], np.uint8))
    cases = {'none': {}, 'two': {'atom_atom': {k: v[:2] for k, v in aa.items()}},
             'one_block': {'atom_atom': {k: v[:8192] for k, v in aa.items()}}, 'blocks': {'atom_atom': aa, 'group_group': gg}}
    for case, bags in cases.items():
        files = {}
        for threads, mmap in (('1', None), ('3', None), ('64', None), ('3', '1'), ('64', '1')):
            monkeypatch.setenv('ARP_EXPORT_THREADS', threads)
            if mmap is None:
                monkeypatch.delenv('ARP_EXPORT_MMAP', raising=False)
            else:
                monkeypatch.setenv('ARP_EXPORT_MMAP', mmap)
            path = tmp_path / f'{case}_{threads}_{mmap}.json'
            export.write_contacts_json(str(path), pc, bags, pc.component_types)
            files[(threads, mmap)] = path.read_bytes()
        first = files[('1', None)]
        assert all(v == first for v in files.values()), (case, {k: len(v) for k, v in files.items()})
        want = json.dumps(export.contacts_json(pc, bags, pc.component_types), indent=4, sort_keys=True)
        assert first.decode('utf-8') == want, case
        assert len(json.loads(first)) == sum(len(b[next(iter(b))]) for b in bags.values())


if __name__ == '__main__':
    try:
        _run_child(sys.argv[1], sys.argv[2])
    except Exception as e:       # a failed HIP call: the parent starts nothing more on this device
        if getattr(e, 'code', None) == -2:      # ARP_E_HIP
            import traceback
            traceback.print_exc()
            sys.exit(HIP_ERROR_EXIT)
        raise
