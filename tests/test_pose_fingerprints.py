"""Pose fingerprints (arp_poses_fingerprints_launch / _fetch / _info, Context.poses_fingerprints, arpeggio_amd.pose_fingerprints,
InteractionComplex.run_pose_fingerprints).

The yardstick is NumPy over the table ``Context.poses_contacts`` fetches — code this feature does not touch: keep the rows whose
``ctype`` is in the mask and whose ``sift`` meets the planes, ``poses.fingerprints`` of those, the selected planes; a pose's
features are a set of integers, ``count`` its size, ``cross`` / ``inter`` ``len(np.intersect1d(...))``, ``occupancy`` the sum over
the poses behind the references, ``bits`` packed by ``pack_bits``.  For one case the table comes from the ensemble route instead
(``poses.as_models``, ``poses.reference_rows``).  Every comparison is exact equality of integers: no tolerance, no time."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

from arpeggio_amd import _capi, pose_fingerprints as fp, poses, synth
from arpeggio_amd.core import config, utils
from arpeggio_amd.core.interactions import EnsembleComplex, InteractionComplex
from helpers import tiny_complex

BIT = {n: 1 << k for k, n in enumerate(config.SIFT_NAMES)}
CT = {n: k for k, n in enumerate(config.CONTACT_TYPE_NAMES)}
ALL15 = 0x7FFF
SCATTERED = BIT['vdw'] | BIT['hbond'] | BIT['hydrophobic'] | BIT['weak_polar']      # a non-contiguous mask
PARAMS = ((5.0, 0.1, False), (4.0, 0.25, True), (6.0, 0.1, False))


# ------------------------------------------------------------------------------------------------------------- yardstick
def pack_bits(sel):
    """bool [P, U, NP] -> uint64 [P, NP, ceil(U / 64)]: feature (u, k) is bit u & 63 of word u >> 6 of plane k."""
    P, U, NP = sel.shape
    wpp = (U + 63) // 64
    padded = np.zeros((P, NP, wpp * 64), np.uint8)
    padded[:, :, :U] = sel.transpose(0, 2, 1)
    return np.packbits(padded, axis=2, bitorder='little').reshape(P, NP, wpp, 8).view('<u8').reshape(P, NP, wpp)


def kept_rows(table, planes, ctype_mask):
    """The participating records of ``table`` as a table of the same poses."""
    keep = (((ctype_mask >> table['ctype'].astype(np.int64)) & 1) != 0) & ((table['sift'] & planes) != 0)
    rows = {k: np.asarray(table[k])[keep] for k in poses.COLUMNS}
    P = poses.n_poses(table)
    rows['pose_off'] = np.searchsorted(poses.pose_of(table)[keep], np.arange(P + 1)).astype(np.uint64)
    rows['movable'] = table['movable']
    return rows


def yardstick(table, pc, planes, ctype_mask=0x7F, level='residue', n_refs=0, all_pairs=False):
    rows = kept_rows(table, planes, ctype_mask)
    bits, ids = poses.fingerprints(rows, pc, level)
    sel = bits[:, :, [k for k in range(15) if (planes >> k) & 1]]
    feats = [np.flatnonzero(sel[p].ravel()) for p in range(len(sel))]
    P = len(feats)
    out = dict(ids=ids.astype(np.int32), count=np.array([len(f) for f in feats], np.uint32),
               cross=np.array([[len(np.intersect1d(feats[p], feats[q])) for q in range(n_refs)] for p in range(P)], np.uint32).reshape(P, n_refs),
               occupancy=sel[n_refs:].sum(axis=0).astype(np.uint32).reshape(len(ids), sel.shape[2]), bits=pack_bits(sel), sel=sel)
    if all_pairs:
        out['inter'] = np.array([[len(np.intersect1d(feats[p], feats[q])) for q in range(P)] for p in range(P)], np.uint32)
    return out


def differences(got, want, keys=('ids', 'count', 'cross', 'occupancy')):
    return [k for k in keys if np.asarray(got[k]).dtype != np.asarray(want[k]).dtype or np.asarray(got[k]).shape != np.asarray(want[k]).shape
            or not np.array_equal(got[k], want[k])]


# ------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def protein():
    return synth.proteinlike(n_res=40, seed=21, n_waters=20)


def _mask(pc, idx):
    m = np.zeros(pc.n_atoms, np.uint8)
    m[idx] = 1
    return m


def _ctx(pc, idx=None):
    ctx = _capi.Context(0)
    ctx.set_complex(pc)
    if idx is not None:
        ctx.set_selection(_mask(pc, idx))
    return ctx


@functools.lru_cache(maxsize=None)
def hem_case():
    """HEM in the small protein, 70 poses (not a multiple of 64) with noise on atoms; pose 0 is the resident one."""
    pc = protein()
    idx = utils.selection_parser(['RESNAME:HEM'], pc)
    x, h = synth.poses_of(pc, idx, 70, seed=11, shift=3.0, jitter=0.2)
    return pc, idx, x, h


@functools.lru_cache(maxsize=None)
def water_case(P):
    """A single water (S = 1 heavy atom) walking through the small protein."""
    pc = protein()
    waters = [r for r in range(pc.n_residues) if pc.res_name[r] == 'HOH']
    heavy = (np.asarray(pc.flags) & config.F_HYDROGEN) == 0

    def partners(r):
        a = pc.xyz[(pc.res_id == r) & heavy].astype(np.float64)
        b = pc.xyz[(pc.res_id != r) & heavy].astype(np.float64)
        return int((np.linalg.norm(a[:, None] - b[None], axis=2) <= 4.5).any(axis=0).sum())
    r = max(waters, key=partners)
    idx = np.nonzero(pc.res_id == r)[0]
    x, h = synth.poses_of(pc, idx, P, seed=3, shift=6.0, jitter=0.0)
    return pc, idx, x, h


def chain_case(K):
    """K receptor atoms on a line 3 A apart, a residue each, and one further atom — the movable set.  Pose k sits 3 A beside
    atom k: at 5 A it reaches k - 1, k, k + 1 (3.0 A and 4.24 A; k +- 2 is 6.7 A away).  Pose K is 50 A away."""
    line = np.stack([3.0 * np.arange(K), np.zeros(K), np.zeros(K)], axis=1)
    pc = tiny_complex(np.concatenate([line, [[0.0, -40.0, 0.0]]]))
    x = np.concatenate([line + np.array([0.0, 3.0, 0.0]), [[0.0, 50.0, 0.0]]]).astype(np.float32)[:, None, :]
    return pc, np.array([K]), x, np.zeros((K + 1, 0, 3))


# ------------------------------------------------------------------------------------------------------------- CPU
def hand_result():
    """Two references and three poses over three nodes (residues 3, 7, 9) and two planes (hbond, hydrophobic), by hand.
                     node 3      node 7      node 9
        ref 0        hb hy       hb .        . .          3 features
        ref 1        .  .        hb .        . hy         2
        pose 2       hb hy       hb .        . hy         4: shares 3 with ref 0, 2 with ref 1
        pose 3       .  .        .  .        . .          0
        pose 4       .  hy       .  .        hb .         2: shares 1 with ref 0, 0 with ref 1"""
    sel = np.zeros((5, 3, 2), bool)
    sel[0, 0] = [1, 1]; sel[0, 1, 0] = 1
    sel[1, 1, 0] = 1; sel[1, 2, 1] = 1
    sel[2, 0] = [1, 1]; sel[2, 1, 0] = 1; sel[2, 2, 1] = 1
    sel[4, 0, 1] = 1; sel[4, 2, 0] = 1
    return dict(ids=np.array([3, 7, 9], np.int32), count=np.array([3, 2, 4, 0, 2], np.uint32),
                cross=np.array([[3, 1], [1, 2], [3, 2], [0, 0], [1, 0]], np.uint32),
                occupancy=np.array([[1, 2], [1, 0], [1, 1]], np.uint32), bits=pack_bits(sel),
                planes=BIT['hbond'] | BIT['hydrophobic'], n_refs=2, level='residue'), sel


def test_the_host_module_on_the_hand_made_result():
    r, sel = hand_result()
    assert fp.plane_names(r['planes']) == ['hbond', 'hydrophobic'] and fp.reference_counts(r).tolist() == [3, 2]
    # the hand-made numbers are those of the definition
    feats = [set(np.flatnonzero(sel[p].ravel()).tolist()) for p in range(5)]
    assert [len(f) for f in feats] == r['count'].tolist()
    assert [[len(feats[p] & feats[q]) for q in range(2)] for p in range(5)] == r['cross'].tolist()
    assert sel[2:].sum(axis=0).tolist() == r['occupancy'].tolist()
    t = fp.tanimoto(r)
    assert t.dtype == np.float64 and t.shape == (5, 2)
    assert t.tolist() == [[1.0, 1 / 4], [1 / 4, 1.0], [3 / 4, 2 / 4], [0.0, 0.0], [1 / 4, 0.0]]
    rec = fp.recovery(r)
    assert rec.tolist() == [[1.0, 1 / 2], [1 / 3, 1.0], [1.0, 1.0], [0.0, 0.0], [1 / 3, 0.0]]
    assert fp.rank(r).tolist() == [0, 2, 1, 4, 3] and fp.rank(r, 1, 'recovery').tolist() == [1, 2, 0, 3, 4]
    assert fp.rank(r, 0, 'shared').tolist() == [0, 2, 1, 4, 3]
    with pytest.raises(ValueError):
        fp.rank(r, 2)
    with pytest.raises(ValueError):
        fp.rank(r, 0, 'distance')
    # the stripped form gives the poses' rows of the same numbers
    s = fp.strip_references(r)
    assert s['count'].tolist() == [4, 0, 2] and s['reference_count'].tolist() == [3, 2] and s['reference_cross'].tolist() == [[3, 1], [1, 2]]
    assert np.array_equal(fp.tanimoto(s), t[2:]) and np.array_equal(fp.recovery(s), rec[2:]) and fp.rank(s).tolist() == [0, 2, 1]
    assert 'bits' not in s and fp.strip_references(s)['count'].tolist() == [4, 0, 2]
    # a pose and a reference both without features: identical fingerprints, as similarity.tanimoto decides it
    e = dict(r, count=np.array([0, 2, 0], np.uint32), cross=np.array([[0], [0], [0]], np.uint32), n_refs=1)
    assert fp.tanimoto(e).tolist() == [[1.0], [0.0], [1.0]] and fp.recovery(e).tolist() == [[1.0], [1.0], [1.0]]
    assert fp.planes(['hbond', 'hydrophobic']) == r['planes'] and fp.planes() == 0x7FFF & ~BIT['proximal']
    with pytest.raises(ValueError):
        fp.planes(['nonsense'])


def test_unpack_against_the_packer():
    r, sel = hand_result()
    assert np.array_equal(fp.unpack(r), sel) and fp.unpack(r).dtype == np.bool_
    rng = np.random.RandomState(5)
    for U in (0, 1, 63, 64, 65, 130):
        s = rng.rand(4, U, 3) < 0.4
        b = pack_bits(s)
        assert b.shape == (4, 3, (U + 63) // 64) and b.dtype == np.uint64
        assert np.array_equal(fp.unpack(dict(bits=b, ids=np.arange(U))), s)
        if U == 65:
            assert (b[:, :, 1] >> np.uint64(1)).max() == 0 and int(b[0, 0, 0]) & 1 == int(s[0, 0, 0])
    with pytest.raises(ValueError):
        fp.unpack(dict(bits=np.zeros((2, 1, 3), np.uint64), ids=np.arange(65)))


def test_merge_adds_occupancy_by_id_and_refuses_other_references():
    r, _ = hand_result()
    # chunk a: the references and pose 2 — node 9 only through reference 1 and pose 2; chunk b: the references, poses 3 and 4
    a = dict(r, count=r['count'][:3], cross=r['cross'][:3], occupancy=np.array([[1, 1], [1, 0], [0, 1]], np.uint32))
    b = dict(r, count=r['count'][[0, 1, 3, 4]], cross=r['cross'][[0, 1, 3, 4]], occupancy=np.array([[0, 1], [0, 0], [1, 0]], np.uint32))
    m = fp.merge([a, b])
    assert differences(m, r) == [] and m['n_refs'] == 2 and m['planes'] == r['planes'] and 'bits' not in m
    assert differences(fp.merge([a]), a) == []
    # disjoint and overlapping ids: chunk c saw nodes 1 and 7 only
    c = dict(b, ids=np.array([1, 7], np.int32), occupancy=np.array([[2, 0], [0, 5]], np.uint32))
    m = fp.merge([a, c])
    assert m['ids'].tolist() == [1, 3, 7, 9] and m['occupancy'].tolist() == [[2, 0], [1, 1], [1, 5], [0, 1]]
    assert m['count'].tolist() == [3, 2, 4, 0, 2]
    bad = dict(b, count=np.array([3, 1, 0, 2], np.uint32))
    with pytest.raises(ValueError, match='different references'):
        fp.merge([a, bad])
    bad = dict(b, cross=np.array([[3, 1], [1, 1], [0, 0], [1, 0]], np.uint32))
    with pytest.raises(ValueError, match='different references'):
        fp.merge([a, bad])
    with pytest.raises(ValueError):
        fp.merge([a, dict(b, planes=BIT['hbond'])])
    with pytest.raises(ValueError):
        fp.merge([])
    with pytest.raises(ValueError):
        fp.merge([fp.strip_references(a), b])


def test_records_and_the_csv_text(tmp_path):
    pc = protein()
    r, _ = hand_result()
    recs = fp.to_records(r, pc)
    assert len(recs) == 8 and recs[2] == {'pose': 2, 'type': 'pose-fingerprint', 'count': 4, 'references': [
        {'reference': 0, 'shared': 3, 'tanimoto': 0.75, 'recovery': 1.0}, {'reference': 1, 'shared': 2, 'tanimoto': 0.5, 'recovery': 1.0}]}
    assert recs[5] == {'node': 'A/4/', 'type': 'pose-occupancy', 'level': 'residue', 'poses': {'hbond': 1, 'hydrophobic': 2}}
    ic = InteractionComplex(pc)
    with pytest.raises(AttributeError):
        ic.write_pose_fingerprints(str(tmp_path))
    ic.pose_fingerprints = fp.strip_references(r)
    path = ic.write_pose_fingerprints(str(tmp_path))
    assert os.path.basename(path) == 'proteinlike.posefp'
    assert open(path).read().splitlines() == [
        'pose,count,shared_0,tanimoto_0,recovery_0,shared_1,tanimoto_1,recovery_1',
        '0,4,3,0.75,1.0,2,0.5,1.0',
        '1,0,0,0.0,0.0,0,0.0,0.0',
        '2,2,1,0.25,0.3333333333333333,0,0.0,0.0',
        'node,hbond,hydrophobic',
        'A/4/,1,2', 'A/8/,1,0', 'A/10/,1,1']
    # atom level labels a node as the other tables label an atom
    a = dict(r, level='atom', ids=np.array([0, 1, 2], np.int32))
    fp.write_csv(str(tmp_path / 'atoms.csv'), a, pc)
    assert open(str(tmp_path / 'atoms.csv')).read().splitlines()[-3:] == ['A/1/%s,%d,%d' % (pc.atom_name[k], *r['occupancy'][k]) for k in range(3)]


def test_the_header_and_the_binding_name_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'arpeggio_hip.h')).read()
    for s in ('arp_poses_fingerprints_launch', 'arp_poses_fingerprints_fetch', 'arp_poses_fingerprints_info'):
        assert s in _capi.SYMBOLS and 'int %s(' % s in hdr
    assert '#define ARP_POSEFP_MAX_REFS %d' % _capi.POSEFP_MAX_REFS in hdr and '#define ARP_POSEFP_PLANES %d' % _capi.POSEFP_PLANES in hdr
    assert '#define ARP_POSEFP_BY_RESIDUE %du' % _capi.POSEFP_BY_RESIDUE in hdr and '#define ARP_POSEFP_ALL_PAIRS %du' % _capi.POSEFP_ALL_PAIRS in hdr
    assert fp.MAX_REFS == _capi.POSEFP_MAX_REFS and fp.N_PLANES == _capi.POSEFP_PLANES


def _slices(W, tiles, num_cu=256):
    """The slicing rule of the popcount products (arp_models_similarity_launch's), on the host."""
    chunks = (W + 31) // 32
    want = max(1, min(chunks, (2 * num_cu + tiles - 1) // tiles))
    per = (chunks + want - 1) // want * 32
    return (W + per - 1) // per


def test_the_slicing_rule_on_the_host():
    assert _slices(15, 2) == 1 and _slices(32, 1) == 1 and _slices(33, 1) == 2 and _slices(45, 2) == 2
    assert _slices(480, 2) == 15 and _slices(480, 16384) == 1 and _slices(480, 300) == 2


# ------------------------------------------------------------------------------------------------------------- GPU: seams
@pytest.mark.gpu
@pytest.mark.parametrize('K', [63, 64, 65, 129])
def test_word_seams(K):
    pc, idx, x, h = chain_case(K)
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, True)
    for planes in (ALL15, BIT['proximal']):
        want = yardstick(table, pc, planes, level='atom', n_refs=2)
        assert len(want['ids']) == K and want['ids'].tolist() == list(range(K))      # the case reaches its seam
        got = ctx.poses_fingerprints(planes, by_residue=False, n_refs=2, bits=True)
        assert differences(got, want, ('ids', 'count', 'cross', 'occupancy', 'bits')) == [], (K, planes)
        info = ctx.poses_fingerprints_info()
        NP = bin(planes).count('1')
        assert (info['poses'], info['n_refs'], info['nodes'], info['planes'], info['words']) == (K + 1, 2, K, NP, NP * ((K + 63) // 64))
        assert got['count'][K] == 0 and not got['cross'][K].any() and not got['bits'][K].any()      # the pose 50 A away
        if planes == ALL15:      # whatever bits a record has: pose k touches the atoms k - 1, k, k + 1
            touched = fp.unpack(got).any(axis=2)
            band = np.abs(np.arange(K + 1)[:, None] - np.arange(K)[None, :]) <= 1
            band[K] = False
            assert np.array_equal(touched, band)
        if K % 64:      # the padding bits of the last word
            assert int((got['bits'][:, :, -1] >> np.uint64(K % 64)).max()) == 0
        assert np.array_equal(fp.unpack(got), want['sel'])
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 2, 63, 64, 65, 130])
def test_tile_seams_of_the_product(P):
    pc, idx, x, h = water_case(130)
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x[:P], h[:P], 5.0, 0.1, False)
    for level in ('residue', 'atom'):
        for Q in sorted({q for q in (0, 1, 2, P if P <= 64 else 64) if q <= P}):
            want = yardstick(table, pc, ALL15, level=level, n_refs=Q)
            got = ctx.poses_fingerprints(ALL15, by_residue=level == 'residue', n_refs=Q, bits=True)
            assert differences(got, want, ('ids', 'count', 'cross', 'occupancy', 'bits')) == [], (P, level, Q)
            assert got['cross'].shape == (P, Q) and got['n_refs'] == Q and got['level'] == level
            assert all(got['cross'][q, q] == got['count'][q] for q in range(Q))
    if P == 130:
        assert len(want['ids']) > 64 and want['count'].max() > 8      # more than one word of columns, rows that are not trivial
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: contents
@pytest.mark.gpu
@pytest.mark.parametrize('params', PARAMS, ids=[f'{c}-{v}-{int(s)}' for c, v, s in PARAMS])
def test_contents_on_the_haem(params):
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, *params)
    for level in ('residue', 'atom'):
        for planes in (ALL15, BIT['hydrophobic'], SCATTERED):
            for ctype_mask in (0x7F, 1 << CT['INTER']):
                want = yardstick(table, pc, planes, ctype_mask, level, n_refs=2)
                got = ctx.poses_fingerprints(planes, ctype_mask, by_residue=level == 'residue', n_refs=2, bits=True)
                assert differences(got, want, ('ids', 'count', 'cross', 'occupancy', 'bits')) == [], (level, planes, ctype_mask)
                assert want['count'].max() > 0
                info = ctx.poses_fingerprints_info()
                if level == 'atom' and planes == ALL15:      # few poses, long rows: word slices, integer atomic adds
                    assert info['words'] > 32 and info['slices'] > 1
                if level == 'residue':
                    assert info['slices'] == 1 and info['words'] <= 32
    # residue level meets a residue touched by several ligand atoms in one pose (asserted of the yardstick's input)
    rows = kept_rows(table, ALL15, 0x7F)
    lig, rec = poses.partners(rows)
    key = np.unique(np.stack([poses.pose_of(rows), pc.res_id[rec].astype(np.int64), lig.astype(np.int64)], axis=1), axis=0)
    _, per = np.unique(key[:, :2], axis=0, return_counts=True)
    assert per.max() >= 2
    assert (table['ctype'] != CT['INTER']).any() and (table['ctype'] == CT['INTER']).any()      # the one-type mask drops records
    ctx.close()


@pytest.mark.gpu
def test_contents_against_the_ensemble_route():
    pc, idx, x, h = hem_case()
    params = PARAMS[0]
    X, H = poses.as_models(pc, idx, x, h)
    ens = EnsembleComplex((copy.copy(pc), X, H))
    ens.run_arpeggio(np.asarray(idx), *params)
    m = _mask(pc, idx)
    rows = [poses.reference_rows(ens._results[f]['bags']['atom_atom'], m) for f in range(len(X))]
    ens._ctx.close()
    table = {k: np.concatenate([r[k] for r in rows]).astype(poses.DTYPES[k]) for k in poses.COLUMNS}
    table['pose_off'] = np.concatenate([[0], np.cumsum([len(r['i']) for r in rows])]).astype(np.uint64)
    table['movable'] = np.asarray(idx, np.int32)
    ctx = _ctx(pc, idx)
    ctx.poses_summary(x, h, *params)
    for level in ('residue', 'atom'):
        want = yardstick(table, pc, ALL15, 0x7F, level, n_refs=3)
        got = ctx.poses_fingerprints(ALL15, by_residue=level == 'residue', n_refs=3, bits=True)
        assert differences(got, want, ('ids', 'count', 'cross', 'occupancy', 'bits')) == [], level
    ctx.close()


@pytest.mark.gpu
def test_empty_poses():
    pc, idx, x, h = hem_case()
    x, h = x[:7].copy(), h[:7]
    x[3] += np.float32(100.0)
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x, h, 5.0, 0.1, False)
    got = ctx.poses_fingerprints(ALL15, n_refs=2)
    assert differences(got, yardstick(table, pc, ALL15, n_refs=2)) == []
    assert got['count'][3] == 0 and not got['cross'][3].any() and got['count'][[0, 1, 2, 4, 5, 6]].min() > 0
    # every pose away: no column at all
    far = x + np.float32(100.0)
    table = ctx.poses_contacts(far, h, 5.0, 0.1, False)
    assert len(table['i']) == 0
    for by_residue in (True, False):
        got = ctx.poses_fingerprints(ALL15, by_residue=by_residue, n_refs=2, all_pairs=True, bits=True)
        assert got['ids'].shape == (0,) and got['count'].tolist() == [0] * 7 and got['cross'].tolist() == [[0, 0]] * 7
        assert got['occupancy'].shape == (0, 15) and got['bits'].shape == (7, 15, 0) and not got['inter'].any()
        assert ctx.poses_fingerprints_info()['nodes'] == 0 and fp.tanimoto(got).tolist() == [[1.0, 1.0]] * 7
    ctx.close()


@pytest.mark.gpu
def test_occupancy_leaves_the_references_out_and_chunks_add_up():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    params = (5.0, 0.1, False)
    for level in ('residue', 'atom'):
        table = ctx.poses_contacts(x, h, *params)
        whole = ctx.poses_fingerprints(ALL15, by_residue=level == 'residue', n_refs=2)
        want = yardstick(table, pc, ALL15, level=level, n_refs=2)
        assert differences(whole, want) == []
        with_refs = yardstick(table, pc, ALL15, level=level, n_refs=0)['occupancy']
        assert not np.array_equal(with_refs, want['occupancy']) and (with_refs >= want['occupancy']).all()
        parts = []
        for a, b in ((2, 30), (30, 70)):
            ctx.poses_summary(np.concatenate([x[:2], x[a:b]]), np.concatenate([h[:2], h[a:b]]), *params)
            parts.append(ctx.poses_fingerprints(ALL15, by_residue=level == 'residue', n_refs=2))
        assert differences(fp.merge(parts), whole) == [], level
    ctx.close()


@pytest.mark.gpu
def test_all_pairs():
    pc, idx, x, h = water_case(130)
    ctx = _ctx(pc, idx)
    table = ctx.poses_contacts(x[:65], h[:65], 5.0, 0.1, False)
    for level in ('residue', 'atom'):
        got = ctx.poses_fingerprints(ALL15, by_residue=level == 'residue', n_refs=1, all_pairs=True)
        want = yardstick(table, pc, ALL15, level=level, n_refs=1, all_pairs=True)
        assert differences(got, want, ('ids', 'count', 'cross', 'occupancy', 'inter')) == []
        assert np.array_equal(got['inter'], got['inter'].T) and np.array_equal(np.diagonal(got['inter']), got['count'])
        assert np.array_equal(got['inter'][:, 0], got['cross'][:, 0])
    # the matrix is not there unless asked for
    ctx.poses_fingerprints(ALL15, n_refs=1)
    n = C.c_int64(0)
    inter = np.zeros((65, 65), np.uint32)
    rc = ctx._L.arp_poses_fingerprints_fetch(ctx._h, 0, None, None, None, None, None, inter.ctypes.data_as(C.c_void_p), C.byref(n))
    assert rc == _capi.ARP_E_ARG and 'ARP_POSEFP_ALL_PAIRS' in ctx._L.arp_last_error(ctx._h).decode()
    # beyond the limit of the square launch
    many = np.repeat(x[:1], 4097, axis=0)
    ctx.poses_summary(many, np.repeat(h[:1], 4097, axis=0), 5.0, 0.1, False)
    before = ctx.poses_fingerprints_info()['launches']
    with pytest.raises(_capi.NativeLibraryError, match='4096') as e:
        ctx.poses_fingerprints(ALL15, n_refs=1, all_pairs=True)
    assert e.value.code == _capi.ARP_E_CAPACITY and 'ARP_SIM_MAX_MODELS' in str(e.value)
    assert ctx.poses_fingerprints_info()['launches'] == before
    got = ctx.poses_fingerprints(ALL15, n_refs=1)      # ... which the rectangular product does not have
    assert len(got['count']) == 4097 and (got['count'] == got['count'][0]).all() and (got['cross'][:, 0] == got['count'][0]).all()
    # 4097 equal poses: every feature is in all 4096 poses behind the reference (65 pose tiles: several blocks add into a counter)
    assert int((got['occupancy'] == 4096).sum()) == int(got['count'][0]) > 0 and int((got['occupancy'] != 0).sum()) == int(got['count'][0])
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- GPU: state
def _same_bytes(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bytes(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _resident_poses(ctx):
    """The resident result of poses_contacts, fetched without a launch."""
    info = ctx.poses_info()
    P, k = info['poses'], info['records']
    t = dict(i=np.empty(k, np.int32), j=np.empty(k, np.int32), dist=np.empty(k, np.float32), sift=np.empty(k, np.uint16),
             ctype=np.empty(k, np.uint8), pose_off=np.empty(P + 1, np.uint64), summary=np.empty((P, 16), np.uint32))
    n = C.c_int64(0)
    ctx._check(ctx._L.arp_poses_contacts_fetch(ctx._h, k, _p(t['pose_off']), _p(t['i']), _p(t['j']), _p(t['dist']), _p(t['sift']), _p(t['ctype']),
                                               _p(t['summary']), C.byref(n)), 'arp_poses_contacts_fetch')
    return t


def _resident_pose_planes(ctx):
    """The resident result of poses_planes, fetched without a launch: offsets, ids and first value column of every table."""
    info = ctx.poses_planes_info()
    out = {}
    for t, name in enumerate(poses.PLANE_TABLES):
        k, P = info[name], info['poses']
        vdt = poses.PLANE_COLUMNS[name][3]
        tab = dict(pose_off=np.empty(P + 1, np.uint64), first=np.empty(k, np.int32), second=np.empty(k, np.int32), dist=np.empty(k, vdt),
                   summary=np.empty((P, 16), np.uint32))
        n = C.c_int64(0)
        ctx._check(ctx._L.arp_poses_planes_fetch(ctx._h, t, k, _p(tab['pose_off']), _p(tab['first']), _p(tab['second']), _p(tab['dist']), None, None,
                                                 None, None, None, None, _p(tab['summary']) if t == 0 else None, C.byref(n)), 'arp_poses_planes_fetch')
        if t:
            del tab['summary']
        out[name] = tab
    return out


def _fetch_everything(ctx):
    packed, _ = ctx.fetch_packed()
    bags = {name: {k: np.array(v) for k, v in bag.items()} for name, bag in packed.items()}      # (copies: the buffer is the context's)
    assert sorted(bags) == ['atom_atom', 'atom_plane', 'group_group', 'group_plane', 'plane_plane']
    return bags, ctx.residue_pairs(), _resident_poses(ctx), _resident_pose_planes(ctx)


@pytest.mark.gpu
def test_a_launch_reads_no_bag_and_voids_nothing():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    counts = ctx.run_launch(5.0, 0.1, False)
    assert counts['atom_atom'] > 0 and len(ctx.residue_pairs()['res_a']) > 0
    ctx.set_plane_atoms(pc)
    planes_table = ctx.poses_planes(x[:9])
    assert sum(len(planes_table[name]['ctype']) for name in poses.PLANE_TABLES) > 0
    table = ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    before = _fetch_everything(ctx)
    assert _same_bytes(before[2], {k: table[k] for k in before[2]})
    for by_residue in (True, False):
        got = ctx.poses_fingerprints(ALL15, by_residue=by_residue, n_refs=2, all_pairs=True, bits=True)
        assert got['count'].max() > 0
        assert _same_bytes(_fetch_everything(ctx), before)
    st = ctx.stats()
    assert st['posefp_launches'] == 2 and st['posefp_nodes'] == len(got['ids']) and st['posefp_words'] == 15 * ((len(got['ids']) + 63) // 64)
    ctx.close()


def _fetch_rc(ctx):
    n = C.c_int64(-1)
    count = np.zeros(1 << 13, np.uint32)
    rc = ctx._L.arp_poses_fingerprints_fetch(ctx._h, 0, None, _p(count), None, None, None, None, C.byref(n))
    return rc, ctx._L.arp_last_error(ctx._h).decode()


@pytest.mark.gpu
def test_same_arguments_do_no_work_and_the_result_goes_with_the_poses_result():
    pc, idx, x, h = hem_case()
    m = _mask(pc, idx)
    params = (5.0, 0.1, False)
    ctx = _ctx(pc, idx)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG and 'no result' in _fetch_rc(ctx)[1]
    assert ctx.poses_fingerprints_info() == dict(poses=0, n_refs=0, nodes=0, planes=0, words=0, slices=0, launches=0, flags=0)
    table = ctx.poses_contacts(x[:9], h[:9], *params)
    first = ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    assert ctx.poses_fingerprints_info()['launches'] == 1
    again = ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    assert ctx.poses_fingerprints_info()['launches'] == 1 and _same_bytes(first, again)          # no work the second time
    for kw in (dict(n_refs=1), dict(n_refs=2, by_residue=False), dict(n_refs=2, ctype_mask=1 << CT['INTER']), dict(n_refs=2, all_pairs=True)):
        before = ctx.poses_fingerprints_info()['launches']
        planes = kw.pop('planes', ALL15)
        got = ctx.poses_fingerprints(planes, **kw)
        assert ctx.poses_fingerprints_info()['launches'] == before + 1, kw                        # other arguments remake it
        want = yardstick(table, pc, planes, kw.get('ctype_mask', 0x7F), 'residue' if kw.get('by_residue', True) else 'atom', kw['n_refs'])
        assert differences(got, want) == [], kw
    other = ctx.poses_fingerprints(SCATTERED, n_refs=2)
    assert differences(other, yardstick(table, pc, SCATTERED, n_refs=2)) == [] and ctx.poses_fingerprints_info()['flags'] == _capi.POSEFP_BY_RESIDUE
    back = ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    assert _same_bytes(back, first)
    # a new poses result, a new selection, a new structure: the fetch refuses, the info is empty, the launches stay counted
    launches = ctx.poses_fingerprints_info()['launches']
    assert _fetch_rc(ctx)[0] == _capi.ARP_OK
    ctx.poses_contacts(x[:9], h[:9], *params)                         # the same poses again: still a new result
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG and 'no result' in _fetch_rc(ctx)[1]
    assert ctx.poses_fingerprints_info() == dict(poses=0, n_refs=0, nodes=0, planes=0, words=0, slices=0, launches=launches, flags=0)
    assert _same_bytes(ctx.poses_fingerprints(ALL15, n_refs=2, bits=True), first) and ctx.poses_fingerprints_info()['launches'] == launches + 1
    ctx.set_selection(m)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG
    with pytest.raises(ValueError, match='no poses result'):
        ctx.poses_fingerprints(ALL15)
    ctx.poses_contacts(x[:9], h[:9], *params)
    ctx.poses_fingerprints(ALL15, n_refs=2)
    assert _fetch_rc(ctx)[0] == _capi.ARP_OK
    ctx.set_complex(pc)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG
    ctx.set_selection(m)
    ctx.poses_contacts(x[:9], h[:9], *params)
    ctx.poses_fingerprints(ALL15, n_refs=2)
    ctx.set_topology(pc)
    X, H = poses.as_models(pc, idx, x[:2], h[:2])
    ctx.set_models(X, H)
    assert _fetch_rc(ctx)[0] == _capi.ARP_E_ARG
    ctx.close()


@pytest.mark.gpu
def test_every_refusal_names_its_cause_and_touches_nothing():
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    L, hd = ctx._L, ctx._h
    info = np.zeros(8, np.int64)

    def refused(word, planes=ALL15, ctype_mask=0x7F, flags=1, n_refs=0, code=_capi.ARP_E_ARG):
        rc = L.arp_poses_fingerprints_launch(hd, planes, ctype_mask, flags, n_refs, _p(info))
        msg = L.arp_last_error(hd).decode()
        assert rc == code and word in msg, (word, rc, msg)
    refused('no poses result')
    ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    good = ctx.poses_fingerprints(ALL15, n_refs=2, bits=True)
    launches = ctx.poses_fingerprints_info()['launches']
    refused('planes mask of 0', planes=0)
    refused('beyond the 15 SIFt bits', planes=1 << 15)
    refused('ctype_mask of 0', ctype_mask=0)
    refused('beyond the 7 contact types', ctype_mask=0x80)
    refused('unknown flag', flags=4)
    refused('n_refs', n_refs=-1)
    refused('n_refs', n_refs=10)                                      # more references than poses
    ctx.run_enqueue(5.0, 0.1, False)
    refused('not been waited for')
    ctx.run_wait()
    assert ctx.poses_fingerprints_info()['launches'] == launches and _same_bytes(ctx.poses_fingerprints(ALL15, n_refs=2, bits=True), good)
    assert ctx.poses_fingerprints_info()['launches'] == launches      # ... the resident result is the one it was
    ctx.poses_contacts(np.repeat(x[:1], 70, axis=0), np.repeat(h[:1], 70, axis=0), 5.0, 0.1, False)
    refused('n_refs', n_refs=65)                                      # more than ARP_POSEFP_MAX_REFS
    assert L.arp_poses_fingerprints_launch(hd, ALL15, 0x7F, 1, 64, _p(info)) == _capi.ARP_OK and info[1] == 64
    assert L.arp_poses_fingerprints_launch(None, ALL15, 0x7F, 1, 0, _p(info)) == _capi.ARP_E_ARG
    assert L.arp_poses_fingerprints_launch(hd, ALL15, 0x7F, 1, 0, None) == _capi.ARP_E_ARG
    ctx.close()


@pytest.mark.gpu
def test_null_pointers_capacity_and_a_caller_owned_stream():
    from test_gpu_paths import _hip_runtime
    pc, idx, x, h = hem_case()
    ctx = _ctx(pc, idx)
    ctx.poses_contacts(x[:9], h[:9], 5.0, 0.1, False)
    want = ctx.poses_fingerprints(ALL15, by_residue=False, n_refs=2, bits=True)
    U = len(want['ids'])
    L, hd = ctx._L, ctx._h
    n = C.c_int64(0)
    assert L.arp_poses_fingerprints_fetch(hd, 0, None, None, None, None, None, None, C.byref(n)) == _capi.ARP_OK and n.value == U
    assert L.arp_poses_fingerprints_fetch(hd, 0, None, None, None, None, None, None, None) == _capi.ARP_E_ARG
    for key in ('ids', 'occupancy', 'bits'):                          # what is sized by the columns needs room for them
        buf = np.full(want[key].shape, 7, want[key].dtype)
        args = {k: (_p(buf) if k == key else None) for k in ('ids', 'count', 'cross', 'occupancy', 'bits')}
        n.value = 0
        rc = L.arp_poses_fingerprints_fetch(hd, U - 1, args['ids'], args['count'], args['cross'], args['occupancy'], args['bits'], None, C.byref(n))
        assert rc == _capi.ARP_E_CAPACITY and n.value == U and (buf == 7).all() and 'too small' in L.arp_last_error(hd).decode()
        rc = L.arp_poses_fingerprints_fetch(hd, U, args['ids'], args['count'], args['cross'], args['occupancy'], args['bits'], None, C.byref(n))
        assert rc == _capi.ARP_OK and np.array_equal(buf, want[key]), key      # one array alone
    count, cross = np.zeros(9, np.uint32), np.zeros((9, 2), np.uint32)
    assert L.arp_poses_fingerprints_fetch(hd, 0, None, _p(count), _p(cross), None, None, None, C.byref(n)) == _capi.ARP_OK      # cap is not looked at
    assert np.array_equal(count, want['count']) and np.array_equal(cross, want['cross'])
    hip = _hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx.use_stream(stream.value)
    ctx.poses_summary(x[:9], h[:9], 5.0, 0.1, False)
    got = ctx.poses_fingerprints(ALL15, by_residue=False, n_refs=2, bits=True)
    assert _same_bytes(got, want)
    ctx.use_stream(0)                                                 # (the caller's stream is destroyed only after that)
    ctx.close()
    assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------------------------------------------------- GPU: end to end
@pytest.mark.gpu
def test_run_pose_fingerprints_end_to_end(tmp_path):
    pc, idx, x, h = hem_case()
    params = (5.0, 0.1, False)
    ic = InteractionComplex(copy.copy(pc))
    whole = ic.run_pose_fingerprints(['RESNAME:HEM'], x, h, *params)
    keys = ('ids', 'count', 'cross', 'occupancy', 'reference_count', 'reference_cross')
    chunked = ic.run_pose_fingerprints(np.asarray(idx), x, h, *params, chunk=16)
    assert differences(chunked, whole, keys) == [] and chunked['n_refs'] == 1 and chunked['level'] == 'residue'
    # the yardstick: the home pose in front of the poses
    atoms, rows = poses.movable(pc, idx)
    rx, rh = pc.xyz[atoms][None].astype(np.float32), pc.h_xyz[rows][None]
    table = ic._ctx.poses_contacts(np.concatenate([rx, x]), np.concatenate([rh, h]), *params)
    want = yardstick(table, pc, fp.planes(), level='residue', n_refs=1)
    assert np.array_equal(whole['ids'], want['ids']) and np.array_equal(whole['occupancy'], want['occupancy'])
    assert np.array_equal(whole['count'], want['count'][1:]) and np.array_equal(whole['cross'], want['cross'][1:])
    assert np.array_equal(whole['reference_count'], want['count'][:1]) and whole['count'].shape == (70,)
    # pose 0 of synth.poses_of is the home pose: it recovers the default reference completely
    assert fp.recovery(whole)[0, 0] == 1.0 and fp.tanimoto(whole)[0, 0] == 1.0 and fp.rank(whole)[0] == 0
    assert whole['cross'][0, 0] == whole['count'][0] == whole['reference_count'][0] > 0
    # two references of the caller's, atom level, one kind of entity, named contacts, all pairs
    two = ic.run_pose_fingerprints(['RESNAME:HEM'], x[2:], h[2:], *params, refs_xyz=x[:2], refs_h_xyz=h[:2], contacts=['hbond', 'hydrophobic'],
                                   interacting_entities=['INTER'], level='atom', all_pairs=True)
    table = ic._ctx.poses_contacts(x, h, *params)
    want = yardstick(table, pc, BIT['hbond'] | BIT['hydrophobic'], 1 << CT['INTER'], 'atom', n_refs=2, all_pairs=True)
    assert np.array_equal(two['count'], want['count'][2:]) and np.array_equal(two['cross'], want['cross'][2:]) and np.array_equal(two['inter'], want['inter'][2:, 2:])
    assert np.array_equal(two['reference_cross'], want['cross'][:2]) and np.array_equal(two['occupancy'], want['occupancy'])
    with pytest.raises(ValueError, match='one chunk'):
        ic.run_pose_fingerprints(['RESNAME:HEM'], x, h, *params, chunk=16, all_pairs=True)
    with pytest.raises(ValueError):
        ic.run_pose_fingerprints(['RESNAME:HEM'], x, h, *params, level='chain')
    # the CSV: its first rows from the yardstick's numbers, by hand
    ic.pose_fingerprints = whole
    path = ic.write_pose_fingerprints(str(tmp_path))
    lines = open(path).read().splitlines()
    assert os.path.basename(path) == 'proteinlike.posefp' and len(lines) == 1 + 70 + 1 + len(whole['ids'])
    n0 = int(whole['reference_count'][0])
    assert lines[0] == 'pose,count,shared_0,tanimoto_0,recovery_0' and lines[1] == f'0,{n0},{n0},1.0,1.0'
    c, s = int(whole['count'][1]), int(whole['cross'][1, 0])
    assert lines[2] == f'1,{c},{s},{s / (c + n0 - s)!r},{s / n0!r}'
    assert lines[71] == 'node,' + ','.join(n for n in config.SIFT_NAMES if n != 'proximal')
    r0 = int(whole['ids'][0])
    assert lines[72] == '%s/%d/,' % (pc.res_chain[r0], int(pc.res_seq[r0])) + ','.join(str(int(v)) for v in whole['occupancy'][0])
