"""The per-pose offsets of the ligand-pose results over more poses than one round of the scan holds (arp_runs.h, ``scan_round``:
1024 values a round, a running carry from round to round; k_poses_offsets for the poses and the poses-planes result,
k_psl_offsets for the shortlist).

What the summaries hold is checked against the ensemble route by tests/test_poses.py and tests/test_poses_planes.py, and what a
shortlist holds against the full tables by tests/test_pose_shortlist.py.  Here only the prefix sums: the reference is
``numpy.cumsum`` over fetched per-pose counts (for the shortlist: over the lengths ``pose_shortlist.take`` / ``take_planes`` keep on
the host), never the kernel under test.  The pose counts sit on the seams of the scan — a wave (63, 64, 65), a round (1023,
1024, 1025), more than two rounds (2049).  Exact: uint64 bytes, no tolerance."""
import numpy as np
import pytest

from arpeggio_amd import pose_shortlist as sl, poses, synth
from test_pose_fingerprints import _ctx, water_case
import test_poses_planes as tpp


def _offsets_of(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts).astype(np.uint64), dtype=np.uint64)]).astype(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('P', (1, 63, 64, 65, 1023, 1024, 1025, 2049))
def test_contacts_offsets_are_the_prefix_sums_of_the_summaries_totals(P):
    pc, idx, x, h = water_case(P)
    ctx = _ctx(pc, idx)
    t = ctx.poses_contacts(x, h, 5.0, 0.1, False)
    assert t['pose_off'].dtype == np.uint64 and t['summary'].shape == (P, 16)
    assert _same(t['pose_off'], _offsets_of(t['summary'][:, 15]))
    assert int(t['pose_off'][P]) == len(t['i']) > 0
    ctx.close()


def _ring_case(P):
    """The mid-chain PHE of the small protein (a moved ring, two amides) in P poses."""
    pc, idx, _, _ = tpp.case_phe()
    x, h = synth.poses_of(pc, idx, P, seed=3, shift=4.0, jitter=0.1)
    return pc, idx, x, h


@pytest.mark.gpu
@pytest.mark.parametrize('P', (1024, 1025, 2049))
def test_planes_offsets_are_the_prefix_sums_of_the_four_table_counts(P):
    pc, idx, x, h = _ring_case(P)
    ctx = _ctx(pc, idx)
    ctx.set_plane_atoms(pc)
    t = ctx.poses_planes(x)
    assert t['summary'].shape == (P, 16)
    for k, name in enumerate(poses.PLANE_TABLES):
        assert _same(t[name]['pose_off'], _offsets_of(t['summary'][:, k])), name
        assert int(t[name]['pose_off'][P]) == len(t[name]['ctype']) > 0, name
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('n_ids', (1025, 2049))
def test_shortlist_offsets_of_a_long_list_with_repeats(n_ids):
    pc, idx, x, h = _ring_case(9)
    ctx = _ctx(pc, idx)
    ctx.set_plane_atoms(pc)
    table, ptable = ctx.poses_contacts(x, h, 5.0, 0.1, False), ctx.poses_planes(x)
    ids = np.random.default_rng(n_ids).integers(0, 9, n_ids).astype(np.int32)
    types = sorted(set(table['ctype'].tolist()))
    for ctype_mask in (0x7F, 1 << types[0]):      # (every record kept; a filter that drops some)
        got = ctx.poses_shortlist('list', pose_ids=ids, tables=sl.TABLES, ctype_mask=ctype_mask)
        assert ctx.poses_shortlist_info()['chosen'] == n_ids and got['pose'].tolist() == ids.tolist()
        want = sl.take(table, ids, 0, ctype_mask)
        assert _same(got['pose_off'], want['pose_off']) and int(got['pose_off'][n_ids]) == len(got['i']) > 0
        pwant = sl.take_planes(ptable, ids, ctype_mask)
        for name in poses.PLANE_TABLES:
            assert _same(got[name]['pose_off'], pwant[name]['pose_off']), name
            assert int(got[name]['pose_off'][n_ids]) == len(got[name]['ctype']), name
        assert sum(len(got[name]['ctype']) for name in poses.PLANE_TABLES) > 0
    ctx.close()
