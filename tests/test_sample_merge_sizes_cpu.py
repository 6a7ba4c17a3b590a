"""The sets that tests/test_sample_merge_sizes_gpu.py merges on the device are reference code themselves: their builders
and the expected result that its largest case states directly are checked here, without a device, against
samples_io.merge_duplicates_host."""
import numpy as np

from corintho_ai_amd.samples_io import merge_duplicates_host
from tests import test_sample_merge_sizes_gpu as M


def _groups(states):
    return np.unique(np.ascontiguousarray(states).view(np.dtype((np.void, 4 * M.STATE))).ravel()).shape[0]


def test_distinct_states_are_distinct():
    for n in M.EDGE_SIZES + [5001]:
        s = M._distinct_states(n)
        assert s.dtype == np.float32 and s.shape == (n, M.STATE)
        assert np.unique(s, axis=0).shape[0] == n and _groups(s) == n
        assert np.isin(s, (0.0, 1.0)).all()


def test_index_bits_of_the_largest_set():
    """all 1 048 577 rows differ, by the 21 columns that hold the index (read back as an integer)"""
    n = M.CARRY_N
    s = np.zeros((n, 21), np.float32)
    M._index_bits(s)
    back = (s.astype(np.int64) << np.arange(21)).sum(1)
    assert np.array_equal(back, np.arange(n))


def test_edge_sets_have_their_structure():
    for n in (1, 2, 257, 1025):
        sp, oc = M._edge_set(n, "distinct")
        assert sp.shape == (n, M.ROW) and oc.shape == (n,) and _groups(sp[:, :M.STATE]) == n
        sp, _ = M._edge_set(n, "one-state")
        assert _groups(sp[:, :M.STATE]) == 1
        sp, _ = M._edge_set(n, "mixed")
        g = _groups(sp[:, :M.STATE])
        assert 1 <= g <= max(1, n // 3) and sp[0, :M.STATE].tobytes() == sp[n - 1, :M.STATE].tobytes()
        if n >= 257:
            assert 1 < g < n
    w = M._weights(1025, 5)
    assert w.dtype == np.float32 and np.sum(w == 0) == 3 and w.min() >= 0 and w.max() < 3
    assert np.sum(M._weights(1, 5) == 0) == 0 and np.sum(M._weights(2, 5) == 0) == 1


def test_group_length_set_has_the_stated_sizes():
    sp, oc, group_of = M._group_length_set()
    assert sp.shape[0] == sum(M.GROUP_LENGTHS) == 912
    assert np.bincount(group_of).tolist() == M.GROUP_LENGTHS
    _, inverse, counts = np.unique(sp[:, :M.STATE], axis=0, return_inverse=True, return_counts=True)
    assert sorted(counts.tolist()) == sorted(M.GROUP_LENGTHS)
    # samples are of one state exactly where they are of one group, and the groups are interleaved
    inverse = np.asarray(inverse).ravel()
    assert all(np.unique(inverse[group_of == g]).size == 1 for g in range(len(M.GROUP_LENGTHS)))
    assert np.count_nonzero(np.diff(group_of)) > 600
    w = merge_duplicates_host(sp, oc, normalize=False)[2]
    firsts = [int(np.flatnonzero(group_of == g)[0]) for g in range(len(M.GROUP_LENGTHS))]
    assert w.tolist() == [float(M.GROUP_LENGTHS[g]) for g in np.argsort(firsts)]


def test_bit_equality_set_has_three_groups_on_the_host():
    sp, oc = M._bit_equality_set()
    words = sp.view(np.uint32)[:, 5]
    assert words.tolist() == [0x00000000, 0x80000000, M.NAN_WORD, M.NAN_WORD]
    assert sp[0, 5] == sp[1, 5] and sp[2, 5] != sp[3, 5]  # as floats it is the other way round
    others = np.delete(sp[:, :M.STATE], 5, axis=1)
    assert (others == others[0]).all()
    msp, moc, mw = merge_duplicates_host(sp, oc, normalize=False)
    assert msp.shape[0] == 3 and mw.tolist() == [1.0, 1.0, 2.0]
    assert msp.view(np.uint32)[:, 5].tolist() == [0x00000000, 0x80000000, M.NAN_WORD]


def test_planted_set_merges_as_stated():
    """the expected result of the 1 048 577-sample case, at n = 5001 where the definition can run on the whole set"""
    n, mid = 5001, 2500
    sp, oc = M._planted_set(n, mid, 65)
    assert _groups(sp[:, :M.STATE]) == n - 3
    src = M._planted_sources(n, mid)
    want = merge_duplicates_host(sp, oc, normalize=False)
    assert want[0].shape[0] == n - 3 == src.size
    parts = [M._planted_expected(sp, oc, mid, src, a, min(n - 3, a + 1024)) for a in range(0, n - 3, 1024)]
    for k, name in enumerate(("state_policy", "outcome", "weights")):
        got = np.concatenate([p[k] for p in parts])
        assert got.dtype == want[k].dtype and got.shape == want[k].shape and got.tobytes() == want[k].tobytes(), name
    assert want[2][:3].tolist() == [3.0, 2.0, 1.0]
    # the size of the device test: the smallest whose histogram scan has 1025 block sums
    assert M.CARRY_N == 1048577 and (256 * ((M.CARRY_N + 255) // 256) + 1023) // 1024 == 1025
