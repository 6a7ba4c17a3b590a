"""The merge of duplicate positions (csrc/nn_samples.hip through Fitter.merge_duplicates) at the sizes where its
launches change, against its definition samples_io.merge_duplicates_host: states, policies, outcomes, weights and
order, bit for bit.  With n samples, SM_TILE = 256 and SM_SCAN = 1024:

  * the radix sort takes ceil(bits / 8) passes, 2^bits >= n: one up to n = 256, two up to 65 536, three from 65 537;
    the pass count is also which of the two key/value buffers the later kernels read;
  * a scan of m entries has ceil(m / 1024) block sums, which sm_k_scan_sums walks 1024 at a time with a carry: the
    histogram scan (m = 256 ceil(n / 256)) needs the carry from n = 4096 * 256 + 1 = 1 048 577, the groups' scan
    (m = n + 1) a second block from n = 1024;
  * sm_k_segment walks a group 64 members at a time, four rows in flight: 63, 64, 65, 127, 128, 129 members are where
    the two loops' ends meet;
  * states are equal when their bits are: +0.0 and -0.0 differ, two NaNs of one word are equal.

The builders of the sets are checked without a device by tests/test_sample_merge_sizes_cpu.py."""
import time

import numpy as np
import pytest

from corintho_ai_amd.fit import Fitter
from corintho_ai_amd.samples_io import merge_duplicates_host
from tests import fit_ref
from tests.test_sample_merge_gpu import _assert_equals_host, _same, _samples_of

pytestmark = pytest.mark.gpu

STATE, ROW = 70, 166
EDGE_SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537]
STRUCTURES = ["distinct", "one-state", "mixed"]
GROUP_LENGTHS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130, 193]
NAN_WORD = 0x7FC00001
CARRY_N = 4096 * 256 + 1  # the smallest n whose histogram scan has more than 1024 block sums


def _index_bits(out):
    """out[i, b] = bit b of i as 0.0 / 1.0 for every bit the largest index needs: n rows, no two alike"""
    n = out.shape[0]
    bits = max(1, int(n - 1).bit_length())
    assert bits <= out.shape[1]
    idx = np.arange(n, dtype=np.int64)
    for b in range(bits):
        out[:, b] = (idx >> b) & 1


def _distinct_states(n):
    s = np.zeros((n, STATE), np.float32)
    _index_bits(s)
    return s


def _weights(n, seed):
    """uniform [0, 3) with exact zeros at up to three samples (never at all of them)"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 3.0, n).astype(np.float32)
    w[rng.choice(n, min(3, n // 2), replace=False)] = 0.0
    return w


def _edge_set(n, structure):
    """(state_policy, outcome) of n samples: all states distinct, all one state, or about n / 3 states drawn with
    repetition and permuted, the first and the last sample of one state"""
    if structure == "distinct":
        states, group_of = _distinct_states(n), np.arange(n)
    elif structure == "one-state":
        states, group_of = _distinct_states(2)[1:], np.zeros(n, np.int64)
    else:
        m = max(1, n // 3)
        rng = np.random.default_rng(1000 + n)
        states, group_of = _distinct_states(m), rng.permutation(rng.integers(0, m, n))
        group_of[n - 1] = group_of[0]
    return _samples_of(states, group_of, 61)


def _group_length_set():
    """912 samples in groups of exactly GROUP_LENGTHS members, interleaved by a fixed permutation"""
    group_of = np.repeat(np.arange(len(GROUP_LENGTHS)), GROUP_LENGTHS)
    group_of = np.random.default_rng(12).permutation(group_of)
    sp, oc = _samples_of(_distinct_states(len(GROUP_LENGTHS)), group_of, 62)
    return sp, oc, group_of


def _bit_equality_set():
    """four samples whose states differ in float 5 alone: +0.0, -0.0, a NaN word, the same NaN word"""
    states = np.repeat(fit_ref.synthetic_samples(1, 63)[0], 4, axis=0)
    states.view(np.uint32)[:, 5] = [0x00000000, 0x80000000, NAN_WORD, NAN_WORD]
    sp, oc = _samples_of(states, np.arange(4), 64)
    assert sp.view(np.uint32)[:, 5].tolist() == [0x00000000, 0x80000000, NAN_WORD, NAN_WORD]
    return sp, oc


def _planted_set(n, mid, seed):
    """n samples whose states are their indices in binary, except that samples mid and n - 1 have the state of
    sample 0 and sample 2 that of sample 1; policies and outcomes of one generator"""
    rng = np.random.default_rng(seed)
    sp = np.zeros((n, ROW), np.float32)
    _index_bits(sp[:, :STATE])
    sp[:, STATE:] = rng.random((n, ROW - STATE), dtype=np.float32)
    oc = rng.integers(-1, 2, n).astype(np.float32)
    sp[[mid, n - 1], :STATE] = sp[0, :STATE]
    sp[2, :STATE] = sp[1, :STATE]
    return sp, oc


def _planted_sources(n, mid):
    """the input row that each row of the merged planted set comes from"""
    return np.delete(np.arange(n), [2, mid, n - 1])


def _planted_expected(sp, oc, mid, src, a, b):
    """rows [a, b) of the unweighted, un-normalised merge of a planted set, from the definition: the input without
    rows 2, mid and n - 1 (src), rows 0 and 1 the merges of their three and two members, weights 3, 2 and ones"""
    n = sp.shape[0]
    want_sp, want_oc = sp[src[a:b]], oc[src[a:b]]
    want_w = np.ones(want_oc.size, np.float32)
    if a == 0:
        for r, members in ((0, [0, mid, n - 1]), (1, [1, 2])):
            m = merge_duplicates_host(sp[members], oc[members], normalize=False)
            assert m[0].shape[0] == 1
            want_sp[r], want_oc[r], want_w[r] = m[0][0], m[1][0], m[2][0]
    return want_sp, want_oc, want_w


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_sizes_at_the_edges(n, structure):
    """one, two and three sort passes (n <= 256, <= 65 536, 65 537), a last sort tile of 255, 256 and 1 keys, one and
    two blocks in the groups' scan (n + 1 <= 1024 or not), and the smallest sets there are"""
    sp, oc = _edge_set(n, structure)
    counts, _ = _assert_equals_host(sp, oc, None, True)
    if structure == "distinct":
        assert counts == (n, n)
    elif structure == "one-state":
        assert counts == (n, 1)
    else:
        assert _same(sp[0, :STATE], sp[n - 1, :STATE]) and counts[1] <= max(1, n // 3)
    _assert_equals_host(sp, oc, _weights(n, 2000 + n), False)


def test_group_lengths_around_the_walk_of_64():
    sp, oc, group_of = _group_length_set()
    n = sum(GROUP_LENGTHS)
    weights = _weights(n, 13)
    for w in (None, weights):
        for normalize in (True, False):
            counts, (_, _, mw) = _assert_equals_host(sp, oc, w, normalize)
            assert counts == (n, len(GROUP_LENGTHS))
            if w is None and not normalize:
                firsts = [int(np.flatnonzero(group_of == g)[0]) for g in range(len(GROUP_LENGTHS))]
                assert mw.tolist() == [float(GROUP_LENGTHS[g]) for g in np.argsort(firsts)]


def test_equality_is_of_bits():
    sp, oc = _bit_equality_set()
    for w in (None, np.array([0.5, 1.5, 2.0, 0.25], np.float32)):
        counts, (msp, _, mw) = _assert_equals_host(sp, oc, w, False)
        assert counts == (4, 3)  # the zeros stay apart, the NaNs merge
        assert msp.view(np.uint32)[:, 5].tolist() == [0x00000000, 0x80000000, NAN_WORD]
        assert mw.tolist() == ([1.0, 1.0, 2.0] if w is None else [0.5, 1.5, 2.25])


def test_the_scan_carries_across_chunks_of_block_sums():
    """n = 1 048 577: 4097 sort tiles, so the histogram scan has 1025 block sums and sm_k_scan_sums a second chunk
    (and the sort three passes).  Every row is compared: a wrong carry misplaces rows far from the planted groups."""
    n, mid = CARRY_N, 524288
    assert (256 * ((n + 255) // 256) + 1023) // 1024 == 1025 and (256 * ((n - 1 + 255) // 256) + 1023) // 1024 == 1024
    t0 = time.perf_counter()
    sp, oc = _planted_set(n, mid, 65)
    src = _planted_sources(n, mid)
    t1 = time.perf_counter()
    with Fitter(max_batch=16384) as f:
        f.add_samples(sp, oc)
        assert f.merge_duplicates(normalize=False) == (n, n - 3)
        assert f.data_info() == (8 * (n - 3), n - 3)
        t2 = time.perf_counter()
        got_w = f.get_sample_weights()
        for a in range(0, n - 3, 65536):
            b = min(n - 3, a + 65536)
            s, e, p = f.fetch_rows(8 * np.arange(a, b, dtype=np.int32))
            want_sp, want_oc, want_w = _planted_expected(sp, oc, mid, src, a, b)
            assert _same(s, want_sp[:, :STATE]), ("states", a)
            assert _same(p, want_sp[:, STATE:]), ("policies", a)
            assert _same(e, want_oc), ("outcomes", a)
            assert _same(got_w[a:b], want_w), ("weights", a)
        assert got_w[:3].tolist() == [3.0, 2.0, 1.0]
    t3 = time.perf_counter()
    print("n = %d: build %.2f s, upload and merge %.2f s, fetch and compare %.2f s" % (n, t1 - t0, t2 - t1, t3 - t2))
