"""Merging the duplicate positions of a packed set on the MI355X (csrc/nn_samples.hip through Fitter.merge_duplicates)
against its definition in plain numpy, samples_io.merge_duplicates_host: states, policies, outcomes, weights and order,
bit for bit."""
import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, Trainer, nets
from corintho_ai_amd.fit import Fitter, fit_samples
from corintho_ai_amd.samples_io import merge_duplicates_host
from tests import fit_ref

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _held(f):
    """(state_policy, outcome, weights) of the packed set a fitter holds: virtual row 8 i is sample i as it is"""
    n = f.data_info()[1]
    s, e, p = f.fetch_rows(8 * np.arange(n, dtype=np.int32))
    return np.concatenate([s, p], axis=1), e, f.get_sample_weights()


def _merged_on_device(sp, oc, weights, normalize):
    with Fitter(max_batch=64) as f:
        f.add_samples(sp, oc)
        if weights is not None:
            f.set_sample_weights(weights)
        counts = f.merge_duplicates(normalize=normalize)
        assert f.data_info() == (8 * counts[1], counts[1])
        return counts, _held(f)


def _assert_equals_host(sp, oc, weights, normalize):
    counts, got = _merged_on_device(sp, oc, weights, normalize)
    want = merge_duplicates_host(sp, oc, weights, normalize=normalize)
    assert counts == (sp.shape[0], want[0].shape[0])
    for name, g, w in zip(("state_policy", "outcome", "weights"), got, want):
        assert _same(g, w), (name, normalize)
    return counts, got


def _samples_of(states, group_of, seed):
    """samples whose states are states[group_of[i]], with policies and outcomes of their own"""
    _, z, p = fit_ref.synthetic_samples(len(group_of), seed)
    return np.concatenate([states[group_of], p], axis=1).astype(np.float32), z


def _hand_built():
    """40 samples in 13 groups: group 0 is the first and the last sample, group 1 has 9 members, group 2 is a
    singleton, groups 3 and 4 differ only in float 0, groups 5 and 6 only in float 69"""
    states = fit_ref.synthetic_samples(13, 31)[0]
    states[4] = states[3]
    states[4, 0] = 1.0 - states[3, 0]
    states[6] = states[5]
    states[6, 69] = states[5, 69] + 0.25
    assert np.unique(states, axis=0).shape[0] == 13
    sizes = [2, 9, 1, 3, 2, 2, 4, 1, 2, 3, 4, 5, 2]
    assert sum(sizes) == 40
    middle = np.repeat(np.arange(1, 13), sizes[1:])
    group_of = np.concatenate([[0], np.random.default_rng(6).permutation(middle), [0]])
    sp, oc = _samples_of(states, group_of, 32)
    return sp, oc, group_of


def test_forty_hand_built_samples():
    sp, oc, group_of = _hand_built()
    rng = np.random.default_rng(7)
    prior = np.ones(40, np.float32)
    some = rng.choice(40, 15, replace=False)
    prior[some] = rng.uniform(0.0, 3.0, 15).astype(np.float32)
    zero_in_nine = np.flatnonzero(group_of == 1)[2]
    prior[zero_in_nine] = 0.0  # a member of weight 0 in a group that stays
    for weights in (None, prior):
        for normalize in (True, False):
            counts, (msp, moc, mw) = _assert_equals_host(sp, oc, weights, normalize)
            assert counts == (40, 13)
            # the order of the first members; the first and the last sample are one group at rank 0
            firsts = [int(np.flatnonzero(group_of == g)[0]) for g in range(13)]
            assert _same(msp[:, :70], sp[sorted(firsts), :70])
            assert _same(msp[0, :70], sp[0, :70]) and _same(msp[0, :70], sp[39, :70])
            if weights is None and not normalize:
                order = np.argsort(firsts)
                assert mw.tolist() == [float(np.sum(group_of == g)) for g in order]
    # a group whose weights are all 0 leaves, members and all
    gone = prior.copy()
    gone[group_of == 2] = 0.0
    gone[group_of == 5] = 0.0
    counts, (msp, _, mw) = _assert_equals_host(sp, oc, gone, True)
    assert counts == (40, 11) and np.all(mw > 0)
    assert not any(_same(row[:70], sp[np.flatnonzero(group_of == 2)[0], :70]) for row in msp)


@pytest.fixture(scope="module")
def six_thousand():
    """6 000 samples drawn from 700 states, 2 500 of them from one: several sort tiles a pass, two passes, a long
    segment, and chains in the table"""
    states = fit_ref.synthetic_samples(700, 41)[0]
    assert np.unique(states, axis=0).shape[0] == 700
    rng = np.random.default_rng(8)
    group_of = np.concatenate([np.zeros(2500, np.int64), np.arange(1, 700), rng.integers(1, 700, 6000 - 2500 - 699)])
    group_of = rng.permutation(group_of)
    return _samples_of(states, group_of, 42) + (group_of,)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_six_thousand_samples_of_700_states(six_thousand, weighted):
    sp, oc, group_of = six_thousand
    weights = np.random.default_rng(9).uniform(0.0, 3.0, 6000).astype(np.float32) if weighted else None
    counts, (msp, moc, mw) = _assert_equals_host(sp, oc, weights, True)
    assert counts == (6000, 700)
    assert abs(float(np.mean(mw.astype(np.float64))) - 1.0) < 1e-6
    if not weighted:
        big = np.flatnonzero((msp[:, :70] == sp[np.flatnonzero(group_of == 0)[0], :70]).all(1))
        assert big.size == 1 and mw[big[0]] == np.float32(np.float64(2500) * (np.float64(700) / np.float64(6000)))


def test_a_second_merge_changes_no_byte(six_thousand):
    sp, oc, _ = six_thousand
    with Fitter(max_batch=64) as f:
        f.add_samples(sp, oc)
        assert f.merge_duplicates(normalize=True) == (6000, 700)
        first = _held(f)
        assert f.merge_duplicates(normalize=False) == (700, 700)
        second = _held(f)
        for a, b in zip(first, second):
            assert _same(a, b)
        # normalising weights whose mean is one already moves them by a rounding at the most; the samples stay
        assert f.merge_duplicates(normalize=True) == (700, 700)
        third = _held(f)
        assert _same(third[0], first[0]) and _same(third[1], first[1])
        np.testing.assert_allclose(third[2], first[2], rtol=3e-7, atol=0)
        want = merge_duplicates_host(*first, normalize=True)
        assert _same(third[2], want[2])


@pytest.fixture(scope="module")
def generation():
    """the un-augmented samples of a 64-game, 50-search fused generation, and the finished trainer"""
    t = Trainer(64, "", 21, 50, 16, 1.0, 0.25, 0, 1, False, stagger=False)
    t.set_net(NET_MLP12X100, nets.init_mlp12x100(3))
    assert t.run()
    sp, oc = t.export_samples()
    yield sp, oc, t
    t.close()


def test_samples_of_a_generation(generation):
    sp, oc, trainer = generation
    want = merge_duplicates_host(sp, oc)
    with Fitter(max_batch=64) as f:
        assert f.add_trainer_samples(trainer) == sp.shape[0]
        before, after = f.merge_duplicates()
        got = _held(f)
    print("a generation of 64 games: %d samples, %d distinct positions" % (before, after))
    assert before == sp.shape[0] and after == want[0].shape[0] and after < before
    for g, w in zip(got, want):
        assert _same(g, w)


def test_fit_samples_with_merge_equals_the_fit_of_the_host_merge(generation):
    sp, oc, _ = generation
    msp, moc, mw = merge_duplicates_host(sp, oc)
    w = nets.init_mlp12x100(4, bn_noise=True)
    a = fit_samples(w, sp, oc, merge_duplicates=True, batch_size=256, epochs=2, seed=5)
    b = fit_samples(w, msp, moc, sample_weight=mw, batch_size=256, epochs=2, seed=5)
    c = fit_samples(w, sp, oc, batch_size=256, epochs=2, seed=5)
    assert a.history == b.history and a.history != c.history
    assert _same(a.weights, b.weights) and _same(a.best_weights, b.best_weights) and not _same(a.weights, w)
    for x, y in zip(a.optimizer[:2] + a.best_optimizer[:2], b.optimizer[:2] + b.best_optimizer[:2]):
        assert _same(x, y)
    assert a.optimizer[2] == b.optimizer[2] and a.best_epoch == b.best_epoch


def test_refusals_leave_the_set_as_it_was():
    s, z, p = fit_ref.synthetic_samples(24, 51)
    sp = np.concatenate([s, p], axis=1).astype(np.float32)
    with Fitter(max_batch=16) as f:
        with pytest.raises(Exception):
            f.merge_duplicates()  # empty
        assert f.data_info() == (0, 0)
        f.set_data(s, z, p)
        with pytest.raises(Exception, match="expanded"):
            f.merge_duplicates()
        assert f.data_info() == (24, 0)
        f.clear_data()
        f.add_samples(sp, z)
        assert f.merge_duplicates() == (24, 24)
        held = _held(f)
        with pytest.raises(Exception, match="clear_data first"):
            f.add_samples(sp, z)
        assert f.data_info() == (192, 24)
        for a, b in zip(held, _held(f)):
            assert _same(a, b)
        f.clear_data()
        f.add_samples(sp, z)  # after clear_data the set takes samples again, and carries no weights
        assert f.data_info() == (192, 24) and _same(f.get_sample_weights(), np.ones(24, np.float32))
