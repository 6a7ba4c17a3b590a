"""The canonical orientation on the MI355X (csrc/nn_samples.hip sm_k_canonicalize through Fitter.canonicalize) against
its definition samples_io.canonicalize_host, and the merge up to symmetry (Fitter.merge_duplicates(symmetries=True))
against samples_io.merge_duplicates_host(symmetries=True): states, policies, outcomes, weights, order and counts, bit
for bit."""
import numpy as np
import pytest

from corintho_ai_amd import nets
from corintho_ai_amd.fit import Fitter, fit_samples
from corintho_ai_amd.samples_io import canonicalize_host, merge_duplicates_host
from tests import fit_ref
from tests import symmetry_cases as SC
from tests.symmetry_cases import same

pytestmark = pytest.mark.gpu


def _held(f):
    """(state_policy, outcome, weights) of the packed set a fitter holds: virtual row 8 i is sample i as it is"""
    n = f.data_info()[1]
    s, e, p = f.fetch_rows(8 * np.arange(n, dtype=np.int32))
    return np.concatenate([s, p], axis=1), e, f.get_sample_weights()


@pytest.fixture(scope="module")
def cases():
    sp, oc = SC.canonical_cases()
    want, k_star = canonicalize_host(sp)
    assert set(k_star.tolist()) == set(range(8))
    return sp, oc, want, k_star


# partial and full four-wave workgroups, and more than one workgroup
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_device_equals_host(cases, n, weighted):
    sp, oc, want, k_star = cases
    first = int(np.flatnonzero(k_star)[0]) if n == 1 else 0  # (one sample: one that moves)
    sp, oc, want, k_star = sp[first:first + n], oc[first:first + n], want[first:first + n], k_star[first:first + n]
    weights = np.random.default_rng(n).uniform(0.0, 3.0, n).astype(np.float32) if weighted else None
    with Fitter(max_batch=16) as f:
        f.add_samples(sp, oc)
        if weighted:
            f.set_sample_weights(weights)
        moved = f.canonicalize()
        assert moved == int(np.count_nonzero(k_star))
        assert moved > 0 or n not in (1, 257)
        assert f.data_info() == (8 * n, n)
        got = _held(f)
        assert same(got[0], want) and same(got[1], oc)
        assert same(got[2], weights if weighted else np.ones(n, np.float32))  # the weights come back unchanged
        assert f.canonicalize() == 0  # a second call moves nothing and changes no byte
        again = _held(f)
        assert all(same(a, b) for a, b in zip(got, again))
        if not weighted:  # the set did not become a weighted one: it takes more samples
            f.add_samples(sp[:1], oc[:1])
            assert f.data_info() == (8 * n + 8, n + 1)


def test_the_cases_hold_what_they_say(cases):
    sp, _, want, k_star = cases
    # -0.0 words, the start position (all eight symmetries fix it: k* = 0), a two-element stabiliser
    assert np.count_nonzero(sp[:, :64].view(np.uint32) == 0x80000000) == 2
    start = np.flatnonzero((sp[:, :70] == SC.start_position()).all(axis=1))
    assert start.size == 1 and k_star[start[0]] == 0
    assert sum(len(SC.stabiliser(row[:70])) == 2 for row in sp) == 3
    # images have one canonical state: at most this many are left (24 images of 3 samples, 3 of one, 2 of one)
    canon = np.unique(np.ascontiguousarray(want[:, :70]).view(np.uint32), axis=0)
    assert 200 < canon.shape[0] <= 257 - 3 * 7 - 2 - 1


@pytest.fixture(scope="module")
def planted():
    """40 samples in 6 orbits, 5 of them exact duplicates of their neighbours"""
    return SC.planted(6, 40, 91, exact=5)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("normalize", [False, True])
def test_merge_up_to_symmetry_equals_host(planted, weighted, normalize):
    sp, oc, orbit_of = planted
    weights = np.random.default_rng(92).uniform(0.0, 3.0, 40).astype(np.float32) if weighted else None
    want = merge_duplicates_host(sp, oc, weights, normalize=normalize, symmetries=True)
    with Fitter(max_batch=64) as f:
        f.add_samples(sp, oc)
        if weighted:
            f.set_sample_weights(weights)
        counts = f.merge_duplicates(normalize=normalize, symmetries=True)
        assert counts == (40, 6) and want[0].shape[0] == 6
        assert f.data_info() == (8 * 6, 6)
        for name, g, w in zip(("state_policy", "outcome", "weights"), _held(f), want):
            assert same(g, w), name


def test_merge_without_the_keyword_is_what_it_was(planted):
    sp, oc, _ = planted
    want = merge_duplicates_host(sp, oc)
    assert 6 < want[0].shape[0] < 40
    with Fitter(max_batch=64) as f:
        f.add_samples(sp, oc)
        assert f.merge_duplicates() == (40, want[0].shape[0])
        for g, w in zip(_held(f), want):
            assert same(g, w)


def test_fit_samples_with_merge_symmetries_equals_the_fit_of_the_host_merge(planted):
    sp, oc, _ = planted
    msp, moc, mw = merge_duplicates_host(sp, oc, symmetries=True)
    w = nets.init_mlp12x100(4, bn_noise=True)
    kw = dict(batch_size=16, epochs=2, seed=5, augmentation="consistent")
    a = fit_samples(w, sp, oc, merge_duplicates=True, merge_symmetries=True, **kw)
    b = fit_samples(w, msp, moc, sample_weight=mw, **kw)
    c = fit_samples(w, sp, oc, merge_duplicates=True, **kw)
    assert a.history == b.history and a.history != c.history
    assert same(a.weights, b.weights) and same(a.best_weights, b.best_weights)


def test_refusals():
    s, z, p = fit_ref.synthetic_samples(24, 51)
    with Fitter(max_batch=16) as f:
        with pytest.raises(Exception, match="no samples"):
            f.canonicalize()  # empty
        with pytest.raises(Exception, match="no samples"):
            f.merge_duplicates(symmetries=True)
        assert f.data_info() == (0, 0)
        f.set_data(s, z, p)
        with pytest.raises(Exception, match="expanded"):
            f.canonicalize()
        assert f.data_info() == (24, 0)
        got = f.fetch_rows(np.arange(24, dtype=np.int32))
        assert same(got[0], s) and same(got[2], p)
