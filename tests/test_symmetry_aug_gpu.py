"""The augmentation choice of a packed set on the MI355X (csrc/nn_train_data.hip ft_k_assemble_consistent through
Fitter.set_augmentation): the 8 n virtual rows against samples_io.expand_host, and a fit from packed samples against the
fit of the host expansion -- bytes in every comparison."""
import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, nets
from corintho_ai_amd.fit import Fitter, fit, fit_samples, net_info
from corintho_ai_amd.samples_io import expand_host
from tests import fit_ref, fit_ref_rescnn4
from tests.symmetry_cases import same

pytestmark = pytest.mark.gpu

NET_CASES = [(NET_MLP12X100, nets.init_mlp12x100, fit_ref), (NET_RESCNN4, nets.init_rescnn4, fit_ref_rescnn4)]
NETS = pytest.mark.parametrize("kind,init,ref", NET_CASES, ids=[net_info(c[0])[0] for c in NET_CASES])


def _same3(got, want):
    return all(same(g, w) for g, w in zip(got, want))


def _distinct(n):
    """n samples whose every cell is distinct and exact in float32: one wrong table entry shows"""
    sp = (256.0 * np.arange(n)[:, None] + np.arange(166)[None, :]).astype(np.float32)
    return sp, (np.arange(n) - 2).astype(np.float32)


@pytest.mark.parametrize("n", [1, 5, 33])  # 33: a batch of 8 n rows of 166 floats is no multiple of the 256 threads
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_virtual_rows_equal_expand_host(n, weighted):
    sp, oc = _distinct(n)
    ref, con = expand_host(sp, oc, "reference"), expand_host(sp, oc, "consistent")
    assert not same(ref[2], con[2])
    natural = np.arange(8 * n, dtype=np.int32)
    permuted = np.random.default_rng(n).permutation(8 * n).astype(np.int32)
    with Fitter(max_batch=8 * n) as f:
        assert f.get_augmentation() == "reference"
        f.add_samples(sp, oc)
        if weighted:
            sw = np.random.default_rng(3).uniform(0.0, 2.0, n).astype(np.float32)
            f.set_sample_weights(sw)
        assert _same3(f.fetch_rows(natural), ref)
        f.set_augmentation("consistent")
        assert f.get_augmentation() == "consistent"
        for rows in (natural, permuted):
            assert _same3(f.fetch_rows(rows), tuple(a[rows] for a in con)), rows
        if weighted:
            assert same(f.get_sample_weights(), sw)
        f.set_augmentation("reference")
        assert f.get_augmentation() == "reference"
        for rows in (natural, permuted):
            assert _same3(f.fetch_rows(rows), tuple(a[rows] for a in ref)), rows


def test_the_setting_belongs_to_the_fitter_and_leaves_an_expanded_set_alone():
    sp, oc = _distinct(5)
    ref, con = expand_host(sp, oc, "reference"), expand_host(sp, oc, "consistent")
    rows = np.arange(40, dtype=np.int32)
    with Fitter(max_batch=16) as f:
        f.set_augmentation("consistent")  # before there is any data
        f.add_samples(sp, oc)
        assert _same3(f.fetch_rows(rows), con)
        f.clear_data()
        assert f.get_augmentation() == "consistent"  # it stays until set again
        f.add_samples(sp, oc)
        assert _same3(f.fetch_rows(rows), con)
        f.set_data(*ref)  # an expanded set: the rows are the caller's
        assert _same3(f.fetch_rows(rows), ref)
        with pytest.raises(ValueError):
            f.set_augmentation("mirror")
        rc = f._L.ca_fitter_set_augmentation(f._h, 2)  # a bad value at the C ABI: CA_ERR_ARG, nothing changes
        assert rc != 0 and b"augmentation" in f._L.ca_last_error()
        assert f._L.ca_fitter_set_augmentation(f._h, -1) != 0
        assert f.get_augmentation() == "consistent"


@NETS
def test_fit_samples_consistent_equals_the_fit_of_the_host_expansion(kind, init, ref):
    s, z, p = ref.synthetic_samples(64, 23)
    sp = np.concatenate([s, p], axis=1).astype(np.float32)
    w = init(5, bn_noise=True)
    kw = dict(batch_size=64, epochs=2, seed=7, net=kind)
    a = fit_samples(w, sp, z, augmentation="consistent", **kw)
    b = fit(w, *expand_host(sp, z, "consistent"), **kw)
    c = fit_samples(w, sp, z, **kw)
    assert a.history == b.history and a.history != c.history
    assert same(a.weights, b.weights) and same(a.best_weights, b.best_weights) and not same(a.weights, c.weights)
    for x, y in zip(a.optimizer[:2] + a.best_optimizer[:2], b.optimizer[:2] + b.best_optimizer[:2]):
        assert same(x, y)
    assert a.optimizer[2] == b.optimizer[2] and a.best_epoch == b.best_epoch
    d = fit(w, *expand_host(sp, z, "reference"), **kw)  # the default is the reference's, as before
    assert c.history == d.history and same(c.weights, d.weights)


def test_the_call_decides_and_fit_resident_leaves_the_setting():
    from corintho_ai_amd.fit import fit_resident
    s, z, p = fit_ref.synthetic_samples(64, 23)
    sp = np.concatenate([s, p], axis=1).astype(np.float32)
    w = nets.init_mlp12x100(5, bn_noise=True)
    kw = dict(batch_size=64, epochs=1, seed=7)
    with Fitter(max_batch=64) as f:
        f.set_augmentation("consistent")
        a = fit_samples(w, sp, z, _backend=f, **kw)  # the call asks for the reference's
        assert f.get_augmentation() == "reference"
        b = fit_samples(w, sp, z, augmentation="consistent", _backend=f, **kw)
        assert f.get_augmentation() == "consistent"
        c = fit_resident(f, w, **kw)
        assert f.get_augmentation() == "consistent"
    assert same(b.weights, c.weights) and not same(a.weights, b.weights)
    assert same(a.weights, fit_samples(w, sp, z, **kw).weights)
