"""Host logic of the packed road (corintho_ai_amd.fit fit_resident, fit_samples, fit_trainer) without a GPU: a
restatement backend that speaks the packed protocol and expands on the host must give what fit() gives on the expanded
arrays, and fit() itself must still need nothing but set_data."""
import numpy as np
import pytest

from corintho_ai_amd import expand_samples, nets
from corintho_ai_amd.fit import fit, fit_resident, fit_samples, fit_trainer
from tests import fit_ref as R
from tests import fit_ref_step as S
from tests.emu import emulib


class PackedRefBackend(S.RefBackend):
    """RefBackend with the packed protocol: the samples are kept un-augmented and expanded by ca_expand_samples"""

    def __init__(self):
        super().__init__("mlp12x100")
        self.calls = []
        self.clear_data()

    def clear_data(self):
        self.calls.append("clear_data")
        self.sp, self.oc = np.zeros((0, 166), np.float32), np.zeros(0, np.float32)
        self.data = None

    def add_samples(self, sp, oc):
        self.calls.append("add_samples")
        self.sp, self.oc = np.concatenate([self.sp, sp]), np.concatenate([self.oc, oc])
        self.data = expand_samples(self.sp, self.oc, _cdll=emulib.load())

    def data_info(self):
        return 8 * self.sp.shape[0], self.sp.shape[0]


class PlainBackend(S.RefBackend):
    """what tests/test_fit_cpu.py drives fit() with; any other method fit() reached for would be missing"""

    def __getattr__(self, name):
        raise AssertionError("fit() called %s on its backend" % name)


@pytest.fixture(scope="module")
def samples():
    s, z, p = R.synthetic_samples(64, 17)
    return np.concatenate([s, p], axis=1).astype(np.float32), z


KW = dict(batch_size=128, epochs=3, seed=6, learning_rate=1e-3)


def _same_fit(a, b):
    assert a.history == b.history
    assert a.best_epoch == b.best_epoch
    assert a.weights.tobytes() == b.weights.tobytes()
    assert a.best_weights.tobytes() == b.best_weights.tobytes()
    assert a.optimizer[2] == b.optimizer[2]


@pytest.fixture(scope="module")
def expanded_fit(samples):
    sp, oc = samples
    be = PlainBackend("mlp12x100")
    res = fit(nets.init_mlp12x100(1), *expand_samples(sp, oc, _cdll=emulib.load()), _backend=be, **KW)
    return res, be


def test_fit_needs_only_set_data(expanded_fit):
    res, be = expanded_fit
    assert len(res.history["loss"]) == 3
    assert len(be.trained_rows) == 3 and be.trained_rows[0].size == 358  # floor(512 * 0.7)


def test_fit_samples_is_fit_on_the_expansion(samples, expanded_fit):
    sp, oc = samples
    be = PackedRefBackend()
    res = fit_samples(nets.init_mlp12x100(1), sp, oc, _backend=be, **KW)
    _same_fit(res, expanded_fit[0])
    assert be.calls == ["clear_data", "clear_data", "add_samples"]  # the constructor's, then fit_samples'
    for a, b in zip(be.trained_rows, expanded_fit[1].trained_rows):
        assert np.array_equal(a, b)


def test_fit_resident_takes_n_from_the_backend(samples, expanded_fit):
    sp, oc = samples
    be = PackedRefBackend()
    be.add_samples(sp[:40], oc[:40])
    be.add_samples(sp[40:], oc[40:])
    assert be.data_info() == (512, 64)
    _same_fit(fit_resident(be, nets.init_mlp12x100(1), **KW), expanded_fit[0])


def test_argument_validation(samples):
    sp, oc = samples
    w = nets.init_mlp12x100(1)
    be = PackedRefBackend()
    with pytest.raises(ValueError, match="state_policy"):
        fit_samples(w, sp[:, :165], oc, _backend=be)
    with pytest.raises(ValueError, match="state_policy"):
        fit_samples(w, sp.ravel(), oc, _backend=be)
    with pytest.raises(ValueError, match="outcome"):
        fit_samples(w, sp, oc[:-1], _backend=be)
    with pytest.raises(ValueError, match="no trainer"):
        fit_trainer(w, [], _backend=be)
    with pytest.raises(ValueError, match="weights"):
        fit_samples(w[:-1], sp, oc, _backend=be)
    with pytest.raises(ValueError, match="batch_size"):
        fit_samples(w, sp, oc, batch_size=0, _backend=be)
    with pytest.raises(ValueError, match="no training or no validation"):
        fit_resident(PackedRefBackend(), w)
