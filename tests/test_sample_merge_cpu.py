"""Merging duplicate positions without a GPU: the properties of its definition in numpy
(samples_io.merge_duplicates_host), and the run driver's flag -- read from TOML and from the command line, and one call
of the fitter's merge_duplicates after the last samples are added and before the fit (a recording fitter on the
emulation build, as tests/test_run_cpu.py)."""
import numpy as np
import pytest

from corintho_ai_amd import RunParams
from corintho_ai_amd import run as R
from corintho_ai_amd.samples_io import merge_duplicates_host
from tests import fit_ref
from tests.test_run_cpu import StubFitter, open_run, small


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def samples():
    """500 samples of 60 states (every state at least once), with weights in [0, 3]"""
    states = fit_ref.synthetic_samples(60, 1)[0]
    assert np.unique(states, axis=0).shape[0] == 60
    rng = np.random.default_rng(2)
    group_of = rng.permutation(np.concatenate([np.arange(60), rng.integers(0, 60, 440)]))
    _, z, p = fit_ref.synthetic_samples(500, 3)
    sp = np.concatenate([states[group_of], p], axis=1).astype(np.float32)
    return sp, z, rng.uniform(0.0, 3.0, 500).astype(np.float32), group_of


@pytest.mark.parametrize("weighted", [False, True])
def test_the_weight_is_conserved_and_normalised(samples, weighted):
    sp, oc, w, group_of = samples
    w = w if weighted else None
    total = float(np.sum(w, dtype=np.float64)) if weighted else 500.0
    msp, moc, mw = merge_duplicates_host(sp, oc, w, normalize=False)
    assert msp.shape == (60, 166) and moc.shape == (60,) and mw.shape == (60,)
    assert msp.dtype == moc.dtype == mw.dtype == np.float32
    assert abs(float(np.sum(mw, dtype=np.float64)) - total) <= 60 * 2.0 ** -24 * total  # one rounding a group
    if not weighted:
        assert mw.tolist() == [float(np.sum(group_of == g)) for g in group_of[np.sort(np.unique(group_of, return_index=True)[1])]]
    nsp, noc, nw = merge_duplicates_host(sp, oc, w, normalize=True)
    assert _same(nsp, msp) and _same(noc, moc)
    assert abs(float(np.mean(nw, dtype=np.float64)) - 1.0) < 1e-6
    np.testing.assert_allclose(nw, mw * (60 / total), rtol=3e-7)


def test_the_means_are_weighted_means(samples):
    sp, oc, w, group_of = samples
    msp, moc, mw = merge_duplicates_host(sp, oc, w, normalize=False)
    # policy rows still sum to what they summed to (1, within float32's rounding of 96 entries)
    assert np.all(np.abs(msp[:, 70:].sum(1, dtype=np.float64) - 1.0) < 1e-5)
    first = np.sort(np.unique(group_of, return_index=True)[1])
    for rank in (0, 17, 59):
        members = np.flatnonzero(group_of == group_of[first[rank]])
        ww = w[members].astype(np.float64)
        want = (sp[members, 70:].astype(np.float64) * ww[:, None]).sum(0) / ww.sum()
        np.testing.assert_allclose(msp[rank, 70:], want, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(moc[rank], (oc[members] * ww).sum() / ww.sum(), rtol=1e-6, atol=1e-7)
        assert _same(msp[rank, :70], sp[first[rank], :70])


def test_the_order_is_that_of_the_first_members(samples):
    sp, oc, w, group_of = samples
    msp = merge_duplicates_host(sp, oc)[0]
    first = np.sort(np.unique(group_of, return_index=True)[1])
    assert _same(msp[:, :70], sp[first, :70])


def test_states_are_compared_by_their_bits():
    sp = np.zeros((4, 166), np.float32)
    sp[:, 70] = 1.0
    sp[1, 3] = -0.0  # equal to 0.0 as a number, another bit pattern
    sp[3, 3] = -0.0
    msp, moc, mw = merge_duplicates_host(sp, np.array([1, 0, -1, 1], np.float32), normalize=False)
    assert msp.shape[0] == 2 and mw.tolist() == [2.0, 2.0] and moc.tolist() == [0.0, 0.5]
    assert np.signbit(msp[1, 3]) and not np.signbit(msp[0, 3])


def test_a_group_of_weight_zero_is_dropped(samples):
    sp, oc, w, group_of = samples
    w = w.copy()
    w[group_of == group_of[0]] = 0.0
    msp, moc, mw = merge_duplicates_host(sp, oc, w)
    assert msp.shape[0] == 59 and np.all(mw > 0)
    assert not (msp[:, :70] == sp[0, :70]).all(1).any()


@pytest.mark.parametrize("weighted", [False, True])
def test_merging_twice_is_merging_once(samples, weighted):
    sp, oc, w, _ = samples
    once = merge_duplicates_host(sp, oc, w if weighted else None, normalize=False)
    twice = merge_duplicates_host(*once, normalize=False)
    for a, b in zip(once, twice):
        assert _same(a, b)
    # normalised weights have mean one to a rounding, so a second normalisation moves them by a rounding at the most
    once = merge_duplicates_host(sp, oc, w if weighted else None, normalize=True)
    twice = merge_duplicates_host(*once, normalize=True)
    assert _same(once[0], twice[0]) and _same(once[1], twice[1])
    np.testing.assert_allclose(twice[2], once[2], rtol=3e-7)


def test_bad_arguments_are_refused(samples):
    sp, oc, w, _ = samples
    for bad in (w[:10], np.where(np.arange(500) == 3, -1.0, w), np.where(np.arange(500) == 3, np.nan, w)):
        with pytest.raises(ValueError):
            merge_duplicates_host(sp, oc, bad)
    with pytest.raises(ValueError):
        merge_duplicates_host(sp[:, :100], oc)
    empty = merge_duplicates_host(np.zeros((0, 166), np.float32), np.zeros(0, np.float32))
    assert [a.shape for a in empty] == [(0, 166), (0,), (0,)]


# ---------------------------------------------------------------------------------------------------- the run's flag
def test_the_flag_from_toml_and_from_the_command_line(tmp_path):
    assert RunParams(seed=1).merge_duplicates is False
    assert R.parse_args(["--seed", "1"])[0].merge_duplicates is False
    assert R.parse_args(["--seed", "1", "--merge-duplicates"])[0].merge_duplicates is True
    toml = tmp_path / "merge.toml"
    toml.write_text("[hyperparameters]\nnum_games = 16\nmerge_duplicates = true\n", encoding="utf-8")
    p, _ = R.parse_args(["--config", str(toml), "--seed", "1"])
    assert p.merge_duplicates is True and p.num_games == 16
    toml.write_text("[hyperparameters]\nmerge_duplicates = false\n", encoding="utf-8")
    assert R.parse_args(["--config", str(toml), "--seed", "1"])[0].merge_duplicates is False
    assert R.parse_args(["--config", str(toml), "--seed", "1", "--merge-duplicates"])[0].merge_duplicates is True
    assert RunParams(seed=1, merge_duplicates=1).as_dict()["merge_duplicates"] is True


class RecordingFitter(StubFitter):
    """the stub fitter of tests/test_run_cpu.py that writes down the calls that shape the data set, and the fit's start"""

    def __init__(self):
        self.calls = []
        super().__init__()

    def clear_data(self):
        self.calls.append("clear_data")
        super().clear_data()

    def add_samples(self, sp, oc):
        self.calls.append("add")
        super().add_samples(sp, oc)

    def merge_duplicates(self, normalize=True):
        self.calls.append(("merge_duplicates", normalize))
        n = self.sp.shape[0]
        return n, n - 3  # the stub keeps its samples: what is recorded is the call and its place

    def set_weights(self, w):
        self.calls.append("fit")
        super().set_weights(w)


@pytest.mark.parametrize("flag", [False, True])
def test_the_run_merges_once_between_the_last_add_and_the_fit(tmp_path, flag):
    fitter = RecordingFitter()
    run = open_run(small(tmp_path, mix_old=True, merge_duplicates=flag), fitter)
    results = []
    for _ in range(2):
        del fitter.calls[:]
        results.append(run.generation())
        calls = [c for c in fitter.calls if c != "clear_data"]
        assert fitter.calls[0] == "clear_data" and fitter.calls.count("clear_data") == 1
        merges = [c for c in calls if isinstance(c, tuple)]
        if not flag:
            assert merges == [] and results[-1].merged is None
            continue
        assert merges == [("merge_duplicates", True)]
        at = calls.index(merges[0])
        adds = len(results)  # this generation's samples, and with mix_old those of the generations before
        assert calls[:at] == ["add"] * adds and calls[at + 1] == "fit"
        n = sum(r.num_samples for r in results)
        assert results[-1].merged == (n, n - 3)
    # the sample file stays the un-merged export
    sp, _ = R.samples_io.load_packed(run._samples(2))
    assert sp.shape[0] == results[1].num_samples
