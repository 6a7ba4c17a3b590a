"""The canonical orientation without a GPU: the properties of its definition in numpy (samples_io.canonicalize_host), the
merge up to symmetry as a composition (samples_io.merge_duplicates_host(symmetries=True)), and the run driver's
merge_symmetries flag -- read from TOML and from the command line, and one call of the fitter's merge with the keyword
(a recording fitter on the emulation build, as tests/test_sample_merge_cpu.py)."""
import numpy as np
import pytest

from corintho_ai_amd import RunParams
from corintho_ai_amd import run as R
from corintho_ai_amd.samples_io import canonicalize_host, merge_duplicates_host
from tests import symmetry_cases as SC
from tests.symmetry_cases import GS, image, same, stabiliser
from tests.test_run_cpu import StubFitter, open_run, small


@pytest.fixture(scope="module")
def base():
    return SC.samples(12, 61)[0]


def test_idempotent_and_k_star_zero_on_a_canonical_set(base):
    mixed = image(base, np.arange(12) % 8)
    once, k1 = canonicalize_host(mixed)
    assert once.dtype == np.float32 and k1.dtype == np.int32 and k1.shape == (12,)
    assert np.count_nonzero(k1) > 0
    twice, k2 = canonicalize_host(once)
    assert same(once, twice) and not k2.any()
    # cells 64..69 never move, and the candidate is the image it says it is
    assert same(once[:, 64:GS], mixed[:, 64:GS])
    assert same(once, image(mixed, k1))
    empty, k0 = canonicalize_host(np.zeros((0, 166), np.float32))
    assert empty.shape == (0, 166) and k0.shape == (0,)
    with pytest.raises(ValueError):
        canonicalize_host(np.zeros((3, 70), np.float32))


def test_every_image_of_a_sample_has_the_same_canonical_sample(base):
    assert all(stabiliser(b[:GS]) == [0] for b in base)
    want = canonicalize_host(base)[0]
    stars = set()
    for j in range(8):
        got, k_star = canonicalize_host(image(base, j))
        assert same(got, want), j  # the state and, the stabiliser being trivial, the policy
        stars.update(k_star.tolist())
    assert stars == set(range(8))


def test_a_symmetric_state_keeps_its_canonical_state_and_the_start_position_stays(base):
    half = base[0].copy()
    half[:GS] = np.maximum(half[:GS], half[:GS][SC.gather()[1]])
    assert stabiliser(half[:GS]) == [0, 1]
    want = canonicalize_host(half[None])[0][0]
    fixing = stabiliser(want[:GS])  # of the canonical state: a conjugate of {0, 1}
    assert len(fixing) == 2 and fixing[0] == 0
    either = [image(want, h)[0] for h in fixing]
    assert not same(either[0], either[1])
    seen = set()
    for j in range(8):
        got = canonicalize_host(image(half, j))[0][0]
        assert same(got[:GS], want[:GS])
        which = [same(got, e) for e in either]  # the policy is one of the two that the stabiliser exchanges
        assert any(which), j
        seen.add(which.index(True))
    assert seen == {0, 1}
    start = np.concatenate([SC.start_position(), base[1][GS:]]).astype(np.float32)
    assert stabiliser(start[:GS]) == list(range(8))
    got, k_star = canonicalize_host(start[None])
    assert k_star.tolist() == [0] and same(got[0], start)


def test_the_order_is_that_of_unsigned_patterns(base):
    """-0.0 (0x80000000) sorts after 0.0 and after 1.0 (0x3f800000): as a signed integer or as a float it would not"""
    s = base[2].copy()
    s[:64] = 0.0
    s[0], s[3] = np.float32(-0.0), np.float32(1.0)  # cell 0 holds {-0.0, 0, 0, 1.0}: its images put it in cells 3, 12, 15
    got, k_star = canonicalize_host(s[None])
    words = got[0, :64].view(np.uint32)
    cands = [image(s, k)[0][:64].view(np.uint32).tolist() for k in range(8)]
    assert words.tolist() == min(cands) and cands.index(min(cands)) == int(k_star[0]) and k_star[0] != 0
    assert words[0] == 0  # a candidate that begins with 0.0 wins over the one that begins with -0.0
    plain = s.copy()
    plain[0] = np.float32(0.0)
    a, b = canonicalize_host(plain[None])[0][0], got[0]
    at = int(np.flatnonzero(a[:64].view(np.uint32) != b[:64].view(np.uint32))[0])
    assert a[:64].view(np.uint32)[at] < b[:64].view(np.uint32)[at]  # the state with -0.0 sorts after the same with 0.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_merge_up_to_symmetry_is_the_merge_of_the_canonical_samples(weighted, normalize):
    sp, oc, orbit_of = SC.planted(9, 70, 81, exact=6)
    w = np.random.default_rng(82).uniform(0.0, 3.0, 70).astype(np.float32) if weighted else None
    got = merge_duplicates_host(sp, oc, w, normalize=normalize, symmetries=True)
    want = merge_duplicates_host(canonicalize_host(sp)[0], oc, w, normalize=normalize)
    for g, x in zip(got, want):
        assert same(g, x)
    assert got[0].shape[0] == 9 == np.unique(orbit_of).size
    plain = merge_duplicates_host(sp, oc, w, normalize=normalize)
    assert plain[0].shape[0] > 9
    for g, x in zip(merge_duplicates_host(sp, oc, w, normalize=normalize, symmetries=False), plain):
        assert same(g, x)
    if not weighted and not normalize:  # a group's weight is the size of its orbit, in the order of the first members
        firsts = [int(np.flatnonzero(orbit_of == o)[0]) for o in range(9)]
        assert got[2].tolist() == [float(np.sum(orbit_of == o)) for o in np.argsort(firsts)]


# ---------------------------------------------------------------------------------------------------- the run's flag
def test_the_flag_from_toml_and_from_the_command_line(tmp_path):
    p = RunParams(seed=1)
    assert p.merge_symmetries is False and p.merge_duplicates is False
    assert R.parse_args(["--seed", "1"])[0].merge_symmetries is False
    p = R.parse_args(["--seed", "1", "--merge-symmetries"])[0]
    assert p.merge_symmetries is True and p.merge_duplicates is True  # it implies the merge
    p = R.parse_args(["--seed", "1", "--merge-duplicates"])[0]
    assert p.merge_symmetries is False and p.merge_duplicates is True
    toml = tmp_path / "merge.toml"
    toml.write_text("[hyperparameters]\nnum_games = 16\nmerge_symmetries = true\n", encoding="utf-8")
    p, _ = R.parse_args(["--config", str(toml), "--seed", "1"])
    assert p.merge_symmetries is True and p.merge_duplicates is True and p.num_games == 16
    toml.write_text("[hyperparameters]\nmerge_symmetries = false\n", encoding="utf-8")
    assert R.parse_args(["--config", str(toml), "--seed", "1"])[0].merge_symmetries is False
    assert R.parse_args(["--config", str(toml), "--seed", "1", "--merge-symmetries"])[0].merge_symmetries is True
    assert RunParams(seed=1, merge_symmetries=1).as_dict()["merge_symmetries"] is True


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

    def merge_duplicates(self, normalize=True, symmetries=False):
        self.calls.append(("merge_duplicates", normalize, symmetries))
        n = self.sp.shape[0]
        return n, n - 5  # the stub keeps its samples: what is recorded is the call and its place

    def set_weights(self, w):
        self.calls.append("fit")
        super().set_weights(w)


@pytest.mark.parametrize("flags, want", [({}, None), ({"merge_duplicates": True}, False), ({"merge_symmetries": True}, True)])
def test_the_run_merges_once_with_the_keyword_between_the_last_add_and_the_fit(tmp_path, flags, want):
    fitter = RecordingFitter()
    run = open_run(small(tmp_path, mix_old=True, **flags), fitter)
    results = []
    for _ in range(2):
        del fitter.calls[:]
        results.append(run.generation())
        calls = [c for c in fitter.calls if c != "clear_data"]
        merges = [c for c in calls if isinstance(c, tuple)]
        if want is None:
            assert merges == [] and results[-1].merged is None
            continue
        assert merges == [("merge_duplicates", True, want)]
        at = calls.index(merges[0])
        assert calls[:at] == ["add"] * len(results) and calls[at + 1] == "fit"
        n = sum(r.num_samples for r in results)
        assert results[-1].merged == (n, n - 5)  # (before, after), as without the keyword
