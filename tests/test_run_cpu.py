"""The training run driver (corintho_ai_amd/run.py) without a GPU: the emulation build plays (through `_cdll`) and a
float32 restatement fitter that speaks the packed protocol fits (through `_fitter`).  What is pinned here is the run's
bookkeeping: the directory, the gate, which weights and which Adam state a generation starts from, the replay window,
resume after an interruption, determinism, the settings and the packed sample files."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from corintho_ai_amd import Run, RunParams, expand_samples, samples_io, train_generation
from corintho_ai_amd import run as R
from tests import fit_ref
from tests import fit_ref_step as S
from tests.conftest import REFERENCE, ROOT
from tests.emu import emulib

TOML = os.path.join(REFERENCE, "toml")


class StubFitter(S.RefBackend):
    """fit_ref's restatement in float32 behind the packed protocol of fit.Fitter; it records what the driver gives it"""

    def __init__(self):
        super().__init__("mlp12x100", torch.float32)
        self.num_weights = R.nets.MLP_NUM_WEIGHTS
        self.started_from = []   # (weights, m, v, iterations) of every fit
        self.datasets = []       # (state_policy, outcome) every fit ran on
        self.clear_data()

    def set_weights(self, w):
        super().set_weights(w)
        self.started_from.append([np.array(w, np.float32)])

    def set_optimizer(self, m, v, iterations):
        super().set_optimizer(m, v, iterations)
        self.started_from[-1] += [np.array(m, np.float32), np.array(v, np.float32), int(iterations)]

    def clear_data(self):
        self.sp, self.oc = np.zeros((0, 166), np.float32), np.zeros(0, np.float32)
        self.data = None

    def add_samples(self, sp, oc):
        self.sp, self.oc = np.concatenate([self.sp, sp]), np.concatenate([self.oc, oc])
        self.data = None

    def add_trainer_samples(self, trainer):
        sp, oc = trainer.export_samples()
        self.add_samples(sp, oc)
        return sp.shape[0]

    def data_info(self):
        return 8 * self.sp.shape[0], self.sp.shape[0]

    def train(self, *a, **kw):
        if self.data is None:
            self.data = expand_samples(self.sp, self.oc, _cdll=emulib.load())
            self.datasets.append((self.sp.copy(), self.oc.copy()))
        return super().train(*a, **kw)


def small(tmp, name="run", **kw):
    """the shapes of this file: 8 games, 24 searches, 4 a batch, 4 test games, 2 epochs of batch 64, 1 game logged"""
    args = dict(cwd=str(tmp), name=name, num_games=8, max_searches=24, searches_per_eval=4, num_test_games=4, epochs=2,
                batch_size=64, num_logged=1, learning_rate=0.001, patience=2, num_old_gens=2, arith="f32", seed=7)
    threshold = kw.pop("test_threshold", None)
    args.update(kw)
    p = RunParams(**args)
    if threshold is not None:
        p.test_threshold = threshold  # outside the clamp of wrapper.py:157-160: a gate that always or never opens
    return p


def open_run(params, fitter=None):
    return Run.open(params, _cdll=emulib.load(), _fitter=fitter or StubFitter())


def tree(root):
    out = set()
    for d, dirs, files in os.walk(root):
        for n in dirs + files:
            out.add(os.path.relpath(os.path.join(d, n), root))
    return out


TIMED = ("play_time.txt", "fit_time.txt")  # hold seconds; metadata.txt holds the start time and the run's own paths


def comparable(root):
    """{relative path: bytes} of a run directory without the files that hold times; metadata.txt as its settings"""
    out = {}
    for rel in sorted(tree(root)):
        path = os.path.join(root, rel)
        if os.path.isdir(path) or os.path.basename(rel) in TIMED:
            continue
        with open(path, "rb") as f:
            data = f.read()
        if os.path.basename(rel) == "metadata.txt":
            d = json.loads(data)
            data = {k: v for k, v in d.items() if k != "start_time" and not isinstance(v, list)
                    and not (isinstance(v, str) and os.sep in v)}
        out[rel] = data
    return out


def model(run, k):
    return R.load_model(os.path.join(run.root, "generations", "gen_%d" % k, "model.npz"))


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """three generations behind a gate that is always open; (run, results, fitter)"""
    fitter = StubFitter()
    run = open_run(small(tmp_path_factory.mktemp("three"), test_threshold=-1), fitter)
    return run, [run.generation() for _ in range(3)], fitter


def test_new_run_layout(tmp_path):
    run = open_run(small(tmp_path))
    assert tree(run.root) == {
        "metadata", "metadata/current_generation.txt", "metadata/best_generation.txt", "metadata/learning_rate.txt",
        "metadata/fails.txt", "generations", "generations/gen_0", "generations/gen_0/model.npz",
        "generations/gen_0/rating.txt", "generations/gen_1", "samples", "samples/gen_1"}
    assert open(os.path.join(run.root, "generations/gen_0/rating.txt")).read() == "100"
    assert run.state() == {"current_generation": 0, "best_generation": 0, "learning_rate": 0.001, "fails": 0, "losses": []}
    with np.load(os.path.join(run.root, "generations/gen_0/model.npz")) as z:
        assert set(z.files) == {"weights", "adam_m", "adam_v", "adam_iterations", "net"}
        assert str(z["net"]) == "mlp12x100" and int(z["adam_iterations"]) == 0
        assert z["weights"].shape == (R.nets.MLP_NUM_WEIGHTS,) and not z["adam_m"].any() and not z["adam_v"].any()


def test_three_generations_layout_and_file_forms(three):
    run, results, _ = three
    assert run.state()["current_generation"] == 3 and [r.generation for r in results] == [1, 2, 3]
    per_generation = {"model.npz", "rating.txt", "metadata.txt", "training_logs", "testing_logs",
                      "training_logs/train_loss.csv", "training_logs/fit_time.txt", "training_logs/play_time.txt",
                      "training_logs/score_verbose.txt", "training_logs/game_0.txt", "testing_logs/score.txt",
                      "testing_logs/score_verbose.txt", "testing_logs/play_time.txt", "testing_logs/game_0.txt"}
    for k, res in zip((1, 2, 3), results):
        g = os.path.join(run.root, "generations", "gen_%d" % k)
        assert tree(g) == per_generation
        assert tree(os.path.join(run.root, "samples", "gen_%d" % k)) == {"samples.npz"}
        meta = json.load(open(os.path.join(g, "metadata.txt")))
        assert meta["num_games"] == 8 and meta["current_generation"] == k - 1 and "start_time" in meta
        assert meta["new_model_location"] == os.path.join(g, "model.npz")
        lines = open(os.path.join(g, "training_logs", "train_loss.csv")).read().splitlines()
        assert lines[0].split("\t")[0] == "epoch" and lines[0].split("\t")[-1] == "val_loss" and len(lines) == 3
        assert [float(x.split("\t")[-1]) for x in lines[1:]] == res.fit.history["val_loss"]
        score_text = open(os.path.join(g, "testing_logs", "score.txt")).read()
        assert score_text == "New agent score %f!\n" % res.score
        score = float(score_text.split()[3][:-1])  # six decimals: exact for the eighths that four games can score
        best_rating = float(open(os.path.join(run.root, "generations", "gen_%d" % (k - 1), "rating.txt")).read())
        with np.errstate(divide="ignore"):
            want = best_rating - 400 * np.log10(1 / score - 1) if score > 0 else best_rating - 400  # main.pyx:278-281
        assert open(os.path.join(g, "rating.txt")).read() == "%s\n" % want and res.rating == want
    assert run.state()["losses"] == [min(r.fit.history["val_loss"]) for r in results]


def test_update_rating_formula(tmp_path):
    f = str(tmp_path / "rating.txt")
    assert R.update_rating(f, 100, 0.75) == 100 - 400 * np.log10(1 / 0.75 - 1)
    assert open(f).read() == "%s\n" % (100 - 400 * np.log10(1 / 0.75 - 1))
    assert R.update_rating(f, 250.0, 0.0) == -150.0 and open(f).read() == "-150.0\n"  # the score == 0 branch
    assert R.update_rating(f, 100, 0.5) == 100.0


def test_gate_open(three):
    run, results, _ = three
    assert all(r.improved for r in results)
    st = run.state()
    assert st["best_generation"] == 3 and st["fails"] == 0 and st["learning_rate"] == 0.001


def expected_rate_rule(losses, fails, rate, patience, factor):
    """write_learning_rate of a failed generation (wrapper.py:451-487), restated for the test"""
    if all(losses[-1] < x for x in losses[:-1]):
        return 0, rate
    if fails + 1 >= patience:
        return 0, rate * factor
    return fails + 1, rate


def test_gate_shut(tmp_path):
    fitter = StubFitter()
    run = open_run(small(tmp_path, test_threshold=2), fitter)
    gen0 = model(run, 0)[0]
    fails, rate = 0, 0.001
    for k in (1, 2, 3, 4):
        res = run.generation()
        st = run.state()
        assert not res.improved and st["best_generation"] == 0 and st["current_generation"] == k
        fails, new_rate = expected_rate_rule(st["losses"], fails, rate, 2, 0.5)
        rate = new_rate
        assert (st["fails"], st["learning_rate"]) == (fails, rate)
        # the fit goes on from the latest model ...
        assert fitter.started_from[-1][0].tobytes() == model(run, k - 1)[0].tobytes()
    # ... while self-play kept taking generation 0's weights: generation 4's samples are those of a trainer with them
    seeds = res.seeds
    t = R._trainer.Trainer(8, "", seeds["selfplay"], 24, 4, 1.0, 0.25, 0, 1, False, _cdll=emulib.load())
    t.set_net(R._trainer.NET_MLP12X100, gen0)
    assert t.run()
    sp, oc = samples_io.load_packed(os.path.join(run.root, "samples", "gen_4"))
    assert sp.tobytes() == t.export_samples()[0].tobytes() and oc.tobytes() == t.export_samples()[1].tobytes()


@pytest.mark.parametrize("losses,fails,want", [
    ([0.9, 0.8, 0.7], 1, (0, None)),        # the last line is the minimum: the loss improved, fails back to 0
    ([0.9, 0.7, 0.7], 0, (1, None)),        # a tie is no improvement; fails below patience
    ([0.7, 0.9, 0.8], 0, (1, None)),        # better than the last generation, but not the minimum of the whole file
    ([0.7, 0.9], 1, (0, 0.004 * 0.5)),      # fails at patience: the rate the generation started with, times the factor
    ([0.7], 1, (0, None)),                  # a single line is its own minimum
], ids=["minimum", "tie", "not-the-minimum", "at-patience", "single"])
def test_write_learning_rate_rule(tmp_path, losses, fails, want):
    loss_file, rate_file, fail_file = (str(tmp_path / n) for n in ("losses.txt", "learning_rate.txt", "fails.txt"))
    open(loss_file, "w").write("".join("%s\n" % x for x in losses))
    open(rate_file, "w").write("0.008")  # what the file holds is not what the factor is applied to
    open(fail_file, "w").write("%d" % fails)
    R.write_learning_rate(0, 5, loss_file, rate_file, fail_file, 0.004, 2, 0.5)
    assert int(open(fail_file).read()) == want[0]
    assert open(rate_file).read() == ("0.008" if want[1] is None else "%s" % want[1])
    # a passed generation: fails to 0 whatever the losses say, the rate untouched
    open(fail_file, "w").write("1")
    R.write_learning_rate(5, 5, loss_file, rate_file, fail_file, 0.004, 2, 0.5)
    assert open(fail_file).read() == "0" and open(rate_file).read() == ("0.008" if want[1] is None else "%s" % want[1])


@pytest.mark.parametrize("threshold", [-1, 2], ids=["passed", "failed"])
def test_fit_starts_from_the_current_generation(tmp_path, threshold):
    fitter = StubFitter()
    run = open_run(small(tmp_path, test_threshold=threshold), fitter)
    run.generation()
    run.generation()
    w, (m, v, it) = model(run, 1)
    got = fitter.started_from[1]
    assert got[0].tobytes() == w.tobytes() and got[1].tobytes() == m.tobytes() and got[2].tobytes() == v.tobytes()
    assert got[3] == it and it > 0 and m.any()
    first = fitter.started_from[0]
    assert first[0].tobytes() == model(run, 0)[0].tobytes() and first[3] == 0 and not first[1].any()


@pytest.fixture(scope="module")
def four_mixed(tmp_path_factory):
    fitter = StubFitter()
    run = open_run(small(tmp_path_factory.mktemp("mixed"), mix_old=True), fitter)
    for _ in range(4):
        run.generation()
    return run, fitter


def test_window_mixed(four_mixed):
    run, fitter = four_mixed
    packed = {k: samples_io.load_packed(os.path.join(run.root, "samples", "gen_%d" % k)) for k in (1, 2, 3, 4)}
    sp, oc = fitter.datasets[3]
    assert sp.tobytes() == np.concatenate([packed[4][0], packed[2][0], packed[3][0]]).tobytes()
    assert oc.tobytes() == np.concatenate([packed[4][1], packed[2][1], packed[3][1]]).tobytes()
    assert fitter.datasets[0][0].tobytes() == packed[1][0].tobytes()  # generation 1 has no window


def test_window_read_but_not_used(tmp_path):
    fitter = StubFitter()
    run = open_run(small(tmp_path), fitter)
    for _ in range(3):
        run.generation()
    sp3 = samples_io.load_packed(os.path.join(run.root, "samples", "gen_3"))[0]
    assert fitter.datasets[2][0].tobytes() == sp3.tobytes()
    old = os.path.join(run.root, "samples", "gen_2", "samples.npz")
    data = open(old, "rb").read()
    open(old, "wb").write(data[:len(data) // 2])
    with pytest.raises(Exception):
        run.generation()
    assert run.state()["current_generation"] == 3


class Interrupt(Exception):
    pass


def interrupt_at(stage):
    def hook(s):
        if s == stage:
            raise Interrupt(stage)
    return hook


@pytest.fixture(scope="module")
def uninterrupted(tmp_path_factory):
    run = open_run(small(tmp_path_factory.mktemp("whole")))
    run.generation()
    run.generation()
    return comparable(run.root)


@pytest.mark.parametrize("stage", ["selfplay", "fit", "arena"])
def test_resume(tmp_path, uninterrupted, stage):
    run = open_run(small(tmp_path))
    run.generation()
    before = run.state()
    with pytest.raises(Interrupt):
        run.generation(_hook=interrupt_at(stage))
    assert run.state()["current_generation"] == 1
    assert {k: v for k, v in run.state().items() if k != "losses"} == {k: v for k, v in before.items() if k != "losses"}
    left = tree(os.path.join(run.root, "generations", "gen_2"))
    assert ("model.npz" in left) == (stage != "selfplay") and ("rating.txt" in left) == (stage == "arena")
    run.close()
    again = open_run(small(tmp_path))  # a new process would do no more than this
    assert again.generation().generation == 2
    got = comparable(again.root)
    assert set(got) == set(uninterrupted)
    for rel in got:
        assert got[rel] == uninterrupted[rel], rel


def test_determinism(tmp_path, uninterrupted):
    run = open_run(small(tmp_path / "other", name="other"))
    run.generation()
    run.generation()
    got = comparable(run.root)
    for rel in ("generations/gen_2/model.npz", "samples/gen_2/samples.npz", "samples/gen_1/samples.npz",
                "metadata/losses.txt", "generations/gen_2/rating.txt"):
        assert got[rel] == uninterrupted[rel], rel
    other_seed = open_run(small(tmp_path / "third", seed=8))
    other_seed.generation()
    assert comparable(other_seed.root)["samples/gen_1/samples.npz"] != uninterrupted["samples/gen_1/samples.npz"]


def test_train_generation_is_exported_and_leaves_the_metadata(tmp_path):
    run = open_run(small(tmp_path))
    state = run.setup_generation()
    res = train_generation(run.params, state, _cdll=emulib.load(), _fitter=StubFitter())
    assert res.generation == 1 and set(res.seeds) == {"selfplay", "arena", "fit"} and res.num_samples > 0
    assert set(res.times) == {"selfplay", "samples", "fit", "arena"}
    assert run.state()["current_generation"] == 0 and run.state()["losses"] == [res.val_loss]


def test_fp16_range_names_x6():
    err = R._lib.EngineError("corintho_hip error -3: mlp12x100h3: an activation left the fp16 range of the f16x3 kernels")
    with pytest.raises(RuntimeError, match='arith="x6"'):
        R._fp16_range(err, 3, "h3")
    R._fp16_range(R._lib.EngineError("something else"), 3, "h3")  # not its business


# ---------------------------------------------------------------------------------------------------- settings
def test_config_train_toml():
    p, generations = R.parse_args(["--config", os.path.join(TOML, "train.toml"), "--seed", "1"])
    want = dict(num_games=25000, max_searches=1600, c_puct=3.0, epsilon=0.25, num_test_games=1600, test_threshold=0.52,
                num_threads=0, searches_per_eval=16, learning_rate=0.001, batch_size=2048, epochs=10, anneal_factor=0.5,
                patience=2, num_old_gens=2, name="train", cwd="./logs", num_logged=10)
    assert {k: getattr(p, k) for k in want} == want and generations == 1
    assert (p.net, p.arith, p.sample_format, p.mix_old, p.zip_logs) == ("mlp12x100", "h3", "packed", False, False)
    # a flag beats the file; the small reader gives what a TOML module gives
    p, generations = R.parse_args(["--config", os.path.join(TOML, "test.toml"), "--num_games=12", "--generations", "3"])
    assert p.num_games == 12 and generations == 3
    for name in ("train.toml", "test.toml"):
        path = os.path.join(TOML, name)
        real = R.read_config(path)
        sys.modules.update(tomllib=None, tomli=None)  # both imports fail: the reader of key = value lines
        try:
            assert R.read_config(path) == real and {type(v) for v in real.values()} <= {int, float, str}
        finally:
            del sys.modules["tomllib"], sys.modules["tomli"]


def test_defaults_and_clamps():
    d = RunParams(seed=0)  # wrapper.py:24-132
    assert (d.anneal_factor, d.batch_size, d.c_puct, d.cwd, d.epochs, d.epsilon, d.learning_rate, d.max_searches, d.name,
            d.num_games, d.num_logged, d.num_old_gens, d.num_test_games, d.searches_per_eval, d.test_threshold) == (
        0.5, 2048, 1.0, ".", 1, 0.25, 0.01, 1600, "", 25000, 0, 20, 400, 1, 0.5)
    assert d.patience == 1  # max(1, min(epochs = 1, 3))
    p = RunParams(anneal_factor=3, batch_size=0, c_puct=-1, epochs=0, epsilon=7, learning_rate=-1, max_searches=1,
                  num_games=0, num_logged=-2, num_old_gens=-1, num_test_games=7, patience=9, searches_per_eval=50,
                  test_threshold=0.1, seed=0)  # wrapper.py:138-160
    assert (p.anneal_factor, p.batch_size, p.c_puct, p.epochs, p.epsilon, p.learning_rate, p.max_searches, p.num_games,
            p.num_logged, p.num_old_gens, p.num_test_games, p.patience, p.searches_per_eval, p.test_threshold) == (
        1.0, 1, 0.0, 1, 1.0, 0.0, 2, 1, 0, 0, 6, 1, 1, 0.5)
    assert RunParams(epochs=10, patience=0, seed=0).patience == 1 and RunParams(epochs=4, patience=9, seed=0).patience == 4
    assert RunParams(max_searches=10, searches_per_eval=40, seed=0).searches_per_eval == 9
    assert RunParams(num_test_games=4, test_threshold=5, seed=0).test_threshold == 3.5 / 4
    assert RunParams(num_threads=64, seed=0).num_threads == 64  # accepted, ignored
    assert isinstance(RunParams().seed, int)  # None: from the clock
    for bad in (dict(net="vgg"), dict(arith="f64"), dict(sample_format="csv")):
        with pytest.raises(ValueError):
            RunParams(**bad)
    assert dataclasses.is_dataclass(RunParams)


def test_help_exits_0():
    r = subprocess.run([sys.executable, "-m", "corintho_ai_amd.run", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--num_games" in r.stdout and "--generations" in r.stdout
    assert "RuntimeWarning" not in r.stderr  # runpy's, had the package imported the module before running it


# ---------------------------------------------------------------------------------------------------- packed files
def test_packed_files(tmp_path):
    s, z, p = fit_ref.synthetic_samples(37, 3)
    sp = np.concatenate([s, p], axis=1).astype(np.float32)
    samples_io.save_packed(str(tmp_path / "a"), sp, z)
    assert os.listdir(str(tmp_path / "a")) == ["samples.npz"]
    got = samples_io.load_packed(str(tmp_path / "a"))
    assert got[0].dtype == np.float32 and got[0].tobytes() == sp.tobytes() and got[1].tobytes() == z.tobytes()
    with np.load(str(tmp_path / "a" / "samples.npz")) as f:
        assert sorted(f.files) == ["outcome", "state_policy"]
    assert os.path.getsize(str(tmp_path / "a" / "samples.npz")) < sp.nbytes + z.nbytes + 1024  # uncompressed, no more
    samples_io.save_packed(str(tmp_path / "b"), sp, z)  # equal arrays, equal bytes
    assert open(str(tmp_path / "a" / "samples.npz"), "rb").read() == open(str(tmp_path / "b" / "samples.npz"), "rb").read()
    # a folder the reference wrote: the symmetry-0 rows of its three files are the samples
    samples_io.save_samples(str(tmp_path / "ref"), *expand_samples(sp, z, _cdll=emulib.load()))
    assert sorted(os.listdir(str(tmp_path / "ref"))) == ["evaluation_labels.npz", "game_states.npz", "probability_labels.npz"]
    got = samples_io.load_packed(str(tmp_path / "ref"))
    assert got[0].tobytes() == sp.tobytes() and got[1].tobytes() == z.tobytes()
    with pytest.raises(ValueError):
        samples_io.save_packed(str(tmp_path / "c"), sp[:, :100], z)
    with pytest.raises(ValueError):
        samples_io.save_packed(str(tmp_path / "c"), sp, z[:-1])


def test_reference_sample_format(tmp_path):
    run = open_run(small(tmp_path, sample_format="reference"))
    run.generation()
    folder = os.path.join(run.root, "samples", "gen_1")
    assert sorted(os.listdir(folder)) == ["evaluation_labels.npz", "game_states.npz", "probability_labels.npz", "samples.npz"]
    want = expand_samples(*samples_io.load_packed(folder), _cdll=emulib.load())
    for a, b in zip(samples_io.load_samples(folder), want):
        assert a.tobytes() == b.tobytes()
