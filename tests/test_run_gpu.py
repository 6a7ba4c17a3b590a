"""The training run driver (corintho_ai_amd/run.py) on the device, through the product path: Trainer.run(), the samples
device to device into a Fitter, fit_resident, the fused arena.  The driver adds bookkeeping and no arithmetic of its own:
a generation repeated by hand from the pieces (Trainer, samples_io.samples_for_training, fit, an arena) with the seeds the
driver reports gives the same weights, optimizer state, samples and score to the bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import corintho_ai_amd
from corintho_ai_amd import Run, RunParams, Trainer, expand_samples, fit, samples_io
from corintho_ai_amd import run as R
from corintho_ai_amd import trainer as trainer_module
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

NET_NAMES = ["mlp12x100", "rescnn4"]
SHAPES = dict(num_games=64, max_searches=50, searches_per_eval=16, num_test_games=32, epochs=2, batch_size=256,
              learning_rate=0.001, patience=2, anneal_factor=0.5, c_puct=3.0, num_old_gens=2, seed=11)


def params(tmp, net, **kw):
    return RunParams(**dict(SHAPES, cwd=str(tmp), name="run", net=net, **kw))


def read(run, *rel):
    with open(os.path.join(run.root, *rel), "rb") as f:
        return f.read()


def model(run, k):
    return R.load_model(os.path.join(run.root, "generations", "gen_%d" % k, "model.npz"))


def no_expansion(mp):
    """the three roads by which expanded rows (5 344 B each) reach the host raise"""
    def refuse(*a, **kw):
        raise AssertionError("the packed product path expanded samples on the host")

    mp.setattr(samples_io, "get_samples", refuse)
    mp.setattr(trainer_module, "expand_samples", refuse)
    mp.setattr(corintho_ai_amd, "expand_samples", refuse)
    mp.setattr(Trainer, "writeSamples", refuse)


@pytest.fixture(scope="module", params=NET_NAMES)
def product(request, tmp_path_factory):
    """three generations, packed samples, the window trained on; (run, results)"""
    with pytest.MonkeyPatch.context() as mp:
        no_expansion(mp)
        with Run.open(params(tmp_path_factory.mktemp(request.param), request.param, mix_old=True)) as run:
            results = [run.generation() for _ in range(3)]
    return run, results


def test_three_generations(product):
    run, results = product
    st = run.state()
    assert st["current_generation"] == 3 and len(st["losses"]) == 3 and [r.generation for r in results] == [1, 2, 3]
    assert st["best_generation"] == max([0] + [r.generation for r in results if r.improved])
    for k, res in zip((1, 2, 3), results):
        for rel in ("model.npz", "rating.txt", "metadata.txt", "training_logs/train_loss.csv", "training_logs/fit_time.txt",
                    "training_logs/play_time.txt", "training_logs/score_verbose.txt", "testing_logs/score.txt",
                    "testing_logs/score_verbose.txt", "testing_logs/play_time.txt"):
            assert read(run, "generations", "gen_%d" % k, rel), rel
        assert os.listdir(os.path.join(run.root, "samples", "gen_%d" % k)) == ["samples.npz"]
        sp, oc = samples_io.load_packed(os.path.join(run.root, "samples", "gen_%d" % k))
        assert sp.shape == (res.num_samples, 166) and oc.shape == (res.num_samples,) and res.num_samples >= 64
        assert 0.0 <= res.score <= 1.0 and res.improved == (res.score > run.params.test_threshold)
        assert np.isfinite(res.fit.history["val_loss"]).all() and len(res.fit.history["val_loss"]) == 2
        w, (m, v, it) = model(run, k)
        assert w.tobytes() == res.fit.best_weights.tobytes() and it == res.fit.best_optimizer[2] > 0


def test_generation_2_pinned_against_the_pieces(product, tmp_path):
    run, results = product
    p, second = run.params, results[1]
    kind, net = R.PLAY_KINDS[(p.net, p.arith)], R.NETS[p.net][0]
    best = 1 if results[0].improved else 0
    best_w = model(run, best)[0]
    cur_w, cur_opt = model(run, 1)
    assert cur_opt[2] > 0
    # self-play: the same arguments, the best generation's weights
    t = Trainer(p.num_games, "", second.seeds["selfplay"], p.max_searches, p.searches_per_eval, p.c_puct, p.epsilon, 0, 1,
                False)
    t.set_net(kind, best_w)
    assert t.run()
    sp, oc = t.export_samples()
    assert sp.tobytes() + oc.tobytes() == b"".join(x.tobytes() for x in samples_io.load_packed(
        os.path.join(run.root, "samples", "gen_2")))
    # the samples by the reference's road: this generation's, then the window's (generation 1) from its three files
    old = str(tmp_path / "old_1")
    samples_io.save_samples(old, *expand_samples(*samples_io.load_packed(os.path.join(run.root, "samples", "gen_1"))))
    gs, ev, pr = samples_io.samples_for_training(t, str(tmp_path / "gen_2"), [old], mix_old=True)
    t.close()
    assert gs.shape[0] == 8 * (results[0].num_samples + second.num_samples)
    # the fit: the current generation's weights and Adam state; generation 1 cannot have changed the rate it started with
    res = fit(cur_w, gs, ev, pr, seed=second.seeds["fit"], optimizer_state=cur_opt, learning_rate=p.learning_rate,
              batch_size=p.batch_size, epochs=p.epochs, anneal_factor=p.anneal_factor, patience=p.patience, net=net)
    assert res.history == second.fit.history
    assert res.best_weights.tobytes() == second.fit.best_weights.tobytes() == model(run, 2)[0].tobytes()
    m, v, it = model(run, 2)[1]
    assert res.best_optimizer[0].tobytes() == m.tobytes() and res.best_optimizer[1].tobytes() == v.tobytes()
    assert res.best_optimizer[2] == it
    # the arena: slot 0 the best model, slot 1 the new one
    a = Trainer(p.num_test_games, "", second.seeds["arena"], p.max_searches, p.searches_per_eval, p.c_puct, p.epsilon, 0, 1,
                True)
    a.set_net(kind, best_w, slot=0)
    a.set_net(kind, res.best_weights, slot=1)
    assert a.run()
    assert a.score() == second.score
    a.close()


class Interrupt(Exception):
    pass


def test_resume_on_the_device(product, tmp_path):
    whole = product[0]

    def after_fit(stage):
        if stage == "fit":
            raise Interrupt

    with Run.open(params(tmp_path, whole.params.net, mix_old=True)) as run:
        run.generation()
        with pytest.raises(Interrupt):
            run.generation(_hook=after_fit)
        assert run.state()["current_generation"] == 1
    with Run.open(params(tmp_path, whole.params.net, mix_old=True)) as run:
        assert run.generation().generation == 2
        for rel in ("generations/gen_2/model.npz", "samples/gen_2/samples.npz", "generations/gen_2/rating.txt",
                    "generations/gen_2/testing_logs/score.txt", "generations/gen_2/training_logs/train_loss.csv"):
            assert read(run, rel) == read(whole, rel), rel
        # the interrupted attempt's line is gone: two generations, two losses, those of the uninterrupted run
        assert read(run, "metadata/losses.txt") == b"".join(read(whole, "metadata/losses.txt").splitlines(True)[:2])


@pytest.mark.parametrize("net", NET_NAMES)
def test_two_processes(net, tmp_path):
    models = []
    for name in ("a", "b"):
        args = ["--%s=%s" % kv for kv in dict(SHAPES, cwd=str(tmp_path / name), name="run", net=net).items()]
        r = subprocess.run([sys.executable, "-m", "corintho_ai_amd.run", "--generations", "2"] + args, cwd=ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = [x for x in r.stdout.splitlines() if x.startswith("generation ")]
        assert len(lines) == 2 and lines[0].startswith("generation 1:") and lines[1].startswith("generation 2:")
        with np.load(str(tmp_path / name / "run" / "generations" / "gen_2" / "model.npz")) as z:
            models.append({k: z[k].tobytes() for k in z.files})
    assert models[0] == models[1] and set(models[0]) == {"weights", "adam_m", "adam_v", "adam_iterations", "net"}


@pytest.mark.parametrize("net", NET_NAMES)
def test_reference_sample_format(net, tmp_path):
    with Run.open(params(tmp_path, net, sample_format="reference")) as run:
        run.generation()
    folder = os.path.join(run.root, "samples", "gen_1")
    assert sorted(os.listdir(folder)) == ["evaluation_labels.npz", "game_states.npz", "probability_labels.npz", "samples.npz"]
    for a, b in zip(samples_io.load_samples(folder), expand_samples(*samples_io.load_packed(folder))):
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("arith", ["x6", "f32"])
@pytest.mark.parametrize("net", NET_NAMES)
def test_arithmetic_kinds(net, arith, tmp_path):
    with Run.open(params(tmp_path, net, arith=arith)) as run:
        res = run.generation()
    assert res.generation == 1 and run.state()["current_generation"] == 1 and res.num_samples >= 64
