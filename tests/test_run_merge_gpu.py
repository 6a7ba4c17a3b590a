"""The run driver's merge_duplicates flag on the device (corintho_ai_amd/run.py): one generation of a tiny run with the
flag set equals the same generation repeated by hand -- Trainer, export_samples, the host merge
(samples_io.merge_duplicates_host), fit_samples with its weights, an arena -- with the seeds the driver reports:
weights, optimizer state and score, bit for bit."""
import os

import pytest

from corintho_ai_amd import Run, Trainer, samples_io
from corintho_ai_amd import run as R
from corintho_ai_amd.fit import fit_samples
from tests.test_run_gpu import model, params

pytestmark = pytest.mark.gpu


def test_a_merged_generation_pinned_against_the_pieces(tmp_path):
    with Run.open(params(tmp_path, "mlp12x100", merge_duplicates=True)) as run:
        first = run.generation()
    p = run.params
    kind, net = R.PLAY_KINDS[(p.net, p.arith)], R.NETS[p.net][0]
    w0, opt0 = model(run, 0)
    # self-play with the driver's seed; the sample file is the un-merged export
    t = Trainer(p.num_games, "", first.seeds["selfplay"], p.max_searches, p.searches_per_eval, p.c_puct, p.epsilon, 0, 1,
                False)
    t.set_net(kind, w0)
    assert t.run()
    sp, oc = t.export_samples()
    t.close()
    assert sp.tobytes() + oc.tobytes() == b"".join(x.tobytes() for x in samples_io.load_packed(
        os.path.join(run.root, "samples", "gen_1")))
    assert first.num_samples == sp.shape[0]
    # the merge, on the host
    msp, moc, mw = samples_io.merge_duplicates_host(sp, oc, normalize=True)
    assert first.merged == (sp.shape[0], msp.shape[0]) and msp.shape[0] < sp.shape[0]
    # the fit on the merged samples with their weights
    res = fit_samples(w0, msp, moc, sample_weight=mw, seed=first.seeds["fit"], optimizer_state=opt0,
                      learning_rate=p.learning_rate, batch_size=p.batch_size, epochs=p.epochs, anneal_factor=p.anneal_factor,
                      patience=p.patience, net=net)
    assert res.history == first.fit.history
    assert res.best_weights.tobytes() == first.fit.best_weights.tobytes() == model(run, 1)[0].tobytes()
    m, v, it = model(run, 1)[1]
    assert res.best_optimizer[0].tobytes() == m.tobytes() and res.best_optimizer[1].tobytes() == v.tobytes()
    assert res.best_optimizer[2] == it > 0
    # fit_time.txt keeps the reference's lines and counts the generation's samples
    with open(os.path.join(run.root, "generations", "gen_1", "training_logs", "fit_time.txt"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    assert len(lines) == 6 and lines[1] == "%d samples" % sp.shape[0]
    # the arena: slot 0 the best model, slot 1 the new one
    a = Trainer(p.num_test_games, "", first.seeds["arena"], p.max_searches, p.searches_per_eval, p.c_puct, p.epsilon, 0, 1,
                True)
    a.set_net(kind, w0, slot=0)
    a.set_net(kind, res.best_weights, slot=1)
    assert a.run()
    assert a.score() == first.score
    a.close()
