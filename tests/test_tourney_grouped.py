"""Grouped tournament rounds (Tourney.set_grouped): one scan, one compaction, one grouped network launch and one search
launch per round, whatever the number of models.  With exact offsets a match reads its own rows, so the matches are the
ones the per-model path plays -- and the ones the oracle plays when the same networks are evaluated for it."""
import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_MLP12X100_H3, NET_RESCNN4_H3, _lib, nets
from corintho_ai_amd.tourney import Tourney
from oracle import oracle as O
from tests import harness as H
from tests.engines import cdll, make_trainer

# the emulation build has the reference's network on the host only (the per-model fallback of the group); the product
# plays with the kind that has a grouped kernel
CASES = [pytest.param("emu", NET_MLP12X100, id="emu"), pytest.param("hip", NET_MLP12X100_H3, marks=pytest.mark.gpu, id="hip")]

# (player_id, model_id, max_searches, spe, c_puct, epsilon, random): three models, model 1 behind two players
PLAYERS = [(0, 0, 40, 4, 1.0, 0.25, False), (1, 1, 32, 8, 1.5, 0.25, False), (2, 1, 24, 16, 1.0, 0.0, False),
           (3, 2, 36, 8, 2.0, 0.25, False), (4, -1, 0, 0, 1.0, 0.25, True)]
MATCHES = [(0, 1), (1, 0), (2, 3), (3, 2), (0, 4), (4, 1), (2, 0), (3, 1), (1, 2), (4, 3), (2, 4), (0, 3)]
ROWS = sum(max(p[3] for p in PLAYERS) for _ in MATCHES)


def _weights():
    return {0: nets.init_mlp12x100(seed=5, bn_noise=True), 1: nets.trained_like_mlp12x100(1), 2: nets.init_mlp12x100(seed=7, bn_noise=True)}


def _build(factory, players=PLAYERS, matches=MATCHES):
    t = factory()
    for p in players:
        t.addPlayer(*p)
    for a, b in matches:
        t.addMatch(a, b, False)
    return t


def _engine_tourney(engine, kind, weights, grouped, players=PLAYERS):
    t = _build(lambda: Tourney(1, "", trace=True, _cdll=cdll(engine)), players)
    for mid, w in weights.items():
        t.set_net(mid, kind, w)
    if grouped:
        t.set_grouped(True)
    else:
        t.set_exact_offsets(True)
    return t


@pytest.fixture(scope="module", params=[pytest.param(("emu", NET_MLP12X100), id="emu"),
                                        pytest.param(("hip", NET_MLP12X100_H3), marks=pytest.mark.gpu, id="hip")])
def played(request):
    """the grouped tournament and the same one on the per-model path, both played to the end, once"""
    engine, kind = request.param
    g = _engine_tourney(engine, kind, _weights(), True)
    assert not g.run(max_rounds=3)
    assert g.run()
    p = _engine_tourney(engine, kind, _weights(), False)
    assert p.run()
    return engine, kind, g, p


def test_grouped_plays_the_matches_of_the_per_model_path(played, tmp_path):
    engine, kind, g, p = played
    assert g.stats()["tourney_path"] == 2 and p.stats()["tourney_path"] == 1
    for i in range(len(MATCHES)):
        assert np.array_equal(g.trace(i), p.trace(i)), "per-ply trace of match %d" % i
        assert g.match_info(i)["result"] == p.match_info(i)["result"] and g.match_info(i)["done"] == 1
        assert g.match_score(i) == p.match_score(i)
    sg, sp = g.stats(), p.stats()
    assert [sg[k] for k in ("searches", "evals", "nodes", "plies")] == [sp[k] for k in ("searches", "evals", "nodes", "plies")]
    fa, fb = tmp_path / "a.txt", tmp_path / "b.txt"
    g.writeScores(fa)
    p.writeScores(fb)
    assert fa.read_text() == fb.read_text() and len(fa.read_text().splitlines()) == len(MATCHES)


def test_grouped_replays_on_the_oracle(played):
    """the oracle with exact offsets, its networks evaluated by the engine's own kernels, one model at a time"""
    engine, kind, g, _ = played
    evaluators = {}
    for mid, w in _weights().items():
        t = make_trainer(engine, 64, "", 1, 50, 16, 1.0, 0.25, 0, 1, False)
        t.set_net(kind, w)
        evaluators[mid] = t
    o = _build(lambda: O.Tourney(2, "", trace=True))
    o.set_exact_offsets(True)
    H.play_tourney(o, [-1, 0, 1, 2], {mid: (lambda s, t=t: t.net_forward(s)) for mid, t in evaluators.items()}, ROWS)
    for i in range(len(MATCHES)):
        assert np.array_equal(g.trace(i), o.trace(i)), "per-ply trace of match %d" % i
        assert g.match_score(i) == o.match_score(i)


def test_launches_do_not_depend_on_the_number_of_models(played):
    """one network launch and one search launch per round: the same matches under three model ids and under two (model 2
    folded into model 1 with the same weights, so the play is the same) queue the same launches; the per-model path
    queues one search launch per model id and round"""
    engine, kind, g, p = played
    w = _weights()
    w[2] = w[1]
    three = _engine_tourney(engine, kind, w, True)
    assert three.run()
    two = _engine_tourney(engine, kind, {0: w[0], 1: w[1]}, True, players=[pl if pl[1] != 2 else (pl[0], 1) + pl[2:] for pl in PLAYERS])
    assert two.run()
    s3, s2 = three.stats(), two.stats()
    assert s3["tourney_path"] == 2 and s2["tourney_path"] == 2
    assert s3["nn_launches"] == s3["mcts_launches"] == s3["iterations"] > 0
    assert (s2["nn_launches"], s2["mcts_launches"]) == (s3["nn_launches"], s3["mcts_launches"])
    for i in range(len(MATCHES)):
        assert np.array_equal(three.trace(i), two.trace(i))
    sg, sp = g.stats(), p.stats()
    assert sg["nn_launches"] == sg["mcts_launches"]
    # (the per-model path: a search launch for each of the four ids -- three models and the random players' -- every round)
    assert sp["mcts_launches"] % 4 == 0 and sp["nn_launches"] == 3 * sp["mcts_launches"] // 4


@pytest.mark.parametrize("engine,kind", CASES)
def test_set_grouped_errors(engine, kind):
    w = _weights()
    t = _engine_tourney(engine, kind, w, True)
    with pytest.raises(_lib.EngineError, match="needs exact offsets"):
        t.set_exact_offsets(False)
    assert not t.run(max_rounds=1)
    with pytest.raises(_lib.EngineError, match="after the tournament has started"):
        t.set_grouped(True)
    # a model that is the caller's function evaluates its own launch: refused when the tournament runs
    f = _build(lambda: Tourney(1, "", _cdll=cdll(engine)))
    for mid in (0, 1):
        f.set_net(mid, kind, w[mid])
    f.set_net_fn(2, lambda *a: None, 8, 8, 8, ROWS)
    f.set_grouped(True)
    with pytest.raises(_lib.EngineError, match="model id 2 is a caller-supplied function"):
        f.run()


@pytest.mark.gpu
def test_models_of_two_kinds_take_the_per_model_path():
    w = _weights()
    t = _build(lambda: Tourney(1, "", trace=True))
    t.set_net(0, NET_MLP12X100_H3, w[0])
    t.set_net(1, NET_MLP12X100, w[1])
    t.set_net(2, NET_MLP12X100_H3, w[2])
    t.set_grouped(True)
    assert t.run()
    assert t.stats()["tourney_path"] == 1
    assert all(t.match_info(i)["done"] == 1 for i in range(len(MATCHES)))


@pytest.mark.gpu
def test_grouped_rescnn4_tournament_plays_the_matches_of_the_per_model_path():
    """the grouped rescnn4 f16x3 kernel in a tournament: tables cut for its 16 positions per workgroup"""
    w = {0: nets.trained_like_rescnn4(0), 1: nets.init_rescnn4(1, bn_noise=True), 2: nets.trained_like_rescnn4(2)}
    g = _engine_tourney("hip", NET_RESCNN4_H3, w, True)
    p = _engine_tourney("hip", NET_RESCNN4_H3, w, False)
    assert g.run() and p.run()
    assert g.stats()["tourney_path"] == 2 and p.stats()["tourney_path"] == 1
    assert g.stats()["nn_launches"] == g.stats()["mcts_launches"]
    for i in range(len(MATCHES)):
        assert np.array_equal(g.trace(i), p.trace(i)), "per-ply trace of match %d" % i
        assert g.match_score(i) == p.match_score(i)


@pytest.mark.parametrize("engine,kind", CASES)
def test_more_rows_than_the_tables_hold_take_the_per_model_path(engine, kind):
    """65 535 request rows are the grouping kernel's limit: 4 096 matches at 16 searches per evaluation are one more"""
    t = Tourney(1, "", _cdll=cdll(engine))
    t.addPlayer(0, 0, 16, 16, 1.0, 0.25, False)
    t.addPlayer(1, -1, 0, 0, 1.0, 0.25, True)
    for i in range(4096):
        t.addMatch(i % 2, 1 - i % 2, False)
    t.set_net(0, kind, _weights()[0])
    t.set_grouped(True)
    assert not t.run(max_rounds=1)
    assert t.stats()["tourney_path"] == 1
