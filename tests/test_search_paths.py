"""Parity cases that make the search take its rare paths (tests/search_cases.py; which branch each one reaches, and how
often, is counted by tests/test_search_census_cpu.py and tabled in DESIGN section 2):

  deep lines       a peaked stand-in network: groups that end at CO_SB_DEPTH, rows that share nodes for several levels
  fresh trees      an arena with one simulation per move
  drawn games      slices of larger generations around a game the oracle draws; arenas and tournaments with a draw
  Analyser         positions a few plies before a drawn or a decisive end, with one legal move, with empty reserves

Everything is compared bit for bit with the oracle, on the emulation build here and on the MI355X with -m gpu."""
import numpy as np
import pytest

from corintho_ai_amd import Tourney
from corintho_ai_amd.analyse import Analyser
from oracle import oracle as O
from tests import harness as H
from tests import search_cases as SC
from tests.engines import ENGINES, cdll, make_trainer

RESULT_DRAW = 2  # util.h:57-64


def run_pair(engine, case, tmp_path):
    """tests/test_engine_parity.py run_pair for a case of search_cases (slices and arena mode too), plus writeScores"""
    t = make_trainer(engine, case.G, "", case.seed, case.sims, case.spe, case.c_puct, case.eps, 0, 1, case.testing,
                     trace=True, stagger=case.stagger, game_base=case.game_base, total_games=case.total_games)
    net, pair = SC.nets_of(case)
    ra = H.play_generation(t, case.G, case.spe, net, nets_by_player=pair, record=True)
    o, rb = SC.run_selfplay_on_oracle(case, trace=True)
    assert ra["iterations"] == rb["iterations"]
    for i, (a, b) in enumerate(zip(ra["log"], rb["log"])):
        assert a[0] == b[0] and a[1].shape == b[1].shape, "request count differs at iteration %d" % i
        assert a[1].tobytes() == b[1].tobytes(), "request rows differ at iteration %d" % i
    for g in range(case.G):
        assert np.array_equal(t.trace(g), o.trace(g)), "per-ply trace of game %d" % g
        assert t.game_info(g)["result"] == o.game_result(g)
    sa, sb = H.get_samples(t), H.get_samples(o)
    for x, y in zip(sa, sb):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    assert t.num_samples() == o.num_samples() and (t.num_samples() == 0) == case.testing
    assert t.score() == o.score()
    assert t.avg_mate_length() == o.avg_mate_length()
    c = o.counters()
    st = t.stats()
    assert (st["searches"], st["evals"], st["nodes"], st["plies"]) == (c["searches"], c["leaf_evals"],
                                                                       c["nodes_created"], c["plies"])
    if not case.testing:
        H.check_sample_properties(*sa)
    fa, fb = str(tmp_path / "engine.txt"), str(tmp_path / "oracle.txt")
    t.writeScores(fa)
    o.writeScores(fb)
    assert open(fa, "rb").read() == open(fb, "rb").read()
    return t, o


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", SC.DEEP, ids=lambda c: "%dx%d_%s" % (c.G, c.sims, c.net))
def test_deep_lines_match_oracle(engine, case, tmp_path):
    run_pair(engine, case, tmp_path)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", SC.DRAWN + SC.DRAWN_ARENA,
                         ids=lambda c: "%s_seed%d_base%d" % ("arena" if c.testing else "train", c.seed, c.game_base))
def test_drawn_games_match_oracle(engine, case, tmp_path):
    """a drawn game's samples (value 0 on every ply), score 0.5, writeScores line and mate length"""
    t, o = run_pair(engine, case, tmp_path)
    drawn = [g for g in range(case.G) if o.game_result(g) == RESULT_DRAW]
    assert drawn, "the case no longer contains a drawn game on the oracle"
    if not case.testing:
        before = sum(o.game_num_samples(g) for g in range(drawn[0]))
        n = o.game_num_samples(drawn[0])
        ev = H.get_samples(t)[1][before * 8:(before + n) * 8]
        assert n > 0 and np.all(ev == 0.0)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", SC.FEW_ARENA, ids=lambda c: "%dx%d" % (c.G, c.sims))
def test_one_simulation_arena_matches_oracle(engine, case, tmp_path):
    """every move chosen at a root that has no visited child: the fresh tree of choose_move_normal"""
    run_pair(engine, case, tmp_path)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("salt", SC.DRAWN_TOURNEY_SALTS)
def test_drawn_match_matches_oracle(engine, salt, tmp_path):
    """tests/test_tourney.py test_tourney_matches_oracle on a tournament one of whose matches ends drawn"""
    players, matches = SC.DRAWN_TOURNEY_PLAYERS, SC.DRAWN_TOURNEY_MATCHES
    nets, rows = SC.drawn_tourney_nets(salt), SC.tourney_rows(players, matches)
    e = SC.build_tourney(lambda: Tourney(1, "", trace=True, _cdll=cdll(engine)), players, matches)
    o = SC.build_tourney(lambda: O.Tourney(2, "", trace=True), players, matches)
    ra = H.play_tourney(e, [-1, 0, 1], nets, rows, record=True)
    rb = H.play_tourney(o, [-1, 0, 1], nets, rows, record=True)
    assert ra["rounds"] == rb["rounds"]
    assert [(a[0], a[1].tobytes()) for a in ra["log"]] == [(b[0], b[1].tobytes()) for b in rb["log"]]
    for i in range(len(matches)):
        assert np.array_equal(e.trace(i), o.trace(i)), "per-ply trace of match %d" % i
        assert e.match_info(i)["result"] == o.match_info(i)["result"]
        assert e.match_score(i) == o.match_score(i)
    drawn = [i for i in range(len(matches)) if o.match_info(i)["result"] == RESULT_DRAW]
    assert drawn and all(e.match_score(i) == 0.5 for i in drawn)
    c, st = o.counters(), e.stats()
    assert (st["searches"], st["evals"], st["nodes"], st["plies"]) == (c["searches"], c["leaf_evals"],
                                                                       c["nodes_created"], c["plies"])
    fa, fb = tmp_path / "a.txt", tmp_path / "b.txt"
    e.writeScores(fa)
    o.writeScores(fb)
    assert fa.read_text() == fb.read_text() and len(fa.read_text().splitlines()) == len(matches)


def test_position_corpus_is_what_the_generator_promises():
    boards, tp, pc, seeds, kind, kinds = SC.load_positions()
    n = len(seeds)
    assert 60 <= n <= 72 and boards.shape == (n, 64) and pc.shape == (n, 6)
    terminal = 0
    for i in range(n):
        g = O.Game.from_arrays(boards[i], int(tp[i]), [int(x) for x in pc[i]])
        mask, _ = g.legal_mask()
        legal = bin(mask).count("1")
        terminal += legal == 0
        name = kinds[kind[i]]
        assert (legal == 0) == (name == "terminal")
        if name == "one_move":
            assert legal == 1
        if name == "empty_reserve":
            assert legal > 1 and sum(pc[i][3 * tp[i]:3 * tp[i] + 3]) == 0
    assert 0 < terminal <= n // 4
    assert {kinds[k] for k in kind} == set(kinds)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("net", SC.ANALYSIS_NETS)
@pytest.mark.parametrize("S_,spe", SC.ANALYSIS_SETTINGS)
def test_analysis_of_rare_positions_matches_dockermc(engine, S_, spe, net):
    """tests/test_analyse.py test_batched_analysis_matches_dockermc on the committed corpus: move, flags, legal moves,
    nodes, evaluation bits, request rows"""
    boards, tp, pc, seeds, _, _ = SC.load_positions()
    n = len(seeds)
    f = SC.NETS[net]()
    a = Analyser(boards, tp, pc, seeds, S_, spe, _cdll=cdll(engine))
    cap = n * spe
    evals = np.zeros(cap, np.float32)
    probs = np.zeros((cap, 96), np.float32)
    gs = np.zeros((cap, 70), np.float32)
    all_rows = set()
    while not a.doIteration(evals, probs):
        k = a.num_requests()
        assert k > 0
        a.writeRequests(gs)
        evals[:k], probs[:k] = f(gs[:k])
        all_rows.update(x.tobytes() for x in gs[:k])
    got = a.results()
    n_pre = 0
    for i in range(n):
        want, log = SC.analyse_on_oracle(boards[i], tp[i], pc[i], seeds[i], S_, spe, f)
        if "pre-result" in want:
            n_pre += 1
            assert got[i] == want
            continue
        g = dict(got[i])
        g.pop("evaluation")
        assert g == want, "position %d" % i
        for r in log:  # every row the single-position search asked for was asked for by the batch
            assert all(x.tobytes() in all_rows for x in r)
    assert 0 < n_pre <= n // 4
