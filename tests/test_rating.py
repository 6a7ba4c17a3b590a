"""The rating driver (corintho_ai_amd/rating.py): the maximum-likelihood fit against the reference's recorded ratings, the
pairing rule and the performance ratings against what the reference's own round.py wrote (tests/golden/rating_round.json,
tools/gen_rating_golden.py), a round on the engine and its resume."""
import json
import os

import numpy as np
import pytest

from corintho_ai_amd import rating as R
from corintho_ai_amd import nets, run
from tests.engines import cdll

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, "golden", "reference", "rating")


@pytest.fixture(scope="module")
def reference_record():
    with open(os.path.join(REF, "results.txt")) as f:
        rows = [tuple(int(v) for v in x.split()) for x in f if x.strip()]
    with open(os.path.join(REF, "gd_ratings.txt")) as f:
        ref = np.array([float(x) for x in f if x.strip()])
    assert ref.shape == (97,)
    return rows, ref, R.fit_ratings(rows, anchor=96)


def test_fit_is_the_maximum_of_the_reference_model(reference_record):
    """Measured (float64 Newton): largest gradient component 5e-11; against the reference's gd_ratings.txt the
    ratings of players 0..94 differ by a constant -2121.77 Elo -- its gradient ascent stopped short along the direction
    that separates the random player from everybody else: its log-likelihood is 67 below the maximum -- and, the median
    offset removed, by at most 0.25 Elo (rms 0.026); the first-move bias is -143.91 Elo.  The bound of 0.5 Elo is twice
    that measured gap, which is the reference's distance from the maximum, not this fit's."""
    rows, ref, fit = reference_record
    print("iterations %d, max gradient %.3g, bias %.2f, log-likelihood %.3f" % (fit.iterations, fit.max_gradient, fit.bias, fit.log_likelihood))
    assert fit.max_gradient < 1e-6 and fit.iterations < 50
    d = fit.ratings[:95] - ref[:95]
    off = np.median(d)
    print("offset %.2f, max difference %.3f, rms %.3f, top rating %.1f" % (off, np.max(np.abs(d - off)), np.sqrt(np.mean((d - off) ** 2)),
                                                                         np.max(fit.ratings[:95])))
    assert np.max(np.abs(d - off)) <= 0.5
    assert fit.ratings[96] == 0.0 and np.all(np.isfinite(fit.ratings))
    # the likelihood at the reference's ratings with the best bias for them (concave in b: golden section)
    lo, hi, g = -1000.0, 1000.0, (5 ** 0.5 - 1) / 2
    for _ in range(80):
        a, b = hi - g * (hi - lo), lo + g * (hi - lo)
        if R.log_likelihood(rows, ref, a) < R.log_likelihood(rows, ref, b):
            lo = a
        else:
            hi = b
    ll_ref = R.log_likelihood(rows, ref, (lo + hi) / 2)
    print("log-likelihood at the reference's ratings, bias %.2f: %.3f" % ((lo + hi) / 2, ll_ref))
    assert fit.log_likelihood >= ll_ref
    assert abs(R.log_likelihood(rows, fit.ratings, fit.bias) - fit.log_likelihood) < 1e-6 * abs(fit.log_likelihood)


def test_a_player_who_won_everything_needs_prior_draws():
    rows = [(0, 1, 5, 1, 4), (1, 0, 3, 2, 5), (2, 0, 6, 0, 0), (1, 2, 0, 0, 4), (0, 3, 7, 1, 2), (3, 1, 2, 2, 6), (3, 2, 0, 0, 2)]
    with pytest.raises(ValueError, match=r"player\(s\) 2 .*prior_draws"):
        R.fit_ratings(rows, anchor=3)
    fit = R.fit_ratings(rows, anchor=3, prior_draws=1)
    assert np.all(np.isfinite(fit.ratings)) and np.isfinite(fit.bias) and fit.max_gradient < 1e-6
    assert fit.ratings[2] == np.max(fit.ratings) and fit.ratings[3] == 0.0


def test_aggregate_counts_wins_draws_losses_per_ordered_pair():
    lines = ["0 1 1\n", "1 0 0.5\n", "0 1 0\n", "0 1 1\n", "2 0 0.5\n", "\n"]
    assert R.aggregate(lines) == [(0, 1, 2, 0, 1), (1, 0, 0, 1, 0), (2, 0, 0, 1, 0)]
    assert R.aggregate([((0, 1), 1.0), ((0, 1), 0.0)]) == [(0, 1, 1, 0, 1)]


@pytest.fixture
def golden_folder(tmp_path):
    with open(os.path.join(HERE, "golden", "rating_round.json")) as f:
        d = json.load(f)
    folder = str(tmp_path)
    for name, text in (("players.txt", d["players"]), ("ratings.txt", d["ratings"])):
        with open(os.path.join(folder, name), "w") as f:
            f.write(text)
    for k, text in enumerate(d["round_results"]):
        os.mkdir(os.path.join(folder, "round_%d" % k))
        with open(os.path.join(folder, "round_%d" % k, "results.txt"), "w") as f:
            f.write(text)
    return folder, d


def test_choose_matches_writes_the_reference_match_files(golden_folder):
    folder, d = golden_folder
    rf = os.path.join(folder, "round_2")
    os.mkdir(rf)
    parts = R.choose_matches(folder, d["num_games"], d["num_parts"], rf)
    assert sum(len(p) for p in parts) == 2 * d["num_games"]
    for i in range(d["num_parts"]):
        with open(os.path.join(rf, "matches_%d.txt" % i)) as f:
            assert f.read() == d["written"]["matches_%d.txt" % i]
    # the first line is the number of PICKS, as the reference writes it; every pick is two lines, and all of them are played
    with open(os.path.join(rf, "matches_0.txt")) as f:
        rows = f.read().splitlines()
    assert int(rows[0]) * 2 == len(rows) - 1 == len(parts[0])
    assert [tuple(int(v) for v in x.split()[:2]) for x in rows[1:]] == parts[0]


def test_performance_ratings_are_the_reference_ratings(golden_folder):
    folder, d = golden_folder
    got = R.performance_ratings(folder)
    want = [float(x) for x in d["written"]["ratings.txt"].split()]
    assert d["written"]["ratings.txt"] == d["folder_ratings_after"]
    assert len(got) == len(want) == 6
    assert np.max(np.abs(np.array(got) - np.array(want))) <= 1e-9
    assert got[5] == 0  # the random player


# ---- a round on the engine: two differing networks, the raw-policy player, the random player
def _round_folder(tmp_path, name):
    models = tmp_path / "models"
    if not models.exists():
        models.mkdir()
        for i, w in enumerate((nets.init_mlp12x100(3, bn_noise=True), nets.trained_like_mlp12x100(4))):
            run.save_model(str(models / ("m%d.npz" % i)), w, (np.zeros_like(w), np.zeros_like(w), 0), "mlp12x100")
    folder = str(tmp_path / name)
    assert R.setup(folder, model_paths=[str(models / "m0.npz"), str(models / "m1.npz")], max_searches=24, searches_per_eval=8) == 4
    return folder


def _tree(folder):
    out = {}
    for root, _, files in os.walk(folder):
        for f in files:
            with open(os.path.join(root, f), "rb") as fh:
                out[os.path.relpath(os.path.join(root, f), folder)] = fh.read()
    return out


ENGINE_KINDS = [pytest.param("emu", "f32", id="emu"), pytest.param("hip", "h3", marks=pytest.mark.gpu, id="hip")]


@pytest.mark.parametrize("engine,arith", ENGINE_KINDS)
def test_a_round_on_the_engine_and_its_resume(engine, arith, tmp_path, monkeypatch):
    """4 players, 6 picks played both ways in 2 parts; then the same folder from a call cut short after part 0 plus a
    resume: byte-equal (no file of the folder holds a time)"""
    L = cdll(engine)
    a = _round_folder(tmp_path, "a")
    assert R.read_players(a) == [(0, 24, 8, 3.0, 0.25, False), (1, 24, 8, 3.0, 0.25, False), (1, 1, 1, 3.0, 0.25, False),
                                 (-1, 24, 8, 3.0, 0.25, True)]
    assert R.play_round(a, 6, 2, seed=5, arith=arith, _cdll=L) == 0
    with open(os.path.join(a, "round_0", "results.txt")) as f:
        lines = f.read().splitlines()
    assert len(lines) == 12 and all(x.split()[2] in ("0", "0.5", "1") for x in lines)
    with open(os.path.join(a, "ratings.txt")) as f:
        ratings = [float(x) for x in f.read().split()]
    assert len(ratings) == 4 and np.all(np.isfinite(ratings)) and ratings[3] == 0
    assert R.current_round(a) == 1
    assert R.play_round(a, 6, 2, seed=5, arith=arith, _cdll=L) == 1  # the pairing now goes by round 0's scores

    class Cut(Exception):
        pass

    def cut(part):
        if part == 0:
            raise Cut()

    b = _round_folder(tmp_path, "b")
    with pytest.raises(Cut):
        R.play_round(b, 6, 2, seed=5, arith=arith, _cdll=L, _hook=cut)
    assert R.current_round(b) == 0 and os.path.exists(os.path.join(b, "round_0", "logs_0", "scores.txt"))
    assert R.play_round(b, 6, 2, seed=5, arith=arith, _cdll=L) == 0
    assert R.play_round(b, 6, 2, seed=5, arith=arith, _cdll=L) == 1
    assert _tree(a) == _tree(b)
    # [seed, round, part] reaches the generator the matches' seeds are drawn from
    from corintho_ai_amd.tourney import Tourney

    seen = []
    monkeypatch.setattr(Tourney, "set_seed", lambda self, seed, _real=Tourney.set_seed: (seen.append(seed), _real(self, seed))[1])
    c = _round_folder(tmp_path, "c")
    R.play_round(c, 6, 2, seed=6, arith=arith, _cdll=L)
    assert seen == [R.part_seed(6, 0, 0), R.part_seed(6, 0, 1)]
    assert len({R.part_seed(s_, r_, p_) for s_ in (5, 6) for r_ in (0, 1) for p_ in (0, 1)}) == 8
    assert _tree(a)["round_0/matches_0.txt"] == _tree(c)["round_0/matches_0.txt"]
    fit = R.write_gd_ratings(a, prior_draws=1)
    assert np.all(np.isfinite(fit.ratings)) and os.path.exists(os.path.join(a, "gd_ratings.txt"))


ENGINES_SEED = [pytest.param("emu", id="emu"), pytest.param("hip", marks=pytest.mark.gpu, id="hip")]


@pytest.mark.parametrize("engine", ENGINES_SEED)
def test_the_tournament_seed_decides_the_games(engine):
    """the same pairings under another set_seed are other games, under the same one the same: the random player's draws
    are in the traces"""
    from corintho_ai_amd.tourney import Tourney

    def play(seed):
        t = Tourney(1, "", trace=True, _cdll=cdll(engine))
        if seed is not None:
            t.set_seed(seed)
        t.addPlayer(0, 0, 8, 4, 1.0, 0.25, False)
        t.addPlayer(1, -1, 0, 0, 1.0, 0.25, True)
        for _ in range(3):
            t.addMatch(0, 1, False)
            t.addMatch(1, 0, False)
        t.set_net(0, 1, nets.init_mlp12x100(3, bn_noise=True))
        assert t.run()
        return [t.trace(i).tobytes() for i in range(6)]

    a, b, c = play(11), play(11), play(12)
    assert a == b and a != c and play(None) != a
    with pytest.raises(Exception, match="after the first addMatch"):
        t = Tourney(1, "", _cdll=cdll(engine))
        t.addPlayer(0, 0, 8, 4, 1.0, 0.25, False)
        t.addPlayer(1, -1, 0, 0, 1.0, 0.25, True)
        t.addMatch(0, 1, False)
        t.set_seed(3)


def test_no_anchor_is_a_clear_error(tmp_path):
    with pytest.raises(ValueError, match="no anchor"):
        R.fit_ratings([(0, 1, 1, 0, 1)], anchor=[])
    folder = str(tmp_path)
    with open(os.path.join(folder, "players.txt"), "w") as f:
        f.write("2\n0 8 4 1.0 0.25 0\n1 8 4 1.0 0.25 0\n")
    os.mkdir(os.path.join(folder, "round_0"))
    with open(os.path.join(folder, "round_0", "results.txt"), "w") as f:
        f.write("0 1 1\n1 0 0.5\n")
    with pytest.raises(ValueError, match="no random player"):
        R.write_gd_ratings(folder)
