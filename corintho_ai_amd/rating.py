"""Rating tournament for a run's models (the reference's corintho_ai/rating: round.py, rating_gd.cpp), the matches on the GPU.

    python -m corintho_ai_amd.rating --folder ratings --run my_run --rounds 5 --num_games 512

The folder keeps the reference's layout:

    players.txt          the count, then per player `model_id max_searches searches_per_eval c_puct epsilon random`
    models.txt           the file of model id i on line i (a generation's model.npz of a run, or a TFLite checkpoint)
    ratings.txt          one rating per player, after the last finished round
    current_round.txt    the round to play next
    round_k/matches_i.txt, logs_i/scores.txt, results.txt, ratings.txt
    gd_ratings.txt       (the CLI, after its last round) the maximum-likelihood ratings and the first-move bias

A round (round.py main): choose_matches picks the pairs whose score is least certain, play_round plays each part as one
Tourney on the device, one after the other (what bounds memory, as the reference's per-thread files do), and
performance_ratings iterates performance ratings to a fixed point.  fit_ratings is the model of rating_gd.cpp solved by
Newton's method instead of a million gradient steps.

Resume: every file goes through a temporary name and os.replace, current_round.txt last; a round_k that exists when round
k starts was cut short and is removed and replayed.  The seeds of a part's matches come from [seed, round, part] and the
ratings a round starts from are those of round_{k-1}, so a resumed folder equals an uninterrupted one.
"""
import argparse
import heapq
import math
import os
import shutil
import sys
from collections import namedtuple

import numpy as np

ELO = 400.0 / math.log(10.0)  # rating points per unit of the logistic model


# ---------------------------------------------------------------------------------------------------- files
def _write_text(path, text):
    tmp = path + ".tmp"
    with open(tmp, "w", encoding="utf-8") as f:
        f.write(text)
    os.replace(tmp, path)


def _read_lines(path):
    with open(path, encoding="utf-8") as f:
        return [x.strip() for x in f.read().splitlines() if x.strip()]


def read_players(folder):
    """[(model_id, max_searches, searches_per_eval, c_puct, epsilon, random)], the player id is the index"""
    rows = _read_lines(os.path.join(folder, "players.txt"))
    out = []
    for x in rows[1:1 + int(rows[0])]:
        v = x.split()
        out.append((int(v[0]), int(v[1]), int(v[2]), float(v[3]), float(v[4]), float(v[5]) == 1.0))
    return out


def current_round(folder):
    return int(_read_lines(os.path.join(folder, "current_round.txt"))[0])


def _round_folders(folder):
    """the finished rounds' folders (those with a results.txt), in round order"""
    out = []
    for item in os.listdir(folder):
        if item.startswith("round_") and item[6:].isdigit() and os.path.exists(os.path.join(folder, item, "results.txt")):
            out.append((int(item[6:]), os.path.join(folder, item)))
    return [p for _, p in sorted(out)]


def read_results(folder):
    """[((player1, player2), score of player1)] of every finished round"""
    out = []
    for rf in _round_folders(folder):
        for x in _read_lines(os.path.join(rf, "results.txt")):
            v = x.split()
            out.append(((int(v[0]), int(v[1])), float(v[2])))
    return out


def load_weights(path):
    """the mlp12x100 / rescnn4 weights of a generation's model.npz, or the mlp12x100 weights of a TFLite checkpoint"""
    if str(path).endswith(".tflite"):
        from .tflite_import import mlp12x100_from_tflite

        return "mlp12x100", np.ascontiguousarray(mlp12x100_from_tflite(path), dtype=np.float32)
    with np.load(path) as z:
        return str(z["net"]), np.ascontiguousarray(z["weights"], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------- setup
def setup(folder, run_dir=None, model_paths=None, *, max_searches=1600, searches_per_eval=16, c_puct=3.0, epsilon=0.25):
    """A new rating folder: one player per generation's model.npz of the run `run_dir` (or per file of `model_paths`), the
    raw-policy player (the last model at one search) and the random player, as the reference's players.txt has them;
    every rating 0, round 0."""
    if (run_dir is None) == (model_paths is None):
        raise ValueError("setup: either run_dir or model_paths")
    if run_dir is not None:
        model_paths, k = [], 0
        while os.path.exists(os.path.join(run_dir, "generations", "gen_%d" % k, "model.npz")):
            model_paths.append(os.path.abspath(os.path.join(run_dir, "generations", "gen_%d" % k, "model.npz")))
            k += 1
    model_paths = [str(p) for p in model_paths]
    if not model_paths:
        raise ValueError("setup: no models")
    os.makedirs(folder, exist_ok=True)
    if os.path.exists(os.path.join(folder, "current_round.txt")):
        raise ValueError("setup: %s holds a rating tournament already" % folder)
    n = len(model_paths)
    players = ["%d %d %d %s %s 0" % (i, max_searches, searches_per_eval, c_puct, epsilon) for i in range(n)]
    players.append("%d 1 1 %s %s 0" % (n - 1, c_puct, epsilon))
    players.append("-1 %d %d %s %s 1" % (max_searches, searches_per_eval, c_puct, epsilon))
    _write_text(os.path.join(folder, "models.txt"), "\n".join(model_paths) + "\n")
    _write_text(os.path.join(folder, "players.txt"), "%d\n%s\n" % (len(players), "\n".join(players)))
    _write_text(os.path.join(folder, "ratings.txt"), "\n".join("0" for _ in players))
    _write_text(os.path.join(folder, "current_round.txt"), "0")
    return len(players)


# ---------------------------------------------------------------------------------------------------- pairing
def _variance(n1, m1, n2, m2):
    """round.py:81-88: the variances of the Beta posteriors of both orders of a pair"""
    return (n1 + 1) * (m1 + 1) / ((n1 + m1 + 2) ** 2 * (n1 + m1 + 3)) + (n2 + 1) * (m2 + 1) / ((n2 + m2 + 2) ** 2 * (n2 + m2 + 3))


def choose_matches(folder, num_games, num_parts=1, round_folder=None):
    """round.py:91-205 write_games: wins and losses per ordered pair from every finished round, the pair of largest
    variance picked num_games times (each pick counted as its expected result before the next), every pick played both
    ways, the list dealt round-robin into matches_i.txt of `round_folder` (none: not written).  Returns the parts' match
    lists [[(player1, player2), ...], ...].  The files are the reference's byte for byte: their first line counts the
    PICKS, each of which is two lines -- the reference's own reader (tourney.pyx:95-97) therefore plays the first half of a
    file only; play_round plays every line."""
    num_players = len(read_players(folder))
    scores = {}
    for pair, sc in read_results(folder):
        s = scores.setdefault(pair, [0, 0])  # wins, losses
        if sc == 0:
            s[1] += 1
        elif sc == 0.5:
            s[0] += 0.5
            s[1] += 0.5
        else:
            s[0] += 1
    heap = []
    for p1 in range(num_players):
        for p2 in range(p1 + 1, num_players):
            n1, m1 = scores.get((p1, p2), (0, 0))
            n2, m2 = scores.get((p2, p1), (0, 0))
            heap.append((-1 * _variance(n1, m1, n2, m2), ((p1, p2), (n1, m1, n2, m2))))
    heapq.heapify(heap)
    picks = []
    for _ in range(num_games):
        _, item = heapq.heappop(heap)
        picks.append(item[0])
        n1, m1, n2, m2 = item[1]
        # (as the reference: the loss count is updated with the win count already updated)
        n1 += n1 / (n1 + m1) if n1 + m1 > 0 else 0.5
        m1 += m1 / (n1 + m1) if n1 + m1 > 0 else 0.5
        n2 += n2 / (n2 + m2) if n2 + m2 > 0 else 0.5
        m2 += m2 / (n2 + m2) if n2 + m2 > 0 else 0.5
        heapq.heappush(heap, (-1 * _variance(n1, m1, n2, m2), (item[0], (n1, m1, n2, m2))))
    parts = []
    for i in range(num_parts):
        mine = picks[i::num_parts]
        parts.append([m for a, b in mine for m in ((a, b), (b, a))])
        if round_folder is not None:
            text = "%d\n" % len(mine) + "".join("%d\t%d\t0\n%d\t%d\t0\n" % (a, b, b, a) for a, b in mine)
            _write_text(os.path.join(round_folder, "matches_%d.txt" % i), text)
    return parts


# ---------------------------------------------------------------------------------------------------- performance ratings
def _performance(score, opponents):
    """round.py:276-297: the rating at which the expected score against `opponents` is `score`, by bisection to 0.1"""
    lo, hi = -10000, 20000
    while hi - lo > 0.1:
        mid = (hi + lo) / 2
        expected = sum([1 / (1 + 10 ** ((o - mid) / 400)) for o in opponents]) / len(opponents)
        if expected < score:
            lo = mid
        else:
            hi = mid
    return lo


def performance_ratings(folder, seed_ratings=None):
    """round.py:300-386 write_ratings: every player's performance rating against the current ratings of its opponents,
    over the games of every finished round, iterated until the largest change is <= 1; random players stay at 0, a
    perfect score counts a quarter point less, a player without a point is 0.  seed_ratings: where the iteration starts
    (none: the folder's ratings.txt).  Returns the list of ratings."""
    if seed_ratings is None:
        seed_ratings = [float(x) for x in _read_lines(os.path.join(folder, "ratings.txt"))]
    randomness = [p[5] for p in read_players(folder)]
    players = {i: ((0, True) if randomness[i] else (r, False)) for i, r in enumerate(seed_ratings)}
    games = {}
    for (p1, p2), sc in read_results(folder):
        games.setdefault(p1, []).append((p2, sc))
        games.setdefault(p2, []).append((p1, 1 - sc))
    delta = 999999
    while delta > 1:
        new, delta = {}, 0
        for player, (rating, is_random) in players.items():
            if is_random:
                new[player] = (0, True)
            elif player not in games:
                new[player] = (rating, False)
            else:
                opponents = [players[o][0] for o, _ in games[player]]
                score = sum([sc for _, sc in games[player]])
                if score == 0:
                    r = 0
                else:
                    if score == len(games[player]):
                        score -= 0.25
                    r = _performance(score / len(opponents), opponents)
                new[player] = (r, False)
                delta = max(delta, abs(r - rating))
        players = new
    return [players[i][0] for i in range(len(seed_ratings))]


def _ratings_text(ratings):
    return "\n".join("%s" % r for r in ratings)


# ---------------------------------------------------------------------------------------------------- the maximum-likelihood fit
FitResult = namedtuple("FitResult", "ratings bias log_likelihood max_gradient iterations")


def aggregate(results):
    """score lines -> the rows of rating/results.txt: [(player1, player2, wins, draws, losses)] of player1, who moves
    first, per ordered pair in order of first appearance.  results: lines `p1 p2 score`, or ((p1, p2), score) pairs."""
    rows = {}
    for x in results:
        if isinstance(x, str):
            v = x.split()
            if not v:
                continue
            pair, sc = (int(v[0]), int(v[1])), float(v[2])
        else:
            pair, sc = (int(x[0][0]), int(x[0][1])), float(x[1])
        r = rows.setdefault(pair, [0, 0, 0])
        r[0 if sc == 1.0 else 1 if sc == 0.5 else 2] += 1
    return [(a, b, w, d, l) for (a, b), (w, d, l) in rows.items()]


def _matchup_arrays(matchups):
    m = np.asarray([tuple(r) for r in matchups], dtype=np.float64).reshape(-1, 5)
    return m[:, 0].astype(np.int64), m[:, 1].astype(np.int64), m[:, 2] + 0.5 * m[:, 3], m[:, 2] + m[:, 3] + m[:, 4]


def log_likelihood(matchups, ratings, bias):
    """the log-likelihood of rating_gd.cpp at `ratings` and `bias` (both in Elo): sum over the rows of
    s lin - n log(1 + exp(lin)), lin = (r1 - r2 + b) ln 10 / 400, s = wins + draws / 2"""
    p1, p2, s, n = _matchup_arrays(matchups)
    r = np.asarray(ratings, np.float64) / ELO
    lin = r[p1] - r[p2] + bias / ELO
    return float(np.sum(s * lin - n * np.logaddexp(0.0, lin)))


def fit_ratings(matchups, anchor, prior_draws=0, num_players=None):
    """The model of rating_gd.cpp: P(the first player scores) = sigmoid(r1 - r2 + b) with one first-move bias b, a draw
    half a win, solved as a float64 Newton iteration on the concave log-likelihood with the players of `anchor` (an index
    or several) fixed at 0.  matchups: rows (player1, player2, wins, draws, losses).  Returns FitResult(ratings in Elo --
    nan for a player without games --, bias in Elo, log-likelihood, largest gradient component, iterations).
    A player who won or lost every game has no finite maximum: ValueError naming them; prior_draws adds that many
    virtual draws each way between every player and the anchor, which makes every maximum finite."""
    anchors = [int(anchor)] if np.isscalar(anchor) else [int(a) for a in anchor]
    if not anchors:
        raise ValueError("fit_ratings: no anchor -- one player or more must be fixed at 0 (the random player, as a rule)")
    p1, p2, s, n = _matchup_arrays(matchups)
    N = int(num_players if num_players is not None else max(p1.max(), p2.max(), max(anchors)) + 1)
    played = np.zeros(N)
    won = np.zeros(N)
    np.add.at(played, p1, n), np.add.at(played, p2, n)
    np.add.at(won, p1, s), np.add.at(won, p2, n - s)
    free = [i for i in range(N) if i not in anchors and played[i] > 0]
    if prior_draws > 0:
        a = anchors[0]
        extra = [(i, a, 0, prior_draws, 0) for i in free] + [(a, i, 0, prior_draws, 0) for i in free]
        q1, q2, qs, qn = _matchup_arrays(extra)
        p1, p2, s, n = np.concatenate([p1, q1]), np.concatenate([p2, q2]), np.concatenate([s, qs]), np.concatenate([n, qn])
    else:
        stuck = [i for i in free if won[i] == 0 or won[i] == played[i]]
        if stuck:
            raise ValueError("fit_ratings: player(s) %s won or lost every game, the likelihood has no finite maximum for them; "
                             "prior_draws=1 adds a virtual draw each way against the anchor" % ", ".join(str(i) for i in stuck))
    col = -np.ones(N, np.int64)
    col[free] = np.arange(len(free))
    K = len(free) + 1  # the free ratings, then b
    c1, c2 = col[p1], col[p2]

    def parts(x):
        r = np.zeros(N)
        r[free] = x[:-1]
        lin = r[p1] - r[p2] + x[-1]
        ll = float(np.sum(s * lin - n * np.logaddexp(0.0, lin)))
        sig = 1.0 / (1.0 + np.exp(-lin))
        return ll, s - n * sig, n * sig * (1.0 - sig)

    def gradient(g):
        out = np.zeros(K)
        np.add.at(out, c1[c1 >= 0], g[c1 >= 0])
        np.add.at(out, c2[c2 >= 0], -g[c2 >= 0])
        out[-1] = g.sum()
        return out

    x = np.zeros(K)
    ll, g, h = parts(x)
    grad = gradient(g)
    it = 0
    while np.max(np.abs(grad)) > 1e-10 and it < 200:
        H = np.zeros((K, K))
        # d lin / d x: +1 at player1's column, -1 at player2's, +1 at b
        for ca, sa in ((c1, 1.0), (c2, -1.0), (np.full(len(h), K - 1), 1.0)):
            for cb, sb in ((c1, 1.0), (c2, -1.0), (np.full(len(h), K - 1), 1.0)):
                ok = (ca >= 0) & (cb >= 0)
                np.add.at(H, (ca[ok], cb[ok]), sa * sb * h[ok])
        try:
            step = np.linalg.solve(H, grad)
        except np.linalg.LinAlgError as e:
            raise ValueError("fit_ratings: the games do not determine the ratings (%s); try prior_draws=1" % e) from e
        t = 1.0
        while True:  # (concave: a full step almost always; halved while it does not improve)
            ll2, g2, h2 = parts(x + t * step)
            if ll2 >= ll - 1e-12 * abs(ll) or t < 1e-6:
                break
            t *= 0.5
        x, ll, g, h = x + t * step, ll2, g2, h2
        grad = gradient(g)
        it += 1
        if not np.all(np.isfinite(x)) or np.max(np.abs(x)) > 1e3:
            raise ValueError("fit_ratings: the ratings diverge, the likelihood has no finite maximum; try prior_draws=1")
    ratings = np.full(N, np.nan)
    ratings[anchors] = 0.0
    ratings[free] = x[:-1] * ELO
    return FitResult(ratings, float(x[-1] * ELO), ll, float(np.max(np.abs(grad))), it)


# ---------------------------------------------------------------------------------------------------- a round on the device
from . import trainer as _T  # noqa: E402

PLAY_KINDS = {("mlp12x100", "f32"): _T.NET_MLP12X100, ("mlp12x100", "x3"): _T.NET_MLP12X100_X3, ("mlp12x100", "x6"): _T.NET_MLP12X100_X6,
              ("mlp12x100", "h3"): _T.NET_MLP12X100_H3, ("rescnn4", "f32"): _T.NET_RESCNN4, ("rescnn4", "x3"): _T.NET_RESCNN4_X3,
              ("rescnn4", "x6"): _T.NET_RESCNN4_X6, ("rescnn4", "h3"): _T.NET_RESCNN4_H3}
# grouped rounds by default: measured 34 x faster than the per-model path at 95 models, 4.8 x at 8 (profiles/rating_round.md)
GROUPED_DEFAULT = True


def part_seed(seed, round_index, part):
    """the seed of the generator a part's matches draw their seeds from"""
    return int(np.random.default_rng([seed, round_index, part]).integers(2 ** 32))


def play_part(folder, round_folder, part, matches, *, seed, round_index, arith="h3", grouped=GROUPED_DEFAULT, device=0, weights=None,
              _cdll=None):
    """one part of a round: its matches as one Tourney on the device, the scores to logs_<part>/scores.txt"""
    from .tourney import Tourney

    players = read_players(folder)
    models = _read_lines(os.path.join(folder, "models.txt"))
    weights = {} if weights is None else weights
    t = Tourney(1, "", device=device, _cdll=_cdll)
    try:
        t.set_seed(part_seed(seed, round_index, part))
        for pid, p in enumerate(players):
            t.addPlayer(pid, *p)
        for a, b in matches:
            t.addMatch(a, b, False)
        for mid in sorted({players[p][0] for m in matches for p in m if players[p][0] >= 0}):
            if mid not in weights:
                weights[mid] = load_weights(models[mid])
            net, w = weights[mid]
            t.set_net(mid, PLAY_KINDS[(net, arith)], w)
        if grouped:
            t.set_grouped(True)
        else:
            t.set_exact_offsets(True)  # (both paths play the same games)
        t.run()
        logs = os.path.join(round_folder, "logs_%d" % part)
        os.makedirs(logs, exist_ok=True)
        tmp = os.path.join(logs, "scores.txt.tmp")
        t.writeScores(tmp)
        os.replace(tmp, os.path.join(logs, "scores.txt"))
        return t.stats()
    finally:
        t.close()


def play_round(folder, num_games, num_parts=1, *, seed=0, arith="h3", grouped=GROUPED_DEFAULT, device=0, _cdll=None, _hook=None):
    """round.py main: the round current_round.txt names -- pairings, the parts one after the other on the device,
    results.txt, the new ratings, and current_round.txt last.  _hook(part) is called after each part (tests)."""
    k = current_round(folder)
    rf = os.path.join(folder, "round_%d" % k)
    if os.path.exists(rf):  # cut short: its matches are replayed from their seeds
        shutil.rmtree(rf)
    os.mkdir(rf)
    parts = choose_matches(folder, num_games, num_parts, rf)
    weights = {}
    for i, matches in enumerate(parts):
        if matches:
            play_part(folder, rf, i, matches, seed=seed, round_index=k, arith=arith, grouped=grouped, device=device, weights=weights,
                      _cdll=_cdll)
        else:
            os.makedirs(os.path.join(rf, "logs_%d" % i), exist_ok=True)
            _write_text(os.path.join(rf, "logs_%d" % i, "scores.txt"), "")
        if _hook is not None:
            _hook(i)
    results = []
    for i in range(num_parts):
        with open(os.path.join(rf, "logs_%d" % i, "scores.txt"), encoding="utf-8") as f:
            results.extend(f.readlines())
    _write_text(os.path.join(rf, "results.txt"), "".join(results))
    # the iteration starts from the ratings of the round before, not from a ratings.txt a cut-short round may have replaced
    prev = os.path.join(folder, "round_%d" % (k - 1), "ratings.txt")
    start = [float(x) for x in _read_lines(prev)] if k > 0 else [0.0] * len(read_players(folder))
    text = _ratings_text(performance_ratings(folder, start))
    _write_text(os.path.join(rf, "ratings.txt"), text)
    _write_text(os.path.join(folder, "ratings.txt"), text)
    _write_text(os.path.join(folder, "current_round.txt"), str(k + 1))
    return k


def write_gd_ratings(folder, prior_draws=0):
    """gd_ratings.txt: the maximum-likelihood ratings of every player over all finished rounds, random players fixed
    at 0, and the first-move bias on a last line `bias <b>`"""
    players = read_players(folder)
    anchors = [i for i, p in enumerate(players) if p[5]]
    if not anchors:
        raise ValueError("write_gd_ratings: players.txt of %s has no random player to fix at 0; call fit_ratings with an anchor of your choice"
                         % folder)
    fit = fit_ratings(aggregate(read_results(folder)), anchors, prior_draws, num_players=len(players))
    _write_text(os.path.join(folder, "gd_ratings.txt"), "".join("%s\n" % r for r in fit.ratings) + "bias %s\n" % fit.bias)
    return fit


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m corintho_ai_amd.rating", description=__doc__.split("\n")[0])
    ap.add_argument("--folder", required=True, help="the rating folder (created by the first call)")
    ap.add_argument("--run", default=None, help="a run directory of corintho_ai_amd.run: one player per generation")
    ap.add_argument("--models", nargs="*", default=None, help="model files instead: model.npz or TFLite checkpoints")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--num_games", type=int, default=512, help="pairs picked per round; each is played both ways")
    ap.add_argument("--num_parts", type=int, default=1, help="tournaments a round is split into, played one after the other")
    ap.add_argument("--max_searches", type=int, default=1600)
    ap.add_argument("--searches_per_eval", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--arith", default="h3", help="arithmetic of the networks: h3, f32, x6 or x3")
    ap.add_argument("--per_model", action="store_true", help="one launch per model id and round instead of grouped rounds")
    ap.add_argument("--prior_draws", type=float, default=0.0, help="virtual draws against the random player in gd_ratings.txt")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if not os.path.exists(os.path.join(a.folder, "current_round.txt")):
        setup(a.folder, run_dir=a.run, model_paths=a.models or None, max_searches=a.max_searches, searches_per_eval=a.searches_per_eval)
    for _ in range(a.rounds):
        k = play_round(a.folder, a.num_games, a.num_parts, seed=a.seed, arith=a.arith, grouped=not a.per_model, device=a.device)
        print("round %d done" % k, flush=True)
    try:
        fit = write_gd_ratings(a.folder, a.prior_draws)
        print("gd_ratings.txt: first-move bias %.2f Elo, log-likelihood %.3f" % (fit.bias, fit.log_likelihood))
    except ValueError as e:
        print("gd_ratings.txt not written: %s" % e, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
