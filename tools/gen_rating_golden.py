"""tests/golden/rating_round.json: what the reference's own rating round writes for a small made-up folder.

Runs write_games and write_ratings of the reference's corintho_ai/rating/round.py (in the checkout named on the command
line) on 6 players, one of them random, with a few dozen result lines in two earlier rounds, num_games 7 and
2 parts, and stores the inputs and every file the two functions wrote.  round.py imports `run` from its compiled tourney
module; these two functions never call it, so a stand-in module takes its place.  tests/test_rating.py reads the JSON only.

    python tools/gen_rating_golden.py <reference checkout>
"""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "rating_round.json")


def inputs():
    rng = np.random.default_rng(20260101)
    players = ["0 40 8 3.0 0.25 0", "1 40 8 3.0 0.25 0", "2 40 8 3.0 0.25 0", "3 40 8 3.0 0.25 0", "3 1 1 3.0 0.25 0", "-1 40 8 3.0 0.25 1"]
    strength = [0.0, 0.6, 1.1, 1.7, 0.2, -2.5]
    rounds = []
    for n in (26, 30):
        lines = []
        for _ in range(n):
            a, b = (int(v) for v in rng.choice(6, 2, replace=False))
            p = 1.0 / (1.0 + np.exp(-(strength[a] - strength[b] + 0.3)))
            u = rng.random()
            sc = "0.5" if u < 0.12 else ("1" if rng.random() < p else "0")
            lines.append("%d %d %s\n" % (a, b, sc))
        rounds.append("".join(lines))
    # (one pair with a perfect score one way and none the other)
    rounds[0] += "3 5 1\n5 3 0\n"
    ratings = "\n".join(["0"] * 6)
    return {"players": "6\n" + "\n".join(players) + "\n", "ratings": ratings, "round_results": rounds, "num_games": 7, "num_parts": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="a checkout of the reference (maxjiang216/corintho-ai)")
    a = ap.parse_args()
    sys.modules["tourney"] = types.SimpleNamespace(run=None)  # round.py: `from tourney import run`
    sys.path.insert(0, os.path.join(a.reference, "corintho_ai", "rating"))
    import round as ref_round  # noqa: A004 -- the reference's module name

    data = inputs()
    with tempfile.TemporaryDirectory() as folder:
        with open(os.path.join(folder, "players.txt"), "w") as f:
            f.write(data["players"])
        with open(os.path.join(folder, "ratings.txt"), "w") as f:
            f.write(data["ratings"])
        for k, text in enumerate(data["round_results"]):
            os.mkdir(os.path.join(folder, "round_%d" % k))
            with open(os.path.join(folder, "round_%d" % k, "results.txt"), "w") as f:
                f.write(text)
        rf = os.path.join(folder, "round_2")
        os.mkdir(rf)
        ref_round.write_games(6, data["num_games"], folder, rf, 0, data["num_parts"])
        ref_round.write_ratings(folder, rf)
        written = {}
        for name in sorted(os.listdir(rf)):
            with open(os.path.join(rf, name)) as f:
                written[name] = f.read()
        with open(os.path.join(folder, "ratings.txt")) as f:
            data["folder_ratings_after"] = f.read()
    data["written"] = written
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
    print("wrote %s: %s" % (os.path.normpath(OUT), ", ".join(written)))


if __name__ == "__main__":
    main()
