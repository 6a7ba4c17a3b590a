#!/usr/bin/env python3
"""Grouped tournament rounds against the per-model path, and the grouped network kernel against its own per-model
launches (profiles/rating_round.md).

    python tools/rating_round_bench.py tourney [--models 95] [--matches 1024] [--searches 1600] [--spe 16] [--path grouped|per_model]
    python tools/rating_round_bench.py kernel  [--rows 4096] [--reps 50] [--net mlp12x100|rescnn4]

tourney: the reference's rating shape -- `models` checkpoints (95 seeds of nets.trained_like_mlp12x100: the committed
fixtures hold three of the reference's 95 TFLite files), each one player at `searches` searches, plus the raw-policy player
(the last model at one search) and the random player; `matches` matches between random pairs of players, each pair both
ways; mlp12x100 at f16x3.  One call plays the tournament once on one path and prints one JSON line: seconds, engine
rounds, launches, rows per network launch, the scores' sum (both paths play the same games).
kernel: the same rows through NetGroup at M = 1, 8 and 95 (kernel-only times from HIP events), against the ungrouped kernel
on the same rows split by model, one launch per model.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from corintho_ai_amd import NET_MLP12X100_H3, NET_RESCNN4_H3, Tourney, Trainer, nets  # noqa: E402
from corintho_ai_amd.net import NetGroup  # noqa: E402


def tourney(a):
    M = a.models
    weights = [nets.trained_like_mlp12x100(s) for s in range(M)]
    players = [(i, i, a.searches, a.spe, 3.0, 0.25, False) for i in range(M)]
    players.append((M, M - 1, 1, 1, 3.0, 0.25, False))
    players.append((M + 1, -1, a.searches, a.spe, 3.0, 0.25, True))
    rng = np.random.default_rng(1)
    t = Tourney(1, "")
    t.set_seed(7)
    for p in players:
        t.addPlayer(*p)
    for _ in range(a.matches // 2):
        x, y = (int(v) for v in rng.choice(len(players), 2, replace=False))
        t.addMatch(x, y, False)
        t.addMatch(y, x, False)
    for i, w in enumerate(weights):
        t.set_net(i, NET_MLP12X100_H3, w)
    if a.path == "grouped":
        t.set_grouped(True)
    else:
        t.set_exact_offsets(True)
    t.run(max_rounds=8)  # (networks built, kernels loaded)
    t0 = time.perf_counter()
    done = t.run()
    dt = time.perf_counter() - t0
    s = t.stats()
    out = {"path": a.path, "tourney_path": s["tourney_path"], "models": M, "players": len(players), "matches": t.num_matches(),
           "searches": a.searches, "spe": a.spe, "done": done, "seconds": round(dt, 3), "engine_rounds": s["iterations"] if a.path == "grouped" else None,
           "nn_launches": s["nn_launches"], "mcts_launches": s["mcts_launches"], "evals": s["evals"],
           "rows_per_nn_launch": round(s["evals"] / max(s["nn_launches"], 1), 1), "plies": s["plies"],
           "score_sum": float(sum(t.match_score(i) for i in range(t.num_matches())))}
    print(json.dumps(out), flush=True)


def kernel(a):
    rng = np.random.default_rng(2)
    n = a.rows
    states = np.zeros((n, 70), np.float32)
    states[:, :64] = rng.integers(0, 2, (n, 64))
    states[:, 64:] = rng.integers(0, 5, (n, 6)) * 0.25
    kind, make = (NET_RESCNN4_H3, nets.trained_like_rescnn4) if a.net == "rescnn4" else (NET_MLP12X100_H3, nets.trained_like_mlp12x100)
    weights = [make(s) for s in range(8)]
    weights = [weights[i % 8] for i in range(95)]  # (a model's weights cost what another's do: eight sets, repeated)
    tr = Trainer((n + 15) // 16, "", 1, 50, 16, 1.0, 0.25, 0, 1, False)
    tr.set_net(kind, weights[0])
    for M in (1, 8, 95):
        model_of_row = rng.integers(0, M, n).astype(np.int32)
        g = NetGroup(kind, weights[:M], max_rows=n)
        runs = [g.bench(states, model_of_row, a.reps) for _ in range(3)]
        group_ms, fwd_ms = min(r[0] for r in runs), min(r[1] for r in runs)
        # the ungrouped kernel on the same rows, one launch per model (every model's weights cost the same: slot 0's)
        per_model = sum(min(tr.net_bench(states[model_of_row == m], a.reps) for _ in range(3)) for m in range(M) if (model_of_row == m).any())
        print(json.dumps({"net": a.net, "M": M, "rows": n, "grouping_kernel_us": round(group_ms * 1e3, 2), "grouped_forward_us": round(fwd_ms * 1e3, 2),
                          "per_model_launches_us": round(per_model * 1e3, 2), "workgroups": len(g.tables()["wg"])}), flush=True)
        g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["tourney", "kernel"])
    ap.add_argument("--models", type=int, default=95)
    ap.add_argument("--matches", type=int, default=1024)
    ap.add_argument("--searches", type=int, default=1600)
    ap.add_argument("--spe", type=int, default=16)
    ap.add_argument("--path", default="grouped", choices=["grouped", "per_model"])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--net", default="mlp12x100", choices=["mlp12x100", "rescnn4"], help="kernel: the network, at f16x3")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    {"tourney": tourney, "kernel": kernel}[a.what](a)
