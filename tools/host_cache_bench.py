#!/usr/bin/env python3
"""The host-driven protocol with and without the evaluation cache (Trainer.set_host_cache), measured side by side.

The `compat` configuration of tools/run_configs.py run_compat -- 4096 games, 400 simulations, the caller's three arrays
page-locked, the caller's network through net_forward on the same GPU -- played in ONE process by two trainers of the
same games: one speaks the plain protocol (the baseline, whose code the cache does not touch), one has the cache on.
After a warm-up generation of each, generations alternate plain / cached on the same seeds; medians are reported for
  * rows handed to the caller against rows the games requested,
  * iterations (doIteration calls),
  * seconds per generation.
Networks: the bench's default (rescnn4, f16x3, random init) and mlp12x100 (f16x3) with the reference's last checkpoint,
tests/golden/trained_last.npz.  Prints one JSON line per network and a markdown table (profiles/host_cache.md).

    python tools/host_cache_bench.py [--games 4096] [--sims 400] [--reps 3] [--nets rescnn4h3,mlp12x100h3]
    --emu: the emulation build of the engine (no device; for checking the tool itself at toy sizes)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from corintho_ai_amd import NET_MLP12X100, NET_MLP12X100_H3, NET_RESCNN4_H3, Trainer, nets  # noqa: E402

SPE = 16


def network(name):
    if name == "rescnn4h3":
        return NET_RESCNN4_H3, nets.init_rescnn4(0), "rescnn4 f16x3, random init (the bench's default)"
    if name in ("mlp12x100h3", "mlp12x100"):  # (the float32 kind: the one network the emulation build has)
        w = np.load(os.path.join(ROOT, "tests", "golden", "trained_last.npz"))["weights"]
        return (NET_MLP12X100_H3 if name.endswith("h3") else NET_MLP12X100), w, \
            "mlp12x100 %s, tests/golden/trained_last.npz" % ("f16x3" if name.endswith("h3") else "float32")
    raise SystemExit("unknown network %r" % name)


class Player:
    """one trainer and the three arrays of main.pyx:132-134, allocated once and page-locked"""

    def __init__(self, G, S, kind, w, cached, cdll):
        self.t = Trainer(G, "", 12345, S, SPE, 1.0, 0.25, 0, 1, False, stagger=False, _cdll=cdll)
        self.t.set_net(kind, w)
        self.cached = cached
        if cached:
            self.t.set_host_cache(True)
        cap = G * SPE
        self.evals = np.zeros(cap, np.float32)
        self.probs = np.zeros((cap, 96), np.float32)
        self.gs = np.zeros((cap, 70), np.float32)
        self.pinned = self.t.pin(self.evals, self.probs, self.gs)
        self.first = True

    def generation(self, seed):
        t = self.t
        if not self.first:
            t.reset(seed)
        self.first = False
        t0 = time.perf_counter()
        iters, rows = 1, 0
        while not t.doIteration(self.evals, self.probs, -1):
            n = t.num_requests(-1)
            if n:  # (cached: 0 rows while games run = every row was served from the table)
                t.writeRequests(self.gs, -1)
                t.net_forward(self.gs[:n], out_evals=self.evals, out_probs=self.probs)
            iters += 1
            rows += n
        dt = time.perf_counter() - t0
        st = t.stats()
        return {"seconds": dt, "iterations": iters, "rows_handed": rows,
                "rows_requested": st["nn_rows"] if self.cached else rows, "score": t.score(), "evals": st["evals"]}


def measure(name, G, S, reps, cdll):
    kind, w, what = network(name)
    plain, cached = Player(G, S, kind, w, False, cdll), Player(G, S, kind, w, True, cdll)
    plain.generation(12345)  # warm-up of each (kernels, allocations, page-locking)
    cached.generation(12345)
    runs = {"plain": [], "cached": []}
    for r in range(reps):
        a = plain.generation(100 + r)
        b = cached.generation(100 + r)
        assert a["score"] == b["score"] and a["evals"] == b["evals"], "the two protocols played different generations"
        assert b["rows_requested"] == a["rows_handed"], (b["rows_requested"], a["rows_handed"])
        runs["plain"].append(a)
        runs["cached"].append(b)
    med = lambda which, key: statistics.median(x[key] for x in runs[which])  # noqa: E731
    rec = {"network": name, "weights": what, "games": G, "sims": S, "searches_per_eval": SPE, "generations_each": reps,
           "pinned_host_arrays": bool(plain.pinned and cached.pinned)}
    for which in ("plain", "cached"):
        rec[which] = {k: med(which, k) for k in ("seconds", "iterations", "rows_handed", "rows_requested")}
        rec[which]["games_per_s"] = G / rec[which]["seconds"]
        rec[which]["seconds_all"] = [round(x["seconds"], 4) for x in runs[which]]
    rec["row_share_handed"] = rec["cached"]["rows_handed"] / rec["cached"]["rows_requested"]
    rec["speedup"] = rec["plain"]["seconds"] / rec["cached"]["seconds"]
    plain.t.close()
    cached.t.close()
    return rec


def table(recs):
    out = ["| network | protocol | rows to the caller | rows requested | share | iterations | s / generation | games/s |",
           "|---|---|---:|---:|---:|---:|---:|---:|"]
    for r in recs:
        for which in ("plain", "cached"):
            x = r[which]
            out.append("| %s | %s | %d | %d | %.1f %% | %d | %.3f | %.0f |" %
                       (r["network"], which, x["rows_handed"], x["rows_requested"],
                        100.0 * x["rows_handed"] / max(x["rows_requested"], 1), x["iterations"], x["seconds"], x["games_per_s"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3, help="generations of each protocol after the warm-up (at least 3 for a figure)")
    ap.add_argument("--nets", default="rescnn4h3,mlp12x100h3")
    ap.add_argument("--emu", action="store_true")
    a = ap.parse_args()
    cdll = None
    if a.emu:
        from tests.emu import emulib

        cdll = emulib.load()
    recs = []
    for name in a.nets.split(","):
        rec = measure(name, a.games, a.sims, a.reps, cdll)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    print()
    print("%d games x %d simulations, %d searches per evaluation; medians of %d generations of each protocol, alternating, "
          "after one warm-up generation of each; host arrays page-locked: %s" %
          (a.games, a.sims, SPE, a.reps, all(r["pinned_host_arrays"] for r in recs)))
    print()
    print(table(recs), flush=True)


if __name__ == "__main__":
    main()
