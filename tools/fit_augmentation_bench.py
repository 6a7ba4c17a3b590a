#!/usr/bin/env python3
"""One fit of a self-play generation per augmentation ("reference", "consistent": Fitter.set_augmentation) on one GPU,
at the sizes of tools/sample_merge_bench.py: a fused generation of --games games (--searches, --spe, c_puct 3, epsilon
0.25, seed 101, the initial weights nets.init_*(1)), then for each augmentation in turn

  * fit_resident (--epochs at --batch, learning rate --learning-rate, validation split 0.3, seed 7): seconds and the best
    val_loss;
  * the policy loss of the best weights on validation rows (every --stride th one, through Fitter.predict against the
    targets Fitter.fetch_rows gives under that augmentation), split into the rows of symmetries 2 and 6 and the rows of
    the other six;
  * the arena score (--arena games, seed 301) of the best weights against the initial ones.

    python tools/fit_augmentation_bench.py [--net rescnn4] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from corintho_ai_amd import Trainer  # noqa: E402
from corintho_ai_amd import run as R  # noqa: E402
from corintho_ai_amd.fit import Fitter, fit_resident, split_index  # noqa: E402


def policy_loss(f, rows, batch):
    """the cross-entropy of every row in `rows`, in float64 on the host"""
    out = np.zeros(rows.size, np.float64)
    for r0 in range(0, rows.size, batch):
        r = rows[r0:r0 + batch]
        logits = f.predict(r)[0].astype(np.float64)
        target = f.fetch_rows(r)[2].astype(np.float64)
        logits -= logits.max(axis=1, keepdims=True)
        out[r0:r0 + r.size] = -(target * (logits - np.log(np.exp(logits).sum(axis=1, keepdims=True)))).sum(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--net", default="mlp12x100", choices=sorted(R.NETS))
    ap.add_argument("--arith", default="h3")
    ap.add_argument("--games", type=int, default=25000)
    ap.add_argument("--searches", type=int, default=1600)
    ap.add_argument("--spe", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--learning-rate", type=float, default=0.001)
    ap.add_argument("--stride", type=int, default=5, help="every this many validation rows are predicted")
    ap.add_argument("--arena", type=int, default=1600)
    ap.add_argument("--out")
    a = ap.parse_args()
    net, init = R.NETS[a.net]
    kind = R.PLAY_KINDS[(a.net, a.arith)]
    w0 = init(1)
    out = {"args": vars(a), "fits": []}
    with Fitter(max_batch=a.batch, net=net) as f:
        t = Trainer(a.games, "", 101, a.searches, a.spe, 3.0, 0.25, 0, 1, False)
        try:
            t.set_net(kind, w0)
            assert t.run()
            n = f.add_trainer_samples(t)
        finally:
            t.close()
        rows = f.data_info()[0]
        valid = np.arange(split_index(rows, 0.3), rows, a.stride, dtype=np.int32)
        turned = np.isin(valid % 8, (2, 6))
        print("generation 1: %d samples, %d rows, %d validation rows predicted" % (n, rows, valid.size), flush=True)
        for augmentation in ("reference", "consistent"):
            f.set_augmentation(augmentation)
            t0 = time.perf_counter()
            res = fit_resident(f, w0, learning_rate=a.learning_rate, batch_size=a.batch, epochs=a.epochs, anneal_factor=0.5,
                               patience=2, seed=7)
            secs = time.perf_counter() - t0
            f.set_weights(res.best_weights)
            ce = policy_loss(f, valid, a.batch)
            row = {"augmentation": augmentation, "fit_s": secs, "best_val_loss": min(res.history["val_loss"]),
                   "best_epoch": res.best_epoch, "val_policy_loss": res.history["val_policy_loss"][res.best_epoch],
                   "policy_loss_symmetries_2_6": float(ce[turned].mean()), "policy_loss_other_six": float(ce[~turned].mean())}
            arena = Trainer(a.arena, "", 301, a.searches, a.spe, 3.0, 0.25, 0, 1, True)
            try:
                arena.set_net(kind, w0, slot=0)
                arena.set_net(kind, res.best_weights, slot=1)
                assert arena.run()
                row["arena"] = arena.score()
            finally:
                arena.close()
            out["fits"].append(row)
            print("%-10s fit %.2f s, best val_loss %.4f (epoch %d, policy %.4f); policy loss of the validation rows: "
                  "symmetries 2 and 6 %.4f, the other six %.4f; arena %.4f"
                  % (augmentation, secs, row["best_val_loss"], res.best_epoch, row["val_policy_loss"],
                     row["policy_loss_symmetries_2_6"], row["policy_loss_other_six"], row["arena"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
