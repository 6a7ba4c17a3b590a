#!/usr/bin/env python3
"""Measures the merging of duplicate positions (Fitter.merge_duplicates, csrc/nn_samples.hip) on one GPU, at the sizes
of a training run.  It plays fused self-play generations (--games, --searches, --spe, c_puct 3, epsilon 0.25: the
reference's toml/train.toml by default) with the initial weights of nets.init_* and, with --trained FILE.npz, one more
with those weights, and reports

  * samples before and after the merge, for each generation and for the window of all of them;
  * milliseconds of merge_duplicates on each of these sets: a host clock around the call (it ends synchronised),
    the set added anew before every repetition, best and median of --reps;
  * seconds of fit_resident (--epochs at --batch) on the first generation without and with the merge, in the same
    process, alternating, --fit-reps times; with --parent-lib LIB.so also the unmerged fit by that build of the
    library (the parent commit's, built with `python -m corintho_ai_amd.build --out LIB.so CSRC_DIR`);
  * best val_loss both ways, and the arena score (--arena games) of each fit's best weights against the initial ones.

With --symmetries every set is also canonicalized and merged up to the eight symmetries (Fitter.canonicalize,
merge_duplicates(symmetries=True)): the samples left, the milliseconds of canonicalize alone (the set added anew before
every repetition) and of the whole merge, and a third way of the fit, "merged up to symmetry".  --augmentation sets how
this library's fitter expands the packed rows in every fit (the parent's library knows only the reference's).

With --merge-only it stops after the merges of the first generation: the process to put under
`rocprofv3 --kernel-trace --stats` for the kernels' shares (tools/rocpd_summary.py reads the result).

    python tools/sample_merge_bench.py [--net rescnn4] [--trained tests/golden/trained_early.npz] [--out file.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, Trainer, _lib, nets  # noqa: E402
from corintho_ai_amd import run as R  # noqa: E402
from corintho_ai_amd.fit import Fitter, fit_resident, net_info  # noqa: E402
from corintho_ai_amd.samples_io import merge_duplicates_host  # noqa: E402


def fitter_on(lib, max_batch, net):
    """a Fitter served by another build of the library (one that may lack the newer entry points)"""
    f = Fitter.__new__(Fitter)
    f.net, f.num_weights, f._L, f._h, f.max_batch, f._data = net, net_info(net)[1], lib, C.c_void_p(), int(max_batch), None
    _lib.check(lib, lib.ca_fitter_create_net(0, int(net), f.max_batch, C.byref(f._h)))
    return f


def play(a, kind, weights, seed):
    t0 = time.perf_counter()
    t = Trainer(a.games, "", seed, a.searches, a.spe, 3.0, 0.25, 0, 1, False)
    try:
        t.set_net(kind, weights)
        assert t.run()
        sp, oc = t.export_samples()
    finally:
        t.close()
    return sp, oc, time.perf_counter() - t0


def time_merge(f, sp, oc, reps, **kw):
    ms, counts = [], None
    for _ in range(reps):
        f.clear_data()
        f.add_samples(sp, oc)
        t0 = time.perf_counter()
        counts = f.merge_duplicates(normalize=True, **kw)
        ms.append((time.perf_counter() - t0) * 1e3)
    return counts, ms


def time_canonicalize(f, sp, oc, reps):
    ms, moved = [], None
    for _ in range(reps):
        f.clear_data()
        f.add_samples(sp, oc)
        t0 = time.perf_counter()
        moved = f.canonicalize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return moved, ms


def largest_group(sp):
    keys = np.ascontiguousarray(sp[:, :70]).view(np.dtype((np.void, 280))).ravel()
    return int(np.unique(keys, return_counts=True)[1].max())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--net", default="mlp12x100", choices=sorted(R.NETS))
    ap.add_argument("--arith", default="h3")
    ap.add_argument("--games", type=int, default=25000)
    ap.add_argument("--searches", type=int, default=1600)
    ap.add_argument("--spe", type=int, default=16)
    ap.add_argument("--generations", type=int, default=3, help="generations of the window")
    ap.add_argument("--trained", help=".npz whose `weights` play one more generation (mlp12x100)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--learning-rate", type=float, default=0.001)
    ap.add_argument("--fit-reps", type=int, default=2)
    ap.add_argument("--arena", type=int, default=1600)
    ap.add_argument("--parent-lib")
    ap.add_argument("--symmetries", action="store_true", help="also canonicalize and merge up to the eight symmetries")
    ap.add_argument("--augmentation", default="reference", choices=("reference", "consistent"),
                    help="how this library's fitter expands the packed rows in the fits")
    ap.add_argument("--merge-only", action="store_true")
    ap.add_argument("--check-host", action="store_true", help="compare the first generation's merge with the host's, by bytes")
    ap.add_argument("--out")
    a = ap.parse_args()
    net, init = R.NETS[a.net]
    kind = R.PLAY_KINDS[(a.net, a.arith)]
    w0 = init(1)
    out = {"args": vars(a), "sets": [], "fits": []}

    sets = []
    for g in range(1 if a.merge_only else a.generations):
        sp, oc, secs = play(a, kind, w0, 101 + g)
        sets.append(("generation %d (initial weights)" % (g + 1), sp, oc))
        print("played generation %d: %d samples in %.2f s" % (g + 1, sp.shape[0], secs), flush=True)
    if len(sets) > 1:
        sets.append(("window of %d generations" % len(sets), np.concatenate([s[1] for s in sets]),
                     np.concatenate([s[2] for s in sets])))
    if a.trained and not a.merge_only:
        with np.load(a.trained) as z:
            wt = z["weights"]
        sp, oc, secs = play(a, kind, wt, 201)
        sets.append(("generation with %s" % os.path.basename(a.trained), sp, oc))
        print("played with %s: %d samples in %.2f s" % (a.trained, sp.shape[0], secs), flush=True)

    with Fitter(max_batch=a.batch, net=net) as f:
        time_merge(f, sets[0][1][:4096], sets[0][2][:4096], 1)  # the kernels' code objects
        if a.symmetries:
            time_canonicalize(f, sets[0][1][:4096], sets[0][2][:4096], 1)
        if a.augmentation != "reference":
            f.set_augmentation(a.augmentation)
        for name, sp, oc in sets:
            counts, ms = time_merge(f, sp, oc, a.reps)
            row = {"set": name, "before": counts[0], "after": counts[1], "largest_group": largest_group(sp),
                   "merge_ms_best": min(ms), "merge_ms_median": float(np.median(ms)), "merge_ms": ms}
            out["sets"].append(row)
            print("%-42s before %8d after %8d (%.1f %% duplicates), largest group %6d, merge %.2f ms best, %.2f median"
                  % (name, counts[0], counts[1], 100.0 * (1 - counts[1] / counts[0]), row["largest_group"], min(ms),
                     float(np.median(ms))), flush=True)
            if a.symmetries:
                moved, cms = time_canonicalize(f, sp, oc, a.reps)
                scounts, sms = time_merge(f, sp, oc, a.reps, symmetries=True)
                row.update(after_symmetries=scounts[1], moved=moved, canonicalize_ms_best=min(cms),
                           canonicalize_ms_median=float(np.median(cms)), merge_symmetries_ms_best=min(sms),
                           merge_symmetries_ms_median=float(np.median(sms)))
                print("%-42s up to symmetry: after %8d (%.1f %% duplicates), %d samples turned; canonicalize %.2f ms best, "
                      "%.2f median; canonicalize + merge %.2f ms best, %.2f median"
                      % ("", scounts[1], 100.0 * (1 - scounts[1] / scounts[0]), moved, min(cms), float(np.median(cms)), min(sms),
                         float(np.median(sms))), flush=True)
        if a.check_host:
            _, sp, oc = sets[0]
            f.clear_data()
            f.add_samples(sp, oc)
            n = f.merge_duplicates()[1]
            s, e, p = f.fetch_rows(8 * np.arange(n, dtype=np.int32))
            want = merge_duplicates_host(sp, oc)
            same = (np.concatenate([s, p], 1).tobytes() == want[0].tobytes() and e.tobytes() == want[1].tobytes()
                    and f.get_sample_weights().tobytes() == want[2].tobytes())
            out["equals_host"] = bool(same)
            print("the device's merge of generation 1 equals the host's by bytes: %s" % same, flush=True)
            assert same
            if a.symmetries:
                f.clear_data()
                f.add_samples(sp, oc)
                n = f.merge_duplicates(symmetries=True)[1]
                s, e, p = f.fetch_rows(8 * np.arange(n, dtype=np.int32))  # (row 8 i: symmetry 0, whatever the augmentation)
                want = merge_duplicates_host(sp, oc, symmetries=True)
                same = (np.concatenate([s, p], 1).tobytes() == want[0].tobytes() and e.tobytes() == want[1].tobytes()
                        and f.get_sample_weights().tobytes() == want[2].tobytes())
                out["equals_host_symmetries"] = bool(same)
                print("the device's merge up to symmetry of generation 1 equals the host's by bytes: %s" % same, flush=True)
                assert same
        if a.merge_only:
            return

        # the fit of the first generation, without and with the merge (and by the parent's library), alternating
        _, sp, oc = sets[0]
        ways = [("unmerged", f, False), ("merged", f, True)]
        if a.symmetries:
            ways.append(("merged up to symmetry", f, "symmetries"))
        if a.parent_lib:
            ways.append(("unmerged, parent library", fitter_on(_lib.declare(C.CDLL(os.path.abspath(a.parent_lib))), a.batch, net),
                         False))
        best = {}
        for rep in range(a.fit_reps):
            for name, be, merge in ways:
                be.clear_data()
                be.add_samples(sp, oc)
                t0 = time.perf_counter()
                if merge == "symmetries":
                    be.merge_duplicates(normalize=True, symmetries=True)
                elif merge:
                    be.merge_duplicates(normalize=True)
                t1 = time.perf_counter()
                res = fit_resident(be, w0, learning_rate=a.learning_rate, batch_size=a.batch, epochs=a.epochs,
                                   anneal_factor=0.5, patience=2, seed=7)
                t2 = time.perf_counter()
                row = {"way": name, "rep": rep, "rows": be.data_info()[0], "merge_s": t1 - t0 if merge else 0.0, "fit_s": t2 - t1,
                       "best_val_loss": min(res.history["val_loss"]), "best_epoch": res.best_epoch}
                out["fits"].append(row)
                best.setdefault(name, res.best_weights)
                print("fit %-26s rep %d: %9d rows, merge %.3f s, fit %.2f s, best val_loss %.4f (epoch %d)"
                      % (name, rep, row["rows"], row["merge_s"], row["fit_s"], row["best_val_loss"], res.best_epoch), flush=True)
        for name, be, _ in ways:
            if be is not f:
                continue
            t = Trainer(a.arena, "", 301, a.searches, a.spe, 3.0, 0.25, 0, 1, True)
            try:
                t.set_net(kind, w0, slot=0)
                t.set_net(kind, best[name], slot=1)
                assert t.run()
                out["arena_" + name] = t.score()
            finally:
                t.close()
            print("arena of the %s fit's best weights against the initial ones: %.4f" % (name, out["arena_" + name]), flush=True)
        for _, be, _ in ways:
            if be is not f:
                be.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
