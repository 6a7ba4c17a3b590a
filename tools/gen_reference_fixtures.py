#!/usr/bin/env python3
"""Data the reference holds, committed under tests/golden/reference/ so that the tests that compare against it run
from this repository alone.  Paths below the output directory mirror the reference's own (corintho_ai/...):

    rating/results.txt, rating/tourney/players.txt   the reference's rating tournament (tests/test_reference_results.py)
    rating/gd_ratings.txt                            the ratings rating_gd.cpp recorded for them (tests/test_rating.py)
    rating/tflite_models/model_{0,51,93}.tflite      three TFLite checkpoints: first, middle, last in name order
                                                     (tests/test_tflite_import.py)
    model/variables.npz                              the Keras SavedModel's variables/: the index file, and the head of the
                                                     data shard that holds every layer variable with the shard's full length
                                                     (the optimizer's slots behind them are left out; tests/test_savedmodel_import.py)
    util_tables.npz                                  the four constant tables of cpp/include/util.h:85-702, parsed from the
                                                     header's text into arrays (tests/test_tables.py)

Files are copied byte for byte, except the SavedModel's data shard (above) and the header, of which only the table
values are kept.

usage: python tools/gen_reference_fixtures.py <reference checkout>
"""
import glob
import os
import re
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from corintho_ai_amd import savedmodel_import as SI  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference")
TFLITE = ("model_0.tflite", "model_51.tflite", "model_93.tflite")


def _ints(block):
    return [int(x) for x in re.findall(r"-?\d+", block)]


def util_tables(src):
    """the four tables of util.h as arrays: line_breakers as bits (column k = bit k of the 96-bit mask)"""
    s = src[src.index("line_breakers = {"):src.index("// Number of buckets")]
    strs = re.findall(r'bitset<kNumMoves>\(\s*((?:"[01]+"\s*)+)\)', s)
    bits = np.zeros((len(strs), 96), np.uint8)
    for idx, t in enumerate(strs):
        b = "".join(re.findall(r'"([01]+)"', t))
        assert len(b) == 96
        for k, ch in enumerate(b):  # bitset string: char k is bit 95-k
            bits[idx, 95 - k] = ch == "1"
    s = src[src.index("gamma_samples[kNumGammaBuckets] = {"):]
    s = s[s.index("{") + 1:s.index("};")]
    gamma = np.array([float(x) for x in re.findall(r"[-+0-9.e]+", s)]).astype(np.float32)
    s = src[src.index("space_symmetries[kNumSymmetries][kBoardSize] = {"):]
    sp = np.array(_ints(s[s.index("{"):s.index("};")]), np.int32).reshape(8, 16)
    s = src[src.index("move_symmetries[kNumSymmetries][kNumMoves] = {"):]
    mv = np.array(_ints(s[s.index("{"):s.index("};")]), np.int32).reshape(8, 96)
    return {"line_breakers_bits": bits, "gamma_samples": gamma, "space_symmetries": sp, "move_symmetries": mv}


def model_variables(d):
    """index bytes, the data shard up to the end of its last layer variable, and the shard's length"""
    with open(os.path.join(d, "variables.index"), "rb") as f:
        index = f.read()
    entries = SI.read_index(index)
    layers = [e for k, e in entries.items() if k.startswith("layer_with_weights-")]
    head = max(e["offset"] + e["size"] for e in layers)
    assert all(e["shard"] == 0 for e in entries.values())
    assert all(e["offset"] >= head for k, e in entries.items() if not k.startswith("layer_with_weights-"))
    with open(os.path.join(d, "variables.data-00000-of-00001"), "rb") as f:
        data = f.read()
    return {"index": np.frombuffer(index, np.uint8), "data_head": np.frombuffer(data[:head], np.uint8),
            "data_size": np.array(len(data), np.int64)}


def main(ref):
    base = os.path.join(ref, "corintho_ai")
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(base, "rating", "tflite_models", "model_*.tflite")))
    assert (names[0], names[len(names) // 2], names[-1]) == TFLITE, names
    files = ["rating/results.txt", "rating/gd_ratings.txt", "rating/tourney/players.txt"] + ["rating/tflite_models/" + n for n in TFLITE]
    for rel in files:
        dst = os.path.join(OUT, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(os.path.join(base, rel), dst)
    os.makedirs(os.path.join(OUT, "model"), exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "model", "variables.npz"), **model_variables(os.path.join(base, "model", "variables")))
    with open(os.path.join(base, "cpp", "include", "util.h")) as f:
        np.savez_compressed(os.path.join(OUT, "util_tables.npz"), **util_tables(f.read()))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
