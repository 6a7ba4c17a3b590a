"""The generated constant tables: digests, and value-for-value equality with the tables of the reference header
(corintho_ai/cpp/include/util.h:85-702), whose values tests/golden/reference/util_tables.npz holds
(tools/gen_reference_fixtures.py)."""
import json
import os

import numpy as np
import pytest

from tests.conftest import REFERENCE
from tools import gen_tables as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables():
    return gt.build_all()


@pytest.fixture(scope="module")
def reference_tables():
    with np.load(os.path.join(REFERENCE, "util_tables.npz")) as z:
        return {k: z[k] for k in z.files}


def test_digests_match_golden(tables):
    with open(os.path.join(ROOT, "tests/golden/tables.json")) as f:
        golden = json.load(f)
    assert gt.digests(*tables) == golden


def test_committed_inc_files_are_current(tables):
    text = gt.emit(*tables)
    for rel in ("corintho_ai_amd/csrc/tables.inc", "oracle/tables.inc"):
        with open(os.path.join(ROOT, rel)) as f:
            assert f.read() == text, rel + " is stale: run tools/gen_tables.py"


def test_symmetries_are_permutations_and_group(tables):
    _, _, sp, mv = tables
    for k in range(8):
        assert sorted(sp[k]) == list(range(16))
        assert sorted(mv[k]) == list(range(96))
    assert list(sp[0]) == list(range(16)) and list(mv[0]) == list(range(96))
    # closed under composition
    rows = {tuple(r) for r in sp}
    for a in sp:
        for b in sp:
            assert tuple(a[b]) in rows


def test_gamma_table_shape(tables):
    gm = tables[1]
    assert gm.dtype == np.float32 and gm.shape == (1024,)
    assert np.all(np.diff(gm) > 0)
    assert abs(float(gm.astype(np.float64).mean()) - 0.3) < 1e-6  # E[Gamma(0.3,1)] = 0.3


def test_line_breakers_equal_reference(tables, reference_tables):
    bits = reference_tables["line_breakers_bits"]
    assert bits.shape == (102, 96)
    for idx, row in enumerate(bits):
        m = 0
        for k in range(96):  # column k: bit k of the 96-bit mask
            if row[k]:
                m |= 1 << k
        assert m == tables[0][idx], "line %d" % idx


def test_gamma_samples_equal_reference(tables, reference_tables):
    ref = reference_tables["gamma_samples"]
    assert ref.dtype == np.float32 and ref.shape == (1024,)
    assert np.array_equal(ref.view(np.uint32), tables[1].view(np.uint32))


def test_symmetries_equal_reference(tables, reference_tables):
    sp = reference_tables["space_symmetries"]
    mv = reference_tables["move_symmetries"]
    assert sp.shape == (8, 16) and mv.shape == (8, 96)
    assert np.array_equal(sp, tables[2])
    assert np.array_equal(mv, tables[3])
