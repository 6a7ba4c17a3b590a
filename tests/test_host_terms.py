"""The 16-bit operand terms the host packs for the split-precision kernels (csrc/nn_split.h split_terms, one copy for the
MLP and the residual CNN), through a tiny g++-compiled driver (its host part compiles under -DCO_EMU): bf16 terms sum back to
the value within the dropped term and keep a NaN a NaN; fp16 terms are numpy.float16's rounding, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _values():
    rng = np.random.default_rng(20240)
    v = (rng.standard_normal(4096) * np.exp2(rng.integers(-30, 31, 4096))).astype(np.float32)
    edge = np.array([0.0, -0.0, np.finfo(np.float32).max, 65504.0, 65520.0, 1e-40], np.float32)
    bits = np.concatenate([v.view(np.uint32), edge.view(np.uint32), np.array([0x7FFFFFFF], np.uint32)])  # NaN, mantissa all ones
    return bits


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("terms") / "split_terms_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DCO_EMU", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "split_terms_driver.cpp")])
    return exe


def _terms(exe, bits, nt, f16):
    text = "".join("%08x\n" % b for b in bits)
    out = subprocess.run([exe, str(nt), str(int(f16))], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
    t = np.array([[int(x, 16) for x in line.split()] for line in out.strip().split("\n")], np.uint16)
    assert t.shape == (len(bits), nt)
    return t


@pytest.mark.parametrize("nt", [2, 3])
def test_bf16_terms_sum_back_to_the_value(driver, nt):
    bits = _values()
    v = bits.view(np.float32).astype(np.float64)
    t = _terms(driver, bits, nt, False)
    f = (t.astype(np.uint32) << 16).view(np.float32).astype(np.float64)  # a bf16 is the upper half of a float32
    nan = np.isnan(v)
    assert nan.sum() == 1 and np.isnan(f[nan]).all(), "NaN stays NaN"
    ok = ~nan
    assert np.isfinite(f[ok]).all(), "a finite value has finite terms (the largest finite float too)"
    # A term is the nearest bf16 (8 significand bits) of what is left, so it leaves at most 2^-8 of it: after nt terms at most
    # 2^(-8 nt) |v| remains -- the size of the term that was dropped.  Below bf16's smallest normal the terms are multiples
    # of its subnormal quantum 2^-133 and half a quantum can remain.  The sum of the terms is exact in float64.
    left = np.abs(v[ok] - f[ok].sum(axis=1))
    bound = np.maximum(np.abs(v[ok]) * 2.0 ** (-8 * nt), 2.0 ** -134)
    worst = float((left / bound).max())
    print("bf16, %d terms: largest remainder / bound = %.4f" % (nt, worst))
    assert (left <= bound).all()
    if nt == 3:  # three bf16 terms hold float32's 24 significand bits: nothing is dropped above bf16's subnormals
        normal = np.abs(v[ok]) >= 2.0 ** -100
        assert (left[normal] == 0).all()
    # zeros keep their sign and leave nothing
    assert (t[bits == 0x00000000] == 0).all()
    assert (t[bits == 0x80000000][:, 0] == 0x8000).all() and (t[bits == 0x80000000][:, 1:] == 0).all()


@pytest.mark.parametrize("nt", [2, 3])
def test_f16_terms_are_numpy_float16_roundings(driver, nt):
    bits = _values()
    t = _terms(driver, bits, nt, True)
    v = bits.view(np.float32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(nt):  # the term is numpy's float16 of what is left, and what is left then is a float32 difference
            h = v.astype(np.float16)
            assert (t[:, i] == h.view(np.uint16)).all(), "term %d" % i
            v = v - h.astype(np.float32)
