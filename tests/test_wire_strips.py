"""The wire feeder's strip plan (trivy_amd/csrc/wire_strips.h), checked through
tsg_test_plan_wire_strips on sizes alone: no engine, no device.

The plan is compared with a restatement of its rules in Python (`model`), and
over random segment sizes, the strip sizes the engine and its tests use and 0
to 16 packers the properties every plan must have are checked on their own:
exact cover in order, aligned offsets, no strip longer than the configured one,
the uniform cut wherever the ramp is off or does not fit.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from trivy_amd import _lib

K64 = 65536
MIB = 1 << 20
BLOCK = 4096
MAX_STRIP = 1 << 30                      # kWireMaxStrip
STRIPS = [4096, K64, MIB, 64 * MIB, MAX_STRIP]


def _header_constant(name):
    """the ramp's tuning constants are the header's to set: read, not repeated here (retuning them needs no edit)"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trivy_amd", "csrc",
                            "wire_strips.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


ROUNDS, BACK, BACK_DIV = (_header_constant(k) for k in ("kWireRampRounds", "kWireRampBack", "kWireRampBackDiv"))


def plan(seg, strip, first, np_):
    n = ctypes.c_uint32()
    L = _lib.lib()
    cap = seg // strip + 64 + 40 * max(np_, 0)
    off = np.zeros(cap, np.uint64)
    ln = np.zeros(cap, np.uint64)
    _lib.check(L.tsg_test_plan_wire_strips(seg, strip, int(first), np_, off.ctypes.data, ln.ctypes.data, cap,
                                           ctypes.byref(n)))
    return off[:n.value].astype(np.int64), ln[:n.value].astype(np.int64)


def _run(a, b, step):
    o = np.arange(a, b, step, dtype=np.int64)
    return o, np.minimum(step, b - o)


def uniform(seg, strip):
    return _run(0, seg, strip)


def front_sizes(strip, np_):
    """the ramp's front: strip i of m is (i + 1) / m of a strip, down to a multiple of 64 KiB"""
    m = ROUNDS * np_
    return [max(K64, strip // K64 * (i + 1) // m * K64) for i in range(m)]


def ramp_min(strip, np_):
    """the shortest segment the ramp fits"""
    return sum(front_sizes(strip, np_)) + BACK * (strip // BACK_DIV)


def model(seg, strip, first, np_):
    if not (first and np_ > 0 and strip >= MIB and strip % MIB == 0 and seg >= ramp_min(strip, np_)):
        return uniform(seg, strip)
    fs = np.array(front_sizes(strip, np_), dtype=np.int64)
    front = int(fs.sum())
    back = (seg - BACK * (strip // BACK_DIV)) // K64 * K64
    parts = [(np.cumsum(fs) - fs, fs), _run(front, back, strip), _run(back, seg, strip // BACK_DIV)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _cases():
    rng = np.random.default_rng(0x57219)
    out = []
    for strip in STRIPS:
        # (log-uniform sizes: 4096-byte strips of an 8 GB segment would be two million entries per case)
        top = 33 if strip >= K64 else 27
        for _ in range(40):
            seg = int(2.0 ** rng.uniform(0, top))
            out.append((max(1, min(seg, (1 << 33) - 1)), strip, int(rng.integers(0, 17))))
        out.append(((1 << 33) - 1, max(strip, K64), 14))
        for np_ in (1, 14, 16):             # around the shortest segment the ramp fits
            edge = ramp_min(strip, np_)
            out += [(edge - 1, strip, np_), (edge, strip, np_), (edge + 1, strip, np_), (edge + K64 + 5, strip, np_)]
    return out


CASES = _cases()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_plan_matches_the_rules():
    ramped = 0
    for seg, strip, np_ in CASES:
        for first in (1, 0):
            off, ln = got = plan(seg, strip, first, np_)
            assert _same(got, model(seg, strip, first, np_)), (seg, strip, first, np_)
            # exact cover, in order
            assert off[0] == 0 and np.array_equal(off[1:], off[:-1] + ln[:-1]) and off[-1] + ln[-1] == seg
            assert ln.min() > 0 and ln.max() <= strip
            assert not (ln[:-1] % BLOCK).any()
            if strip % K64 == 0:
                assert not (off % K64).any(), (seg, strip, first, np_)
            is_uniform = _same(got, uniform(seg, strip))
            if not first or np_ == 0 or strip < MIB or seg < ramp_min(strip, np_):
                assert is_uniform, (seg, strip, first, np_)
            else:
                # the ramp: growing strips up to a whole one at the front, small ones at the back
                ramped += 1
                m = ROUNDS * np_
                assert (np.diff(ln[:m]) >= 0).all() and ln[0] <= max(K64, strip // m) and ln[m - 1] == strip
                assert ln[-BACK:].max() <= strip // BACK_DIV
                assert seg - off[-BACK] <= BACK * (strip // BACK_DIV) + K64
    assert ramped >= 20


def test_default_strip_plan():
    """config 2's first segment: 3.33 GB, 64 MiB strips, 14 packers"""
    seg, S = 3_333_333_333, 64 * MIB
    off, ln = plan(seg, S, 1, 14)
    m = ROUNDS * 14
    assert ln[:m].tolist() == [1024 * (i + 1) // m * K64 for i in range(m)]
    assert ln[0] == 1024 // m * K64 and ln[m - 1] == ln[m] == S
    back = (seg - BACK * (S // BACK_DIV)) // K64 * K64
    i = int(np.searchsorted(off, back))
    assert off[i] == back and (ln[i:-1] == S // BACK_DIV).all() and len(ln) - i in (BACK, BACK + 1)
    assert (ln[m:i - 1] == S).all() and ln[i - 1] <= S and ln[i - 1] % K64 == 0
    assert _same(plan(seg, S, 0, 14), uniform(seg, S))


@pytest.mark.parametrize("seg", [1, 5, K64 - 1, K64, K64 + 1, 524288, 524288 + 5, 2 * MIB + 12345])
def test_64k_cut_is_the_uniform_one(seg):
    """the GPU wire tests run 64 KiB strips and pin strip counts and wire bytes"""
    for first in (0, 1):
        for np_ in (0, 6, 14):
            off, ln = plan(seg, K64, first, np_)
            assert len(off) == -(-seg // K64)
            assert off.tolist() == [k * K64 for k in range(len(off))]
            assert ln[:-1].tolist() == [K64] * (len(off) - 1) and ln[-1] == seg - off[-1]


def test_bad_arguments():
    n = ctypes.c_uint32()
    L = _lib.lib()
    assert L.tsg_test_plan_wire_strips(100, 0, 1, 1, None, None, 0, ctypes.byref(n)) != 0
    off = np.zeros(2, np.uint64)
    assert L.tsg_test_plan_wire_strips(10 * K64, K64, 1, 1, off.ctypes.data, off.ctypes.data, 2, ctypes.byref(n)) != 0
    assert n.value == 10
