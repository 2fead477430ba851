"""Where Engine::scan cuts a batch (trivy_amd/csrc/segments.h, plan_segments),
checked on the offsets array alone through tsg_test_plan_segments: no engine,
no device.  The cuts decide every step time in the README (3 x 3.33 GB for
config 2, the halving tail of dense batches, the 10 % / 8 % resident pieces);
the GPU tests only see `pieces >= N`.

The exact cuts restate the rules by hand: upload targets are the first file
boundary at or past `rest / ceil(rest / segment)` (balanced), `segment` (full)
or `rest / 2` while that is >= segment_min (geometric: dense batches, or a
total under two segments); resident targets are the first boundary at or past
the shares first, first + mid * k / nmid, ..., 1 - last of the total."""
import ctypes
import random

import numpy as np
import pytest

from trivy_amd import _lib

MB = 1 << 20
# the engine's defaults (SegmentPolicy in segments.h; kDenseFilesPerGB)
DEFAULTS = dict(pieces=5, first_piece=0.1, first_piece_few=0.2, last_piece=0.08, min_piece=256 * MB,
                segment=4 << 30, segment_min=64 * MB, balanced=1, dense_files_per_gb=8000.0)


def plan(sizes, resident=False, base=0, paths=True, **policy):
    """-> (segments as dicts, each with its rebased offsets under 'off')"""
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(sizes, np.uint64))
    pol = _lib.TsgSegmentPolicy(**{**DEFAULTS, **policy})
    cap = len(sizes)
    out = (_lib.TsgSegmentInfo * cap)()
    nout = ctypes.c_uint32()
    reb = np.zeros(len(sizes) + 2 * cap, np.uint64)
    _lib.check(_lib.lib().tsg_test_plan_segments(off.ctypes.data, len(sizes), int(resident), base, int(paths),
                                                  ctypes.byref(pol), out, cap, ctypes.byref(nout),
                                                  reb.ctypes.data, len(reb)))
    segs, r = [], 0
    for s in out[:nout.value]:
        d = {k: getattr(s, k) for k, _ in s._fields_}
        d["off"] = [int(x) for x in reb[r:r + s.nfiles + 1]]
        r += s.nfiles + 1
        segs.append(d)
    return segs


def cuts(segs):
    return [s["f0"] for s in segs] + [segs[-1]["f0"] + segs[-1]["nfiles"] - segs[-1]["lead"]]


def check_invariants(sizes, segs, resident, base, paths=True):
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    c = cuts(segs)
    assert c[0] == 0 and c[-1] == len(sizes), c
    assert all(a < b for a, b in zip(c, c[1:])), c          # strictly increasing: every segment has a file
    assert sum(s["bytes"] for s in segs) == off[-1]
    for k, s in enumerate(segs):
        a, b = c[k], c[k + 1]
        assert s["b0"] == off[a] and s["bytes"] == off[b] - off[a]
        assert s["nfiles"] == b - a + s["lead"] and s["nfiles"] - s["lead"] >= 1
        delta = (base + s["b0"]) % 256 if resident and k > 0 else 0
        assert s["lead"] == (1 if delta and paths else 0), (k, delta, s)
        lead_bytes = delta if s["lead"] else 0
        # rebased offsets: from 0 to the segment's bytes, the lead's bytes first
        assert s["off"][0] == 0 and s["off"][-1] == s["bytes"] + lead_bytes
        assert s["off"][s["lead"]:] == [o - off[a] + lead_bytes for o in off[a:b + 1]]
        if resident:
            assert s["d_data"] == base + s["b0"] - lead_bytes
            if k > 0 and paths:
                assert s["d_data"] % 256 == 0               # (base + b0 - lead_delta) % 256 == 0


UPLOAD = [
    ("balanced thirds", [MB] * 10, dict(segment=4 * MB, segment_min=MB), [0, 4, 7, 10]),
    ("full segments", [MB] * 10, dict(segment=4 * MB, segment_min=MB, balanced=0), [0, 4, 8, 10]),
    ("halving tail", [MB] * 10, dict(segment=8 * MB, segment_min=MB), [0, 5, 8, 9, 10]),
    ("dense", [64 << 10] * 400, dict(segment=4 * MB, segment_min=MB), [0, 64, 128, 192, 256, 320, 360, 380, 400]),
    ("file larger than a segment", [9 * MB, MB, MB], dict(segment=4 * MB, segment_min=MB), [0, 1, 3]),
    ("one large file", [5 * MB], dict(segment=4 * MB), [0, 1]),
    ("empty files", [0, 3 * MB, 0, 0, 3 * MB, 0, 3 * MB, 0], dict(segment=4 * MB, segment_min=MB), [0, 2, 5, 8]),
]
RESIDENT = [
    ("defaults", [MB] * 100, dict(min_piece=1), [0, 10, 38, 65, 92, 100]),
    ("3 pieces", [MB] * 100, dict(pieces=3, min_piece=1), [0, 20, 60, 100]),
    ("4 pieces", [MB] * 100, dict(pieces=4, min_piece=1), [0, 10, 40, 70, 100]),
    ("9 pieces", [MB] * 100, dict(pieces=9, first_piece=0.03, min_piece=1), [0, 3, 16, 29, 42, 54, 67, 80, 92, 100]),
    ("no short last piece", [MB] * 100, dict(last_piece=0.0, min_piece=1), [0, 10, 33, 55, 78, 100]),
    ("min_piece limits the pieces", [MB] * 100, dict(min_piece=40 * MB), [0, 10, 100]),
    ("one dominant file", [90 * MB] + [MB] * 10, dict(min_piece=1), [0, 1, 3, 11]),
]


@pytest.mark.parametrize("name,sizes,policy,want", UPLOAD, ids=[c[0] for c in UPLOAD])
def test_upload_cuts(name, sizes, policy, want):
    segs = plan(sizes, **policy)
    assert cuts(segs) == want
    check_invariants(sizes, segs, False, 0)


@pytest.mark.parametrize("name,sizes,policy,want", RESIDENT, ids=[c[0] for c in RESIDENT])
def test_resident_cuts(name, sizes, policy, want):
    segs = plan(sizes, resident=True, base=1 << 30, **policy)
    assert cuts(segs) == want
    check_invariants(sizes, segs, True, 1 << 30)


@pytest.mark.parametrize("base", [0, 1 << 30, (1 << 30) + 16])
def test_resident_lead_files(base):
    # file sizes that are no multiple of 256: every piece after the first
    # starts off the 256-byte grid and gets a lead file down to it
    sizes = [1000003] * 100
    segs = plan(sizes, resident=True, base=base, min_piece=1)
    assert len(segs) == 5 and [s["lead"] for s in segs] == [0, 1, 1, 1, 1]
    check_invariants(sizes, segs, True, base)
    # the first piece starts at the batch's base and never has one
    assert segs[0]["d_data"] == base and segs[0]["off"][0] == 0


def test_resident_without_paths_has_no_lead():
    sizes = [1000003] * 100
    segs = plan(sizes, resident=True, base=0, paths=False, min_piece=1)
    assert len(segs) == 5 and all(s["lead"] == 0 for s in segs)
    assert cuts(segs) == cuts(plan(sizes, resident=True, base=0, min_piece=1))
    check_invariants(sizes, segs, True, 0, paths=False)


def _random_sizes(rng):
    n = rng.choice([1, 2, 3, 7, 40, 300])
    kind = rng.random()
    sizes = []
    for _ in range(n):
        r = rng.random()
        if r < 0.2:
            sizes.append(0)
        elif kind < 0.3:
            sizes.append(rng.randrange(0, 4096))             # many small files: dense
        else:
            sizes.append(int(2 ** rng.uniform(0, 22)))        # log-uniform up to 4 MiB
    if rng.random() < 0.5:
        sizes[rng.randrange(n)] = rng.randrange(4 * MB, 12 * MB)   # one file larger than `segment`
    if sum(sizes) == 0:
        sizes[0] = 1
    return sizes


def test_invariants_random():
    rng = random.Random(20240607)
    for _ in range(400):
        sizes = _random_sizes(rng)
        resident = rng.random() < 0.5
        base = rng.choice([0, 1 << 30, (1 << 30) + 16 * rng.randrange(16)])
        paths = rng.random() < 0.8
        policy = dict(segment=rng.choice([MB, 4 * MB]), segment_min=rng.choice([4096, 256 << 10, MB]),
                      balanced=rng.randrange(2), pieces=rng.choice([1, 2, 3, 4, 5, 9, 64]),
                      min_piece=rng.choice([1, 64 << 10, MB]), last_piece=rng.choice([0.0, 0.08, 0.3]),
                      first_piece=rng.choice([0.03, 0.1, 0.5]))
        segs = plan(sizes, resident=resident, base=base, paths=paths, **policy)
        check_invariants(sizes, segs, resident, base, paths)
