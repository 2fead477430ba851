"""The split block mode of the 6-bit wire codec on the GPU (the fourth branch
of tsg_wire_unpack2 in trivy_amd/csrc/wirepack.hip, and TSG_WIRE_PACK=3 /
force3 in the strip feeder of Engine::scan):

* the unpack kernel alone (tsg_test_wire_unpack3_device, which keeps a guard
  pattern past the strip and fails if it was touched) restores strips of 5
  bytes to five blocks, and one of a region and a block: every hot count and
  length that changes a lane's share or a scan (all hot, odd hot count, a
  5-bit run that is no multiple of 8, lengths that are no multiple of 8 or 16),
  escapes at byte 0, at the last byte and sixteen in one lane, hot and warm
  bytes in turn, runs that flip at bytes 1024, 2048 and 3072 (the wave edges),
  strips with all four modes and a short last block of each;
* the 2 MB batch of test_gpu_wirepack2 gives the oracle's findings under
  force3, 3 and 3 without packers; under force3 the bytes on the link and the
  blocks per mode are what test_wirepack3.model says, and fewer than the v2
  model's;
* staging slots are reused across scans, and a failed scan leaves the lane
  clean for the next one.
"""
import numpy as np
import pytest

import test_gpu_wirepack as W
import test_gpu_wirepack2 as G2
import test_wirepack2 as M2
import test_wirepack3 as M
from trivy_amd import _lib

pytestmark = pytest.mark.gpu

BLOCK, REGION, STRIP = M.BLOCK, M.REGION, W.STRIP


def _edges(at, xval):
    buf = M.crafted("hhhw" * (BLOCK // 4))[0]
    for k in at:
        buf[k] = xval
    return bytes(buf)


def _four(tail):
    """a strip with a split, a 6-bit, a 7-bit and a raw block and a last block of the classes `tail` ('r': raw)"""
    cl = "hhw" * (BLOCK // 3) + "h" + "w" * BLOCK + "wx" * (BLOCK // 2) + "w" * BLOCK + tail.replace("r", "w")
    buf = M.crafted(cl)[0]
    buf[3 * BLOCK:4 * BLOCK] = b"\xc3\xa9" * (BLOCK // 2)         # (bytes >= 0x80 are not sampled: the alphabet stays)
    if "r" in tail:
        buf[4 * BLOCK:] = (b"\xc3\xa9" * len(tail))[:len(tail)]
    return bytes(buf)


def _strip_cases():
    return {
        "five": (bytes(M.crafted("hhhhw")[0]), ["raw"]),
        "one": (bytes(M.block(2000, 10)), ["split"]),
        "all_hot": (b"e" * BLOCK, ["split"]),
        "all_hot_odd_len": (b"e" * 3001, ["split"]),
        "h_odd": (bytes(M.block(1501, 7)), ["split"]),
        "len_odd": (bytes(M.block(1500, 7, ln=BLOCK - 3)), ["split"]),
        "len_2999": (bytes(M.block(900, 7, ln=2999)), ["split"]),
        "len_1501": (bytes(M.block(701, 7, ln=1501)), ["split"]),
        "few_hot": (bytes(M.block(128, 0)), ["split"]),
        "esc_first": (_edges([0], 0x80), ["split"]),
        "esc_last": (_edges([BLOCK - 1], 0xFF), ["split"]),
        "esc_lane": (_edges(range(16 * 77, 16 * 78), 0x7F), ["split"]),
        "esc_many": (bytes(M.block(1024, 1136, xval=0x80)), ["split"]),
        "esc_cold": (bytes(M.block(1024, 112, e6=0)), ["split"]),
        "alternate": (bytes(M.crafted("hw" * (BLOCK // 2))[0]), ["split"]),
        "wave_edges": (bytes(M.crafted(("h" * 1024 + "w" * 1024) * 2)[0]), ["split"]),
        "wave_edges_off": (bytes(M.crafted("w" * 1023 + "h" * 1025 + "w" * 1024 + "h" * 1024)[0]), ["split"]),
        "four": (_four("hhw" * 518 + "h"), ["split", "6", "7", "raw", "split"]),
        "tail6": (_four("w" * 1200), ["split", "6", "7", "raw", "6"]),
        "tail7": (_four("wx" * 388 + "w"), ["split", "6", "7", "raw", "7"]),
        "tailraw": (_four("r" * 100), ["split", "6", "7", "raw", "raw"]),
        "region": (bytes(M.crafted("hhw" * ((REGION + BLOCK) // 3) + "hw")[0]), ["split"] * 17),
    }


@pytest.mark.parametrize("case", sorted(_strip_cases()))
def test_unpack_kernel(case):
    buf, want_modes = _strip_cases()[case]
    packed, table, alpha, _, _, _ = M.pack3(buf)
    assert (packed, table, alpha) == M.model(buf)[:3] and M.modes(table) == want_modes
    p, t, a = (np.frombuffer(x, np.uint8).copy() for x in (packed, np.array(table, np.uint32).tobytes(), alpha))
    out = np.zeros(len(buf), np.uint8)
    _lib.check(_lib.lib().tsg_test_wire_unpack3_device(p.ctypes.data, len(p), t.ctypes.data, a.ctypes.data, len(buf),
                                                       out.ctypes.data))
    assert out.tobytes() == buf


# ---- end to end

MODE_KEYS = G2.MODE_KEYS + ("blocks_split",)


def _predict(data, offsets, cut, model):
    """as test_gpu_wirepack2._predict, by the given model; the counts have the split blocks as a fifth value"""
    nstrips = wire = raw = 0
    counts = [0, 0, 0, 0, 0]
    for a, b in zip(cut[:-1], cut[1:]):
        seg = data[offsets[a]:offsets[b]]
        for s in range(0, len(seg), STRIP):
            strip = seg[s:s + STRIP]
            packed, table, alpha, c = model(strip)
            sent = M2.pad(4 * len(table), 256) + len(alpha) + len(packed)
            nstrips += 1
            if sent >= len(strip):
                raw += 1
                wire += len(strip)
            else:
                wire += sent
                counts = [x + y for x, y in zip(counts, list(c) + [0])]
    return nstrips, wire, raw, counts


_PRED = {}


def _predicted():
    if not _PRED:
        data, offsets, paths, cut, want = G2._fixture()
        _PRED["v"] = (_predict(data, offsets, cut, M.model), _predict(data, offsets, cut, M2.model))
    return _PRED["v"]


@pytest.mark.parametrize("mode", ["force3", "race3", "nothreads3"])
def test_end_to_end_oracle(monkeypatch, mode):
    data, offsets, paths, cut, want = G2._fixture()
    (nstrips, wire, raw, counts), v2 = _predicted()
    # a condition on the fixture: the split mode gains on it
    assert wire < v2[1] and counts[4] > 0
    sc = W._scanner(monkeypatch, {"force3": "force3", "race3": "3", "nothreads3": "3"}[mode],
                    0 if mode == "nothreads3" else None)
    pin = W._Pinned(data)
    try:
        got, st = W._scan(sc, pin, offsets, paths)
    finally:
        pin.free()
    print(mode, {k: st[k] for k in ("pieces", "bytes", "wire_bytes", "packed_strips", "raw_strips", "pack_ms") + MODE_KEYS})
    assert got == want
    assert st["pieces"] == len(cut) - 1 and st["bytes"] == len(data)
    if mode == "force3":
        assert st["raw_strips"] == raw and st["packed_strips"] == nstrips - raw
        assert st["wire_bytes"] == wire
        assert [st[k] for k in MODE_KEYS] == counts and st["blocks_split"] > 0
    elif mode == "race3":
        assert st["packed_strips"] + st["raw_strips"] == nstrips
        assert wire <= st["wire_bytes"] <= len(data)
    else:
        assert (st["packed_strips"], st["raw_strips"]) == (0, nstrips)
        assert st["wire_bytes"] == len(data) and [st[k] for k in MODE_KEYS] == [0, 0, 0, 0, 0]


def test_repeated_scans_and_failure(monkeypatch):
    data, offsets, paths, cut, want = G2._fixture()
    (_, wire, _, counts), _ = _predicted()
    sc = W._scanner(monkeypatch, "force3")
    pin = W._Pinned(data)
    try:
        for _ in range(2):                            # the second scan reuses the staging slots
            got, st = W._scan(sc, pin, offsets, paths)
            assert got == want and st["wire_bytes"] == wire and [st[k] for k in MODE_KEYS] == counts
        lanes = W._lanes(sc)
        _lib.check(_lib.lib().tsg_test_inject_segment_failures(sc.engine(), 1))
        with pytest.raises(Exception, match="injected segment failure"):
            W._scan(sc, pin, offsets, paths)
        got, st = W._scan(sc, pin, offsets, paths)
        assert got == want and st["wire_bytes"] == wire
        assert W._lanes(sc) == lanes == 1
    finally:
        pin.free()
