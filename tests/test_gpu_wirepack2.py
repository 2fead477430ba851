"""The 6-bit wire codec with escapes on the GPU (tsg_wire_unpack2 in
trivy_amd/csrc/wirepack.hip and the strip feeder of Engine::scan):

* the unpack kernel alone (tsg_test_wire_unpack2_device, which keeps a guard
  pattern past the strip and fails if it was touched) restores strips of 5
  bytes to five blocks, and one of two regions, in every mode: no escape,
  escapes on block edges and in a last partial group, the escape counts where
  7-bit and raw take over, short last blocks of each mode;
* the 2 MB batch of test_gpu_wirepack.py (several segments of several 64 KiB
  strips; secrets across block, strip and segment edges, which in a
  one-region strip are region edges too; empty files on strip starts; UTF-8
  fold characters and lone 0x80 / 0xFF bytes) with a stretch of noise and one
  of UTF-8 text added, so that all three modes occur, gives the oracle's
  findings under force2, 2, the default and 2 without packers; under force2 the
  bytes on the link and the blocks per mode are what test_wirepack2.model says;
* staging slots are reused across scans, and a failed scan leaves the lane
  clean for the next one.
"""
import numpy as np
import pytest

import test_gpu_wirepack as W
import test_wirepack2 as M
from _oracle_pool import oracle_scan_many
from trivy_amd import _lib

pytestmark = pytest.mark.gpu

BLOCK, REGION, STRIP = M.BLOCK, M.REGION, W.STRIP


def _with(buf, edits):
    for pos, v in edits:
        buf[pos] = v
    return bytes(buf)


def _strip_cases():
    esc496, esc497 = M._with_escapes(496, ord("#")), M._with_escapes(497, ord("#"))
    esc1008, esc1009 = M._with_escapes(1008, 0x80), M._with_escapes(1009, 0x80)
    tail6 = M.words(2 * BLOCK + 1030, 3)
    tail6[-1] = tail6[-2] = ord("@")
    three = M.words(2 * BLOCK, 11) + M.noise(BLOCK, 12) + bytearray(b"\xc3\xa9" * (BLOCK // 2)) + M.words(BLOCK, 13)
    return {
        "five": (bytes(M.words(5, 5)), ["raw"]),
        "one": (bytes(M.words(BLOCK, 4)), ["6"]),
        "edges": (_with(M.words(4 * BLOCK, 2), [(0, 0xE2), (BLOCK - 1, ord("#")), (BLOCK, 0x00), (4 * BLOCK - 1, 0xFF)]),
                  ["6"] * 4),
        "esc496": (bytes(esc496), ["6"]), "esc497": (bytes(esc497), ["7"]),
        "esc1008": (bytes(esc1008), ["6"]), "esc1009": (bytes(esc1009), ["raw"]),
        "tail6": (bytes(tail6), ["6"] * 3),
        "tail7": (bytes(M.noise(2 * BLOCK + 100, 6)), ["7"] * 3),
        "tail5raw": (_with(M.words(2 * BLOCK + 5, 7), [(2 * BLOCK + 4, 0xC3)]), ["6", "6", "raw"]),
        "three": (bytes(three), ["6", "6", "7", "raw", "6"]),
        "regions": (bytes(M.words(REGION, 21) + M.words(BLOCK + 5, 22, M.PUNCT)), ["6"] * 17 + ["raw"]),
    }


@pytest.mark.parametrize("case", ["five", "one", "edges", "esc496", "esc497", "esc1008", "esc1009", "tail6", "tail7",
                                  "tail5raw", "three", "regions"])
def test_unpack_kernel(case):
    buf, want_modes = _strip_cases()[case]
    packed, table, alpha, _, _, _ = M.pack2(buf)
    assert (packed, table, alpha) == M.model(buf)[:3] and M.modes(table) == want_modes
    p, t, a = (np.frombuffer(x, np.uint8).copy() for x in (packed, np.array(table, np.uint32).tobytes(), alpha))
    out = np.zeros(len(buf), np.uint8)
    _lib.check(_lib.lib().tsg_test_wire_unpack2_device(p.ctypes.data, len(p), t.ctypes.data, a.ctypes.data, len(buf),
                                                       out.ctypes.data))
    assert out.tobytes() == buf


# ---- end to end

_CACHE = {}


def _fixture():
    if not _CACHE:
        data, offsets, paths, cut = W._batch()
        data = bytearray(data)
        # three blocks of noise (7-bit) and three of UTF-8 text (raw) inside file 4, clear of what _batch planted
        o = offsets[4] + 50_000
        data[o:o + 3 * BLOCK] = M.noise(3 * BLOCK, 31)
        o = offsets[4] + 120_000
        data[o:o + 3 * BLOCK] = "é".encode("utf-8") * (3 * BLOCK // 2)
        data = bytes(data)
        items = [(paths[i], data[offsets[i]:offsets[i + 1]], False) for i in range(len(paths))]
        want = oracle_scan_many(items, procs=8)
        assert sum(len(w["Findings"]) for w in want) >= 8
        _CACHE["v"] = (data, offsets, paths, cut, want)
    return _CACHE["v"]


def _predict(data, offsets, cut):
    """(strips, wire bytes, strips that gain nothing and go raw, [6-bit, 7-bit, raw blocks, escaped bytes] of the
    others) with every strip through the packers"""
    nstrips = wire = raw = 0
    counts = [0, 0, 0, 0]
    for a, b in zip(cut[:-1], cut[1:]):
        seg = data[offsets[a]:offsets[b]]
        for s in range(0, len(seg), STRIP):
            strip = seg[s:s + STRIP]
            packed, table, alpha, c = M.model(strip)
            sent = M.pad(4 * len(table), 256) + len(alpha) + len(packed)
            nstrips += 1
            if sent >= len(strip):
                raw += 1
                wire += len(strip)
            else:
                wire += sent
                counts = [x + y for x, y in zip(counts, c)]
    return nstrips, wire, raw, counts


MODE_KEYS = ("blocks_6bit", "blocks_7bit", "blocks_raw", "escaped_bytes")


@pytest.mark.parametrize("mode", ["force2", "race2", "default", "nothreads2"])
def test_end_to_end_oracle(monkeypatch, mode):
    data, offsets, paths, cut, want = _fixture()
    nstrips, wire, raw, counts = _predict(data, offsets, cut)
    assert 1 <= raw <= 3 and all(c > 0 for c in counts)
    assert wire < 0.80 * len(data)
    sc = W._scanner(monkeypatch, {"force2": "force2", "race2": "2", "default": None, "nothreads2": "2"}[mode],
                    0 if mode == "nothreads2" else None)
    pin = W._Pinned(data)
    try:
        got, st = W._scan(sc, pin, offsets, paths)
    finally:
        pin.free()
    print(mode, {k: st[k] for k in ("pieces", "bytes", "wire_bytes", "packed_strips", "raw_strips", "pack_ms") + MODE_KEYS})
    assert got == want
    assert st["pieces"] == len(cut) - 1 and st["bytes"] == len(data)
    if mode == "force2":
        assert st["raw_strips"] == raw and st["packed_strips"] == nstrips - raw
        assert st["wire_bytes"] == wire
        assert [st[k] for k in MODE_KEYS] == counts
    elif mode in ("race2", "default"):
        assert st["packed_strips"] + st["raw_strips"] == nstrips
        assert wire <= st["wire_bytes"] <= len(data)
        # 6-bit blocks only come from the v2 packer: the default is v2
        assert (st["blocks_6bit"] > 0) == (st["packed_strips"] > 0)
    else:
        assert (st["packed_strips"], st["raw_strips"]) == (0, nstrips)
        assert st["wire_bytes"] == len(data) and [st[k] for k in MODE_KEYS] == [0, 0, 0, 0]


def test_repeated_scans_and_failure(monkeypatch):
    data, offsets, paths, cut, want = _fixture()
    _, wire, _, counts = _predict(data, offsets, cut)
    sc = W._scanner(monkeypatch, "force2")
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
