"""The wire feeder's strip plan and its two copy streams on the GPU
(trivy_amd/csrc/wire_strips.h, WireFeed in trivy_amd/csrc/engine.hip).

24 MB of text in 12 files, scanned as three segments with 1 MiB strips and
four packers, so that the first segment is cut with the ramp: four strips
growing from 256 KiB to 1 MiB, whole strips, and its last 2 MiB in 64 KiB
pieces.  Secrets lie across the first ramp-strip edge, an edge between two
growing strips, the edge to the whole strips, both edges of the first small
back strip, a uniform strip edge of the second segment and a segment edge; an
empty file starts on a ramp strip, and a run of UTF-8 text (raw blocks) lies
inside a small strip.

The findings (the full types.Secret JSON) of every way to send the batch are
those of the scan with wire packing off: racing and forced packers of both
codecs, no packers, the uniform cut (TSG_WIRE_RAMP=0), one and two copy
streams.  Where every strip waits for a packer (force2) the strip counts are
the plan's and the bytes on the link are what test_wirepack2.model gives for
the planned strips.  Nothing is timed.
"""
import numpy as np
import pytest

import test_gpu_wirepack as W
import test_wire_strips as TS
import test_wirepack2 as M

pytestmark = pytest.mark.gpu

K64, MIB = 65536, 1 << 20
STRIP = MIB
SEGMENT = 8 * MIB
PACKERS = 4
FRONT_SIZES = TS.front_sizes(STRIP, PACKERS)          # 256 KiB, 512 KiB, 768 KiB, 1 MiB
FRONT = sum(FRONT_SIZES)
BACK = TS.BACK * (STRIP // TS.BACK_DIV)


def _batch():
    sizes = [FRONT_SIZES[0] + FRONT_SIZES[1], 0] + [2_100_000 + 1_013 * i for i in range(10)]
    sizes[-1] += 24_000_000 - sum(sizes)
    offsets = [0]
    for s in sizes:
        offsets.append(offsets[-1] + s)
    cut = W._cuts(offsets, SEGMENT)
    assert len(cut) == 4 and len(sizes) == 12
    base = bytes(W._filler(MIB, 77))
    data = bytearray()
    for i, s in enumerate(sizes):
        rot = base[1000 * i:] + base[:1000 * i]
        data += (rot * (s // MIB + 1))[:s]
    seg = [offsets[c] for c in cut]
    seg0 = seg[1]
    assert seg0 >= FRONT + BACK + STRIP
    back = (seg0 - BACK) // K64 * K64
    assert offsets[1] == offsets[2] == sum(FRONT_SIZES[:2])    # the empty file 1 starts on the third ramp strip
    for pos in (FRONT_SIZES[0], sum(FRONT_SIZES[:3]), FRONT, back, back + K64, seg[1] + 3 * STRIP, seg[2] + 5 * W.BLOCK):
        W._plant(data, pos)
    data[seg[1] - len(W.SECRET):seg[1]] = W.SECRET
    data[seg[1]:seg[1] + len(W.SECRET) - 1] = W.SECRET[1:]
    # UTF-8 inside the first ramp strip (256 KiB): fold characters, then a block and a half of two-byte characters
    o = 3 * K64 + 1000
    utf = "token = Key-ſecret  # Kſ\n".encode("utf-8") + "é".encode("utf-8") * 3000 + b"\n"
    data[o:o + len(utf)] = utf
    W._plant(data, o + len(utf) + 100)
    paths = ["src/g%02d.py" % i for i in range(len(sizes))]
    return bytes(data), offsets, paths, cut


def _plans(offsets, cut, ramp, packers):
    out = []
    for k, (a, b) in enumerate(zip(cut[:-1], cut[1:])):
        off, ln = TS.model(offsets[b] - offsets[a], STRIP, ramp and k == 0, packers)
        out.append([(offsets[a] + int(o), int(n)) for o, n in zip(off, ln)])
    return out


_CACHE = {}


def _predict(data, plans):
    """(strips, wire bytes with every strip through the 6-bit packer, strips that gain nothing, head bytes)"""
    nstrips = wire = raw = heads = 0
    for plan in plans:
        for o, n in plan:
            key = (o, n)
            if key not in _CACHE:
                packed, table, alpha, _ = M.model(data[o:o + n])
                _CACHE[key] = (M.pad(4 * len(table), 256) + len(alpha), len(packed))
            head, body = _CACHE[key]
            nstrips += 1
            heads += head
            if head + body >= n:
                raw += 1
                wire += n
            else:
                wire += head + body
    return nstrips, wire, raw, heads


def _scan(monkeypatch, data, offsets, paths, env):
    from trivy_amd import secret as S
    for k in ("TSG_WIRE_PACK", "TSG_WIRE_PACK_THREADS", "TSG_WIRE_RAMP", "TSG_WIRE_COPY_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSG_WIRE_STRIP_BYTES", str(STRIP))
    monkeypatch.setenv("TSG_SEGMENT_BYTES", str(SEGMENT))
    monkeypatch.setenv("TSG_WIRE_PACK_THREADS", str(PACKERS))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = S.Scanner(None)
    pin = W._Pinned(data)
    try:
        return W._scan(sc, pin, offsets, paths)
    finally:
        pin.free()


def _fixture(monkeypatch):
    if "v" not in _CACHE:
        data, offsets, paths, cut = _batch()
        want, st = _scan(monkeypatch, data, offsets, paths, {"TSG_WIRE_PACK": "0"})
        assert (st["packed_strips"], st["raw_strips"]) == (0, 0) and st["wire_bytes"] == st["bytes"] == len(data)
        assert st["pieces"] == 3
        nfound = sum(len(w.get("Findings") or []) for w in want)
        assert nfound >= 10, nfound                    # the nine planted keys (two at the segment edge) and more
        assert len(want[1].get("Findings") or []) == 0 and len(want[0]["Findings"]) >= 1
        _CACHE["v"] = (data, offsets, paths, cut, want)
    return _CACHE["v"]


MODES = {
    "race": {"TSG_WIRE_PACK": "2"},
    "force2": {"TSG_WIRE_PACK": "force2"},
    "force": {"TSG_WIRE_PACK": "force"},
    "nothreads": {"TSG_WIRE_PACK": "2", "TSG_WIRE_PACK_THREADS": "0"},
    "noramp": {"TSG_WIRE_PACK": "force2", "TSG_WIRE_RAMP": "0"},
    "streams1": {"TSG_WIRE_PACK": "force2", "TSG_WIRE_COPY_STREAMS": "1"},
    "streams2": {"TSG_WIRE_PACK": "force2", "TSG_WIRE_COPY_STREAMS": "2"},
    "race_streams1": {"TSG_WIRE_PACK": "2", "TSG_WIRE_COPY_STREAMS": "1"},
    "streams_other": {"TSG_WIRE_PACK": "force2", "TSG_WIRE_COPY_STREAMS": "0"},     # neither 1 nor 2: ignored
}


def test_plan_of_the_batch():
    """(no GPU work: the fixture's first segment has every kind of strip the other tests rely on)"""
    data, offsets, paths, cut = _batch()
    ramp, flat = _plans(offsets, cut, True, PACKERS), _plans(offsets, cut, False, PACKERS)
    lens = [n for _, n in ramp[0]]
    assert lens[:len(FRONT_SIZES)] == FRONT_SIZES and lens[len(FRONT_SIZES)] == STRIP
    assert FRONT_SIZES[0] < STRIP and FRONT_SIZES[-1] == STRIP and len(FRONT_SIZES) >= 3
    assert lens[-TS.BACK:-1] == [STRIP // TS.BACK_DIV] * (TS.BACK - 1) and len(ramp[0]) > len(flat[0])
    assert ramp[1:] == flat[1:] and all(n == STRIP for p in flat for _, n in p[:-1])
    assert _plans(offsets, cut, True, 0) == flat


@pytest.mark.parametrize("mode", list(MODES))
def test_findings_and_link_bytes(monkeypatch, mode):
    data, offsets, paths, cut, want = _fixture(monkeypatch)
    env = MODES[mode]
    ramp = env.get("TSG_WIRE_RAMP") != "0" and env.get("TSG_WIRE_PACK_THREADS") != "0"
    plans = _plans(offsets, cut, ramp, PACKERS)
    got, st = _scan(monkeypatch, data, offsets, paths, env)
    print(mode, {k: st[k] for k in ("pieces", "bytes", "wire_bytes", "packed_strips", "raw_strips")})
    assert got == want
    assert st["pieces"] == 3 and st["bytes"] == len(data)
    nstrips = sum(len(p) for p in plans)
    assert st["packed_strips"] + st["raw_strips"] == nstrips
    if env["TSG_WIRE_PACK"] == "force2":
        n, wire, raw, _ = _predict(data, plans)
        assert n == nstrips and wire < 0.85 * len(data)
        assert st["raw_strips"] == raw and st["packed_strips"] == nstrips - raw
        assert st["wire_bytes"] == wire
    elif mode == "nothreads":
        assert st["packed_strips"] == 0 and st["wire_bytes"] == len(data)
    elif env["TSG_WIRE_PACK"] == "2":
        _, _, _, heads = _predict(data, plans)
        assert st["wire_bytes"] <= len(data) + heads
    else:
        # 7-bit: 7/8 and the heads; only a segment's short last strip can gain nothing
        assert st["raw_strips"] <= 3 and st["wire_bytes"] < 0.9 * len(data)
