"""Line windows on the GPU (tsg_scan_batch_device_opts2, csrc/gather.hip
tsg_gw_lines): on every corpus of tests/_line_window_corpus.py the classes, the
run table, first runs (goff), the gathered bytes and the insufficient files
equal the CPU model's (tsg_scan_device_model_opts2, whose windows come from
the files' bytes); the findings equal tsg_scan_batch_resident's byte for byte;
cap 0 through the new entry is tsg_scan_batch_device_opts.
"""
import numpy as np
import pytest

import _line_window_corpus as LC
from test_gpu_window_gather import check_fallback_record
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

_SC = {}
STAT_KEYS = ("gather_files", "gather_bytes", "gather_runs", "window_files", "window_runs", "window_bytes",
             "fallback_files", "fallback_bytes")


def scanners(c, monkeypatch, **env):
    monkeypatch.setenv("TSG_K1_CHUNK", str(c.chunk))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    key = (repr(c.cfg), c.chunk, tuple(sorted(env.items())))
    if key not in _SC:
        sc = S.Scanner(c.cfg)
        sc.engine()
        _SC[key] = (sc, S.Scanner(c.cfg))
    return _SC[key]


def check_against_the_model(c, sc, msc):
    want = S.scan_table_model(msc, c.args)
    mout, mrec, mfb, mst = S.scan_device_model_windows(msc, c.args, c.chunk, c.window, window_lines=c.cap)
    assert mout == want
    got, _, info = S.scan_device_raw(sc, c.args, window=c.window, window_lines=c.cap)
    assert got == want
    res, _, _ = S.scan_raw(sc, c.args, resident=True)
    assert res == got
    assert len(info["segments"]) == 1 and info["segments"][0]["chunk_bytes"] == c.chunk
    g = info["segments"][0]["gather"]
    assert np.array_equal(g["cls"], mrec["cls"]), (g["cls"], mrec["cls"])
    assert np.array_equal(g["runs"], mrec["runs"]), (g["runs"], mrec["runs"])
    assert g["total"] == mrec["total"]
    assert np.array_equal(g["goff"], mrec["goff"])                         # every file in the run the model placed it in
    for src, dst, n in g["runs"].astype(np.int64):
        assert np.array_equal(g["bytes"][dst:dst + n], mrec["bytes"][dst:dst + n]), (src, dst, n)
    assert g["insufficient"] == mrec["insufficient"]
    assert g["caps"] and g["caps"][-1] >= g["total"] and all(g["guard_ok"])
    st = info["gather_stats"]
    for k in STAT_KEYS:
        assert st[k] == mst[k], (k, st[k], mst[k])
    assert st["fallback_files"] == len(mrec["insufficient"])
    # one record per candidate: the device's list holds the model's starts, a repeated record counting again
    assert st["line_widened"] >= mst["line_widened"] and (st["line_widened"] > 0) == (mst["line_widened"] > 0)
    assert st["line_capped"] >= mst["line_capped"] and (st["line_capped"] > 0) == (mst["line_capped"] > 0)
    assert 0 <= st["line_ms"] <= st["gather_ms"]
    return info, mrec, mfb


@pytest.mark.parametrize("name", LC.NAMES)
def test_line_windows_equal_the_model_gpu(name, monkeypatch):
    c = LC.corpus(name)
    sc, msc = scanners(c, monkeypatch)
    info, mrec, mfb = check_against_the_model(c, sc, msc)
    assert info["segments"][0]["gather"]["insufficient"] == c.insufficient
    if name in LC.NO_FALLBACK:
        assert info["gather_stats"]["fallback_files"] == 0
    check_fallback_record(c, info, mfb)


@pytest.mark.parametrize("name", ["long_own_line", "chunk_phases", "unchanged_builtin"])
def test_cap_zero_is_the_byte_window_scan_gpu(name, monkeypatch):
    c = LC.corpus(name)
    sc, _ = scanners(c, monkeypatch)
    base, _, binfo = S.scan_device_raw(sc, c.args, window=c.window)
    got, _, info = S.scan_device_raw(sc, c.args, window=c.window, window_lines=0)
    assert got == base and len(info["segments"]) == len(binfo["segments"]) == 1
    for k in ("cls", "need", "goff", "runs", "bytes"):
        assert np.array_equal(info["segments"][0]["gather"][k], binfo["segments"][0]["gather"][k]), k
    assert info["segments"][0]["gather"]["insufficient"] == binfo["segments"][0]["gather"]["insufficient"] == c.plain
    for k in STAT_KEYS:
        assert info["gather_stats"][k] == binfo["gather_stats"][k], k
    assert info["gather_stats"]["line_widened"] == info["gather_stats"]["line_capped"] == 0
    assert info["gather_stats"]["line_ms"] == 0
    assert (info["fallback"] is None) == (binfo["fallback"] is None)
    if info["fallback"] is not None:
        for k in ("need", "goff", "runs", "bytes"):
            assert np.array_equal(info["fallback"][k], binfo["fallback"][k]), k


@pytest.mark.parametrize("reverse", [False, True])
def test_the_whole_corpus_as_one_batch_gpu(reverse, monkeypatch):
    c = LC.combined(reverse)
    sc, msc = scanners(c, monkeypatch)
    info, mrec, mfb = check_against_the_model(c, sc, msc)
    names = [a.FilePath for a in c.args]
    assert sorted(names[f] for f in mrec["insufficient"]) == ["k/line40k.log", "m/long.pem"]


@pytest.mark.parametrize("name", ["long_own_line", "shared_chunks", "multi_line", "cap_short"])
def test_line_windows_in_pieces_with_lead_files_gpu(name, monkeypatch):
    # several pieces (lead files in front of the later ones): windows meet piece cuts and leads
    c = LC.corpus(name) if name != "long_own_line" else LC.combined()
    sc, msc = scanners(c, monkeypatch, TSG_PIECES=3, TSG_MIN_PIECE_BYTES=1)
    want = S.scan_table_model(msc, c.args)
    got, _, info = S.scan_device_raw(sc, c.args, window=c.window, window_lines=c.cap)
    assert got == want
    res, _, _ = S.scan_raw(sc, c.args, resident=True)
    assert res == got
    if c.name == "combined":
        assert info["stats"]["pieces"] == 3
    _, mrec, _, mst = S.scan_device_model_windows(msc, c.args, c.chunk, c.window, window_lines=c.cap)
    short = sorted(s["f0"] + f - s["lead"] for s in info["segments"] for f in s["gather"]["insufficient"])
    # a piece's frame has its own chunk grid, so a file's chunks differ from the one-segment model's; which
    # files fall back does not: those with a line beyond the cap or a match beyond `after`, in any phase
    assert short == mrec["insufficient"]
    assert info["gather_stats"]["fallback_files"] == len(short)
    for s in info["segments"]:
        assert all(s["gather"]["guard_ok"])
    c2 = LC.LineCorpus(c.name, "", [(a.FilePath, a.Content) for a in c.args], plain=[], insufficient=short,
                       window=c.window, cap=c.cap, cfg=c.cfg)
    check_fallback_record(c2, info)


def test_compressed_layer_chain_with_line_windows_gpu(monkeypatch):
    import gzip
    import io
    import tarfile
    import _zstd_corpus as Z
    c = LC.corpus("long_own_line")
    e = LC.corpus("file_edges")

    def tar_of(args):
        buf = io.BytesIO()
        with tarfile.open(fileobj=buf, mode="w") as tf:
            for a in args:
                ti = tarfile.TarInfo(a.FilePath)
                ti.size = len(a.Content)
                tf.addfile(ti, io.BytesIO(a.Content))
        return buf.getvalue()
    monkeypatch.setenv("TSG_K1_CHUNK", str(c.chunk))
    blobs = [gzip.compress(tar_of(c.args)), Z.raw_frame(tar_of(e.args[:4]), fcs_bytes=4, checksum=True), tar_of(e.args[4:])]
    sc = S.Scanner(None)
    base = sc.ScanLayersCompressedDevice(blobs)
    seen = []
    real = sc.ScanBatchDevice

    def spy(d_data, offsets, paths, binary=None, with_stats=False, window=None, window_lines=None):
        out, st = real(d_data, offsets, paths, binary, with_stats=True, window=window, window_lines=window_lines)
        seen.append((window, window_lines, st))
        return (out, st) if with_stats else out
    monkeypatch.setattr(sc, "ScanBatchDevice", spy)
    got = sc.ScanLayersCompressedDevice(blobs, window=c.window, window_lines=c.cap)
    assert [x[2] for x in got] == [x[2] for x in base]
    assert [sum(len(s["Findings"]) for s in x[2]) for x in got] == [2, 4, 4]
    assert len(seen) == 3 and all(w == c.window and cap == c.cap for w, cap, _ in seen)
    assert [st["window_files"] for _, _, st in seen] == [2, 4, 4] and all(st["fallback_files"] == 0 for _, _, st in seen)
    assert seen[0][2]["line_widened"] > 0
    lines_bytes = seen[0][2]["gather_bytes"]
    seen.clear()
    plain = sc.ScanLayersCompressedDevice(blobs, window=c.window)
    assert [x[2] for x in plain] == [x[2] for x in base]
    assert seen[0][1] is None and seen[0][2]["fallback_files"] == 2 and seen[0][2]["gather_bytes"] > 10 * lines_bytes
    seen.clear()
    gz = sc.ScanLayersGzipDevice(blobs[:1], window=c.window, window_lines=c.cap)
    assert [x[2] for x in gz] == [x[2] for x in base[:1]] and seen[0][2]["gather_bytes"] == lines_bytes
    with pytest.raises(ValueError):
        sc.ScanLayersCompressedDevice(blobs, window_lines=c.cap)
