"""The device-only scan with windows on the GPU (tsg_scan_batch_device_opts,
csrc/gather.hip tsg_gw_*): on every corpus of tests/_window_corpus.py the
findings equal tsg_scan_batch_resident's and the table model's; the classes,
the run table, the gathered bytes and the fallback set equal the CPU model
(tsg_scan_device_model_opts); the guard bytes behind the gather buffer are
whole; the stats agree with the records.
"""
import numpy as np
import pytest

import _window_corpus as WC
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

_SC = {}


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


@pytest.mark.parametrize("name", WC.NAMES)
def test_windows_equal_the_model_gpu(name, monkeypatch):
    c = WC.corpus(name)
    sc, msc = scanners(c, monkeypatch)
    want = S.scan_table_model(msc, c.args)
    mout, mrec, mfb, mst = S.scan_device_model_windows(msc, c.args, c.chunk, c.window)
    assert mout == want
    got, _, info = S.scan_device_raw(sc, c.args, window=c.window)
    assert got == want
    res, _, _ = S.scan_raw(sc, c.args, resident=True)
    assert res == got
    assert len(info["segments"]) == 1 and info["segments"][0]["chunk_bytes"] == c.chunk
    g = info["segments"][0]["gather"]
    assert np.array_equal(g["cls"], mrec["cls"]), (g["cls"], mrec["cls"])
    assert g["insufficient"] == mrec["insufficient"] == c.insufficient
    assert np.array_equal(g["runs"], mrec["runs"]) and g["total"] == mrec["total"]
    assert np.array_equal(g["goff"], mrec["goff"])
    for src, dst, n in g["runs"].astype(np.int64):
        assert np.array_equal(g["bytes"][dst:dst + n], mrec["bytes"][dst:dst + n]), (src, dst, n)
    assert g["caps"] and g["caps"][-1] >= g["total"] and all(g["guard_ok"])
    st = info["gather_stats"]
    for k in ("gather_files", "gather_bytes", "gather_runs", "window_files", "window_runs", "window_bytes",
              "fallback_files", "fallback_bytes"):
        assert st[k] == mst[k], (k, st[k], mst[k])
    assert S.gather_pool(sc)[0] == S.gather_pool(sc)[1] > 0
    check_fallback_record(c, info, mfb)


def check_fallback_record(c, info, mfb=None):
    """The fallback round's gather as the device delivered it: plan_gather over the insufficient files per segment,
    the bytes of every run equal to the batch's, the guard behind the buffer whole."""
    fb = info["fallback"]
    if not c.insufficient:
        assert fb is None
        return
    data, off = S.pack(c.args)
    need = np.zeros(len(c.args), np.uint8)
    need[c.insufficient] = 1
    assert np.array_equal(fb["need"], need) and fb["caps"] and fb["caps"][-1] >= fb["total"] and all(fb["guard_ok"])
    assert fb["total"] == info["gather_stats"]["fallback_bytes"] and fb["total"] % 64 == 0
    r = fb["runs"].astype(np.int64)
    assert (r[:, 1] % 64 == 0).all() and (r[1:, 1] >= r[:-1, 1] + r[:-1, 2]).all()
    for src, dst, n in r:
        assert np.array_equal(fb["bytes"][dst:dst + n], data[src:src + n]), (src, dst, n)
    for f in c.insufficient:                              # every file whole, at its goff
        a, b = int(off[f]), int(off[f + 1])
        g = int(fb["goff"][f])
        assert np.array_equal(fb["bytes"][g:g + b - a], data[a:b]), f
    assert (fb["goff"][need == 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    if mfb is not None and len(info["segments"]) == 1:    # one segment: the model's round, record for record
        assert np.array_equal(fb["goff"], mfb["goff"]) and np.array_equal(fb["runs"], mfb["runs"])
        assert fb["total"] == mfb["total"] and np.array_equal(fb["bytes"], mfb["bytes"])


def test_large_sparse_window_bytes_gpu(monkeypatch):
    c = WC.corpus("large_sparse")
    sc, msc = scanners(c, monkeypatch)
    _, mrec, _, mst = S.scan_device_model_windows(msc, c.args, c.chunk, c.window)
    _, _, info = S.scan_device_raw(sc, c.args, window=c.window)
    st = info["gather_stats"]
    assert st["fallback_files"] == 0 and st["window_bytes"] == mst["window_bytes"] == mrec["total"]
    assert st["gather_bytes"] == st["window_bytes"] < int(c.offsets[-1]) // 100


@pytest.mark.parametrize("name", ["positions", "fallbacks"])
def test_windows_in_pieces_with_lead_files_gpu(name, monkeypatch):
    # several pieces (lead files in front of the later ones), two drivers: the findings and the fallback set
    c = WC.corpus(name)
    sc, msc = scanners(c, monkeypatch, TSG_PIECES=3, TSG_MIN_PIECE_BYTES=1)
    want = S.scan_table_model(msc, c.args)
    got, _, info = S.scan_device_raw(sc, c.args, window=c.window)
    assert got == want and info["stats"]["pieces"] == 3
    short = sorted(s["f0"] + f - s["lead"] for s in info["segments"] for f in s["gather"]["insufficient"])
    assert short == c.insufficient
    assert info["gather_stats"]["fallback_files"] == len(c.insufficient)
    for s in info["segments"]:
        assert all(s["gather"]["guard_ok"])
    check_fallback_record(c, info)


def test_small_gather_buffer_is_grown_gpu(monkeypatch):
    c = WC.corpus("whole_builtin")
    sc, msc = scanners(c, monkeypatch, TSG_GATHER_CAP=256)
    got, _, info = S.scan_device_raw(sc, c.args, window=c.window)
    assert got == S.scan_table_model(msc, c.args)
    g = info["segments"][0]["gather"]
    assert len(g["caps"]) >= 2 and g["caps"][0] == 256 and all(g["guard_ok"]) and info["gather_stats"]["gather_retries"] >= 1


def test_options_off_is_scan_batch_device_gpu(monkeypatch):
    c = WC.corpus("whole_builtin")
    sc, _ = scanners(c, monkeypatch)
    base, _, binfo = S.scan_device_raw(sc, c.args)
    for window in ((0, 0, 0), (0, 0, 4096)):
        got, _, info = S.scan_device_raw(sc, c.args, window=window)
        assert got == base
        for k in ("need", "goff", "runs", "bytes"):
            assert np.array_equal(info["segments"][0]["gather"][k], binfo["segments"][0]["gather"][k]), k
        for k in ("gather_files", "gather_bytes", "gather_runs"):
            assert info["gather_stats"][k] == binfo["gather_stats"][k]
        assert info["gather_stats"]["window_bytes"] == 0


def test_compressed_layer_chain_with_windows_gpu(monkeypatch):
    import io
    import tarfile
    import gzip
    c = WC.corpus("positions")
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w") as tf:
        for a in c.args[:4]:
            ti = tarfile.TarInfo(a.FilePath)
            ti.size = len(a.Content)
            tf.addfile(ti, io.BytesIO(a.Content))
    blob = gzip.compress(buf.getvalue())
    sc = S.Scanner(None)
    base = sc.ScanLayersCompressedDevice([blob])
    # the scans the chain makes, seen through the call it ends in: the keyword must arrive there
    seen = []
    real = sc.ScanBatchDevice

    def spy(d_data, offsets, paths, binary=None, with_stats=False, window=None):
        out, st = real(d_data, offsets, paths, binary, with_stats=True, window=window)
        seen.append((window, st))
        return (out, st) if with_stats else out
    monkeypatch.setattr(sc, "ScanBatchDevice", spy)
    got = sc.ScanLayersCompressedDevice([blob], window=c.window)
    assert [x[2] for x in got] == [x[2] for x in base]
    assert sum(len(s["Findings"]) for s in got[0][2]) >= 4
    assert len(seen) == 1 and seen[0][0] == c.window
    st = seen[0][1]
    assert st["window_files"] == 4 and st["fallback_files"] == 0 and 0 < st["window_bytes"] == st["gather_bytes"]
    seen.clear()
    sc.ScanLayersGzipDevice([blob])
    assert seen[0][0] is None and seen[0][1]["window_files"] == 0 and seen[0][1]["gather_bytes"] > 10 * st["gather_bytes"]
    seen.clear()
    sc.ScanLayersGzipDevice([blob], window=c.window)
    assert seen[0][1]["window_files"] == 4 and seen[0][1]["gather_bytes"] == st["gather_bytes"]
