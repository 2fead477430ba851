"""CPU model of the device-side content preparation (tsg_prepare_device_model:
csrc/prep.h plan_prep, the kernels' per-byte rule stated sequentially) against
two independent restatements of Analyze's preparation
(pkg/fanal/analyzer/secret/secret.go:103-150): the host feed
(tsg_prepare_batch_opts, feed.cpp prepare_core) and the oracle
(oracle.secret_oracle: required, is_binary, extract_printable_bytes,
replace(b"\\r", b"")), on every corpus of tests/_prep_corpus.py.  The corpora's
own conditions are asserted, not assumed.  No GPU."""
import ctypes
import re

import numpy as np
import pytest

import _prep_corpus as PC
from oracle import secret_oracle as so
from trivy_amd import _lib
from trivy_amd import secret as S

CORPORA = PC.corpora()
KIND = {"dropped": 0, "text": 1, "printable": 2}
_scanners = {}


def scanner(config_path):
    if config_path not in _scanners:
        _scanners[config_path] = S.Scanner(S.ParseConfig(config_path) if config_path else None)
    return _scanners[config_path]


_oracle = {}


def oracle_prepare(c):
    """[(index, content, binary)] of the kept files by the oracle, once per corpus."""
    if c.name not in _oracle:
        a = so.SecretAnalyzer(c.config_path)
        pats = [re.compile(p.split(":", 1)[1]) for p in c.file_patterns if p.startswith("secret:")]
        out = []
        for i, (p, raw) in enumerate(c.raw_files):
            if not (any(rx.search(p) for rx in pats) or a.required(p, len(raw))):
                continue
            binary = so.is_binary(raw[:300])
            if binary and so.go_ext(p) != ".pyc":
                continue
            out.append((i, so.extract_printable_bytes(raw) if binary else raw.replace(b"\r", b""), binary))
        _oracle[c.name] = out
    return _oracle[c.name]


def test_corpus_list_is_complete():
    assert sorted(CORPORA) == sorted(PC.NAMES)


@pytest.mark.parametrize("name", PC.NAMES)
def test_model_equals_host_feed_and_oracle(name):
    c = CORPORA[name]
    sc = scanner(c.config_path)
    m = S.prepare_batch_view(sc, c.raw_files, c.config_path, c.file_patterns, model=True)
    h = S.prepare_batch_view(sc, c.raw_files, c.config_path, c.file_patterns)
    # every file's fate is the one the corpus names
    assert m["kinds"] == [KIND[f] for _, _, f in c.files]
    # the host feed: kept index, binary flags, offsets, bytes
    assert m["index"] == h["index"]
    assert m["binary"] == h["binary"]
    assert np.array_equal(m["offsets"], h["offsets"])
    assert m["data"] == h["data"]
    # the oracle, file by file
    want = oracle_prepare(c)
    assert [w[0] for w in want] == m["index"]
    assert [int(w[2]) for w in want] == m["binary"]
    assert b"".join(w[1] for w in want) == m["data"]
    off = m["offsets"]
    for k, (i, content, _b) in enumerate(want):
        assert m["data"][int(off[k]):int(off[k + 1])] == content, c.files[i][0]
    # per raw file: a dropped file has zero length in the device's starts
    no = m["new_offsets"]
    assert int(no[0]) == 0 and int(no[-1]) == len(m["data"])
    assert all(int(no[i + 1]) >= int(no[i]) for i in range(len(c.files)))
    for i, (_p, _d, fate) in enumerate(c.files):
        if fate == "dropped":
            assert int(no[i + 1]) == int(no[i])
    assert [int(no[i]) for i in m["index"]] == [int(x) for x in off[:-1]]
    # Rule 5's size bound
    n_allowed = sum(1 for p, _, _ in c.files if p.endswith(".pyc"))
    assert len(m["data"]) <= c.total + n_allowed


def test_printable_table_equals_oracle():
    tab = S.prepare_print_table()
    assert tab == [int(so._latin1_printable(b)) for b in range(256)]
    assert sum(tab) == 189


def _sizes(name):
    c = CORPORA[name]
    m = S.prepare_batch_view(scanner(c.config_path), c.raw_files, c.config_path, c.file_patterns, model=True)
    no = m["new_offsets"]
    return c, m, {p: (len(d), int(no[i + 1]) - int(no[i])) for i, (p, d, _) in enumerate(c.files)}


def test_corpora_contain_their_cases():
    c, m, size = _sizes("runs")
    raw, new = size["r/grows.pyc"]
    assert new == raw + 1                                   # some file grows by one
    data = dict((p, d) for p, d, _ in c.files)
    # some run is cut by a file end: the two halves would make a kept run of 6
    assert data["r/end3.pyc"].endswith(b"xyz") and data["r/begin3.pyc"].startswith(b"uvw")
    k = m["index"].index([p for p, _, _ in c.files].index("r/end3.pyc"))
    off = m["offsets"]
    assert m["data"][int(off[k]):int(off[k + 1])] == b"abcdefg\n"
    assert m["data"][int(off[k + 1]):int(off[k + 2])] == b"hijklmn\n"
    # runs of 4 go, runs of 5 stay, whatever delimits them
    for d in PC.RUN_DELIMS:
        i = [p for p, _, _ in c.files].index("r/delim%02x.pyc" % d)
        k = m["index"].index(i)
        assert m["data"][int(off[k]):int(off[k + 1])] == b"".join(bytes([ord("a") + n]) * n + b"\n" for n in range(5, 10))
    # the clean-head .pyc took the text path
    i = [p for p, _, _ in c.files].index("r/clean_head.pyc")
    k = m["index"].index(i)
    assert m["binary"][k] == 0 and m["data"][int(off[k]):int(off[k + 1])] == b"A" * 300 + b"\nab\x00cd\x01e"
    # heads that cross a sub-tile edge and a region edge, of every fate
    c = CORPORA["head_edges"]
    fates = dict((p, f) for p, _, f in c.files)
    for unit in (PC.SUB, PC.REGION):
        crossing = [p for p in PC.head_straddles(c, unit) if "straddle" in p]
        assert {fates[p] for p in crossing} == {"dropped", "printable", "text"}, unit
    # the bound prepared <= total + n_allowed is reached
    c, m, size = _sizes("all_grow")
    assert len(m["data"]) == c.total + len(c.files)
    # the long run is kept whole with one '\n'
    c, m, size = _sizes("long_run")
    assert size["l/run.pyc"] == (200_002, 200_001) and size["l/run_to_end.pyc"] == (70_001, 70_001)
    # every file dropped
    c, m, size = _sizes("all_dropped")
    assert m["index"] == [] and len(m["data"]) == 0 and [int(x) for x in m["offsets"]] == [0]
    # totals 0, 1, 15 (mod 16); 300 tiny files inside one sub-tile
    assert [CORPORA["sizes_mod%d" % r].total % 16 for r in (0, 1, 15)] == [0, 1, 15]
    c = CORPORA["tiny_mixed"]
    starts = np.cumsum([0] + [len(d) for _, d, _ in c.files])
    tiny = [i for i, (p, _, _) in enumerate(c.files) if p[2:3].isdigit()]
    assert len(tiny) == 300 and starts[tiny[0]] // PC.SUB == (starts[tiny[-1] + 1] - 1) // PC.SUB
    assert {f for _, _, f in c.files} == {"text", "printable", "dropped"}
    # runs at every offset -8..+8 around each edge kind: 17 kept, 17 gone
    for name, unit in (("runs_word_edges", PC.WORD), ("runs_subtile_edges", PC.SUB), ("runs_region_edges", PC.REGION)):
        c, m, size = _sizes(name)
        i = [p for p, _, _ in c.files].index("e/edges.pyc")
        k = m["index"].index(i)
        runs = m["data"][int(m["offsets"][k]):int(m["offsets"][k + 1])].split(b"\n")
        assert len(runs) == 18 and all(len(r) == 5 for r in runs[:-1]) and runs[-1] == b""
        b = np.frombuffer(c.files[i][1], np.uint8)
        at = np.flatnonzero((b != 0) & np.concatenate([[True], b[:-1] == 0])) + int(starts_of(c)[i])
        step = max(unit, 64)                                 # one run per edge; 16-byte edges 64 bytes apart
        rel = sorted({int(r) if r <= step // 2 else int(r) - step for r in at % step})
        assert len(at) == 34 and rel == list(range(-8, 9)), name


def starts_of(c):
    return np.cumsum([0] + [len(d) for _, d, _ in c.files])


def test_prepare_batch_device_rejects_null_arguments_cpu():
    L = _lib.lib()
    h, ms = ctypes.c_void_p(), ctypes.c_double()
    off = np.zeros(1, np.uint64)
    assert L.tsg_prepare_batch_device(None, None, off.ctypes.data, 0, None, None, None, None, 0, ctypes.byref(h),
                                      ctypes.byref(ms)) != 0
    assert "NULL" in L.tsg_last_error().decode()
    assert L.tsg_prepare_device_model(None, None, off.ctypes.data, 0, None, None, None, None, None,
                                      ctypes.byref(h)) != 0
    assert "NULL" in L.tsg_last_error().decode()
