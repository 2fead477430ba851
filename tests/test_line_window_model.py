"""Line windows without a GPU: the layout with a line cap (csrc/gather.h
line_window inside plan_gather_windows, through tsg_test_plan_gather_lines)
against a restatement written here from the files' bytes alone -- no table, no
shared code -- and the whole-mode CPU model with the cap
(tsg_scan_device_model_opts2: table-model candidates, the layout, every run
in an allocation of its own, the windowed confirmation, the fallback round)
against the table model and the oracle on every corpus of
tests/_line_window_corpus.py, with the insufficient files equal to the sets
each corpus names for byte windows and for line windows.
"""
import json
import tempfile

import numpy as np
import pytest

import _line_window_corpus as LC
import _window_corpus as WC
from _oracle_pool import oracle_scan_many
from oracle import secret_oracle as so
from trivy_amd import secret as S

NONE, WHOLE, WINDOW = WC.NONE, WC.WHOLE, WC.WINDOW
_SC = {}


def scanner(cfg):
    key = repr(cfg)
    if key not in _SC:
        _SC[key] = S.Scanner(cfg)
    return _SC[key]


# ------------------------------------------------- the rule, from the bytes
def line_window(text, s, before, after, cap):
    """File bytes [a, b) of the window of start s < len(text), and whether a walk ended at the cap."""
    n = len(text)
    t = min(n, s + after)
    # backward: the 3rd '\n' met from s - 1 down, no lower than s - cap; the '\n' itself belongs to the window
    lower = max(0, s - cap)
    found = [i for i in range(s - 1, lower - 1, -1) if text[i] == 10][:3]
    back = found[2] if len(found) == 3 else lower
    capped = len(found) < 3 and lower > 0
    a = min(max(s - before, 0), back)
    # forward: 2 + the '\n' of [s, t) many, from t on, no further than t + cap
    need = 2 + text[s:t].count(b"\n")
    upper = min(n, t + cap)
    pos, got = t, 0
    fwd = upper
    while pos < upper:
        k = text.find(b"\n", pos, upper)
        if k < 0:
            break
        got += 1
        if got == need:
            fwd = k + 1
            break
        pos = k + 1
    capped = capped or (got < need and t + cap < n)
    b = max(t, fwd, s + 1)
    return a, b, capped


def python_layout(texts, cands, fflags, all_rules, windowable, chunk, window, cap, lead=0):
    """The windowed layout with a line cap, pass for pass in sets and numpy; cap 0: byte windows."""
    before, after, min_file = window
    lens = np.array([len(t) for t in texts], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    nfiles, total = len(texts), int(off[-1])
    nchunks = -(-total // chunk)
    has, whole = np.zeros(nfiles, bool), np.zeros(nfiles, bool)
    for f, r, s in cands:
        if lead <= f < nfiles:
            has[f] = True
            if r >= len(windowable) or not windowable[r] or s >= lens[f]:
                whole[f] = True
    cls = np.zeros(nfiles, np.uint8)
    marks = np.zeros(nchunks, bool)
    for f in range(lead, nfiles):
        if all_rules or fflags[f] or has[f]:
            w = all_rules or fflags[f] or whole[f] or lens[f] < min_file or lens[f] == 0
            cls[f] = WHOLE if w else WINDOW
            if not w:
                marks[off[f] // chunk] = True
    widened = capped = 0
    for f, r, s in cands:
        if lead <= f < nfiles and cls[f] == WINDOW:
            plo, phi = WC.window_chunks(int(off[f]), int(lens[f]), s, before, after, chunk)
            lo, hi = plo, phi
            if cap:
                a, b, cp = line_window(texts[f], s, before, after, cap)
                lo, hi = (int(off[f]) + a) // chunk, (int(off[f]) + b - 1) // chunk
                widened += lo < plo or hi > phi
                capped += cp
            nfc = (off[f + 1] - 1) // chunk - off[f] // chunk + 1
            if 2 * (hi - lo + 1) > nfc:
                whole[f] = True
            else:
                marks[lo:hi + 1] = True
    window_marks = marks.copy()
    for f in range(lead, nfiles):
        if cls[f] == WINDOW:
            c0, c1 = off[f] // chunk, (off[f + 1] - 1) // chunk
            if whole[f] or 2 * int(window_marks[c0:c1 + 1].sum()) > c1 - c0 + 1:
                cls[f] = WHOLE
    for f in range(lead, nfiles):
        if cls[f] == WHOLE:
            if lens[f] == 0:
                if off[f] // chunk < nchunks:
                    marks[off[f] // chunk] = True
            else:
                marks[off[f] // chunk:(off[f + 1] - 1) // chunk + 1] = True
    m = np.concatenate([[False], marks, [False]]).astype(np.int8)
    starts, ends = np.nonzero(np.diff(m) == 1)[0], np.nonzero(np.diff(m) == -1)[0]
    in_front = np.concatenate([[0], np.cumsum(marks)])
    runs = np.array([(a * chunk, in_front[a] * chunk, min(b * chunk, total) - a * chunk) for a, b in zip(starts, ends)],
                    np.uint64).reshape(-1, 3)
    gathered = int(runs[-1][1] + runs[-1][2]) if len(runs) else 0
    first = np.full(nfiles, 0xFFFFFFFF, np.uint32)
    for f in range(lead, nfiles):
        if cls[f] != NONE and off[f] // chunk < nchunks:
            k = np.searchsorted(runs[:, 0].astype(np.int64), off[f] // chunk * chunk, side="right") - 1
            first[f] = k
    return {"cls": cls, "marks": marks, "runs": runs, "total": -(-gathered // 64) * 64, "first_run": first,
            "widened": widened, "capped": capped}


def check_layout(texts, cands, fflags, all_rules, windowable, chunk, window, cap, lead=0):
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    got = S.plan_gather_lines(b"".join(bytes(t) for t in texts), off, cands, fflags, all_rules, windowable, chunk, window,
                              cap, lead=lead)
    want = python_layout([bytes(t) for t in texts], cands, fflags, all_rules, windowable, chunk, window, cap, lead)
    assert np.array_equal(got["cls"], want["cls"]), (got["cls"], want["cls"])
    assert np.array_equal(got["marks"].astype(bool), want["marks"]), np.nonzero(got["marks"].astype(bool) != want["marks"])
    assert np.array_equal(got["runs"], want["runs"]) and got["total"] == want["total"]
    assert np.array_equal(got["first_run"], want["first_run"])
    assert (got["widened"], got["capped"]) == (want["widened"], want["capped"])
    return got


def test_layout_against_the_restatement_random():
    rng = np.random.RandomState(11)
    for trial in range(200):
        chunk = int(rng.choice([128, 256, 1024]))
        nfiles = int(rng.randint(1, 10))
        texts = []
        for _ in range(nfiles):
            n = int(rng.choice([0, 1, 57, chunk - 1, chunk, chunk + 1, 5 * chunk + 3, 40 * chunk, 90 * chunk + 77]))
            t = rng.randint(97, 123, n).astype(np.uint8)
            density = float(rng.choice([0.0, 0.0005, 0.003, 0.02, 0.3]))   # lines of every length, none at all too
            t[rng.rand(n) < density] = 10
            texts.append(t.tobytes())
        lead = int(rng.randint(0, 2)) if nfiles > 1 else 0
        windowable = np.array([1, 1, 0, 1], np.uint8)
        cands = []
        for _ in range(int(rng.randint(0, 16))):
            f = int(rng.randint(0, nfiles + 1))
            n = len(texts[f]) if f < nfiles else 10
            s = int(rng.randint(0, n + 2)) if rng.rand() < 0.95 else 0xFFFFFFFFFFFFFFFF
            cands.append((f, int(rng.choice([0, 1, 3, 3, 3, 2, 9])), s))
        cands += cands[:2]
        fflags = (rng.rand(nfiles) < 0.05).astype(np.uint32)
        window = (int(rng.choice([0, 5, 100, 700])), int(rng.choice([1, 64, 300, 3 * chunk + 5])), int(rng.choice([0, 1000])))
        cap = int(rng.choice([1, 100, chunk, 3 * chunk + 17, 16384, 1 << 20]))
        check_layout(texts, cands, fflags, trial % 19 == 0, windowable, chunk, window, cap, lead)


def model_inputs(c):
    sc = scanner(c.cfg)
    cands, info = S.prefilter_table_model(sc, c.args, with_info=True)
    rows, _ = S.windowable_rows(sc)
    flat = [(f, r, int(s)) for (f, r), v in cands.items() for s in v]
    return sc, cands, flat, info["special"].astype(np.uint32), rows


@pytest.mark.parametrize("name", LC.NAMES)
def test_layout_of_every_corpus(name):
    c = LC.corpus(name)
    sc, cands, flat, special, rows = model_inputs(c)
    LC.holds(c, cands)
    texts = [a.Content for a in c.args]
    line = check_layout(texts, flat, special, False, rows, c.chunk, c.window, c.cap)
    plain = check_layout(texts, flat, special, False, rows, c.chunk, c.window, 0)
    for f, want in c.classes.items():
        assert plain["cls"][f] == want, (name, f, plain["cls"])
    for f, want in c.line_classes.items():
        assert line["cls"][f] == want, (name, f, line["cls"])
    # the line windows hold the byte windows
    if np.array_equal(line["cls"], plain["cls"]):
        assert (line["marks"] >= plain["marks"]).all()
    if name == "merging":
        off = c.offsets
        in_f0 = lambda lay: int(((lay["runs"][:, 0].astype(np.int64) < off[1])).sum())
        assert in_f0(plain) == 3 and in_f0(line) == 2          # the head chunk and two windows; the windows as one run
    if name.startswith("cap_"):
        assert (line["capped"] > 0) == (c.insufficient == [0])
    if name in ("long_own_line", "long_neighbours", "chunk_phases", "merging"):
        assert line["widened"] > 0


def test_cap_zero_is_the_byte_window_layout_bit_for_bit():
    for name in WC.NAMES:
        c = WC.corpus(name)
        sc, cands, flat, special, rows = model_inputs(c)
        all_rules = name == "whole_mode1"
        base = S.plan_gather_windows(c.offsets, flat, special, all_rules, rows, c.chunk, c.window)
        data = b"".join(a.Content for a in c.args)
        for d in (data, np.zeros(0, np.uint8)):                 # cap 0 never reads the data
            if isinstance(d, np.ndarray) and len(data):
                d = np.zeros(len(data), np.uint8)
            got = S.plan_gather_lines(d, c.offsets, flat, special, all_rules, rows, c.chunk, c.window, 0)
            for k in ("cls", "first_run", "marks", "runs"):
                assert got[k].tobytes() == base[k].tobytes() and got[k].dtype == base[k].dtype, (name, k)
            assert got["total"] == base["total"] and got["widened"] == got["capped"] == 0


# ------------------------------------------------------------ the model
_ORACLE = {}


def oracle(c):
    if c.name not in _ORACLE:
        cfg = None
        if c.cfg is not None:
            with tempfile.NamedTemporaryFile("w", suffix=".yaml") as fp:
                json.dump(c.cfg, fp)
                fp.flush()
                cfg = so.parse_config(fp.name)
        _ORACLE[c.name] = oracle_scan_many([(a.FilePath, a.Content, a.Binary) for a in c.args], procs=4, cfg=cfg)
    return _ORACLE[c.name]


@pytest.mark.parametrize("name", LC.NAMES)
def test_line_window_model(name):
    c = LC.corpus(name)
    sc, cands, flat, special, rows = model_inputs(c)
    want = S.scan_device_model(sc, c.args, c.chunk)            # the device-only model without windows
    assert want == S.scan_table_model(sc, c.args) == oracle(c)
    got, rec, fb, st = S.scan_device_model_windows(sc, c.args, c.chunk, c.window, window_lines=c.cap)
    assert got == want
    assert rec["insufficient"] == c.insufficient, (name, rec["insufficient"])
    pgot, prec, pfb, pst = S.scan_device_model_windows(sc, c.args, c.chunk, c.window)
    assert pgot == want
    assert prec["insufficient"] == c.plain, (name, prec["insufficient"])
    for f, cls in c.line_classes.items():
        assert rec["cls"][f] == cls, (f, rec["cls"])
    # the record against the layout hook, the stats against the record
    lay = S.plan_gather_lines(b"".join(a.Content for a in c.args), c.offsets, flat, special, False, rows, c.chunk,
                              c.window, c.cap)
    assert np.array_equal(rec["cls"], lay["cls"]) and np.array_equal(rec["runs"], lay["runs"]) and rec["total"] == lay["total"]
    data, _off = S.pack(c.args)
    for src, dst, n in rec["runs"].astype(np.int64):
        assert np.array_equal(rec["bytes"][dst:dst + n], data[src:src + n])
    assert st["fallback_files"] == len(c.insufficient)
    assert st["window_files"] == int((rec["cls"] == WINDOW).sum()) - len(c.insufficient)
    assert st["window_bytes"] == rec["total"] and st["gather_bytes"] == rec["total"] + st["fallback_bytes"]
    assert (st["line_widened"], st["line_capped"]) == (lay["widened"], lay["capped"])
    assert (fb is None or fb["total"] == 0) == (not c.insufficient)
    if name in LC.NO_FALLBACK:
        assert st["fallback_files"] == 0
    # cap 0 through the new hook: the byte-window model, record for record
    zgot, zrec, zfb, zst = S.scan_device_model_windows(sc, c.args, c.chunk, c.window, window_lines=0)
    assert zgot == pgot and zrec["insufficient"] == prec["insufficient"]
    for k in ("cls", "goff", "runs", "bytes"):
        assert np.array_equal(zrec[k], prec[k]), k
    for k in pst:
        assert zst[k] == pst[k], k
    assert zst["line_widened"] == zst["line_capped"] == 0


def test_the_corpus_exercises_the_feature():
    # corpus 1 falls back under byte windows and not under line windows, and crosses less for it
    c = LC.corpus("long_own_line")
    sc = scanner(c.cfg)
    _, prec, _, pst = S.scan_device_model_windows(sc, c.args, c.chunk, c.window)
    _, rec, _, st = S.scan_device_model_windows(sc, c.args, c.chunk, c.window, window_lines=c.cap)
    assert prec["insufficient"] == [0, 1] and pst["fallback_files"] == 2
    assert rec["insufficient"] == [] and st["fallback_files"] == 0 and st["window_files"] == 2
    assert st["gather_bytes"] < pst["gather_bytes"] // 10


@pytest.mark.parametrize("reverse", [False, True])
def test_the_whole_corpus_as_one_batch(reverse):
    c = LC.combined(reverse)
    sc, cands, flat, special, rows = model_inputs(c)
    check_layout([a.Content for a in c.args], flat, special, False, rows, c.chunk, c.window, c.cap)
    want = S.scan_table_model(sc, c.args)
    got, rec, fb, st = S.scan_device_model_windows(sc, c.args, c.chunk, c.window, window_lines=c.cap)
    assert got == want
    names = [a.FilePath for a in c.args]
    # the line of 40 KiB under the cap of 16 KiB and the key block longer than `after`, whatever the files' phases
    assert [names[f] for f in rec["insufficient"]] == [n for n in names if n in ("k/line40k.log", "m/long.pem")]


def test_other_chunks_windows_and_caps():
    for name in ("long_own_line", "file_edges", "shared_chunks", "multi_line"):
        c = LC.corpus(name)
        sc = scanner(c.cfg)
        want = S.scan_table_model(sc, c.args)
        for chunk, window, cap in ((256, (8, 40, 0), 777), (512, (700, 700, 0), 4096), (1024, (3, 3, 0), 100000),
                                   (128, (64, 64, 0), 1)):
            got, rec, fb, st = S.scan_device_model_windows(sc, c.args, chunk, window, window_lines=cap)
            assert got == want, (name, chunk, window, cap)


def test_window_lines_needs_a_window():
    c = LC.corpus("long_own_line")
    sc = scanner(c.cfg)
    with pytest.raises(ValueError):
        S.scan_device_model_windows(sc, c.args, c.chunk, None, window_lines=4096)
    with pytest.raises(Exception, match="window_line_cap needs"):
        S.scan_device_model_windows(sc, c.args, c.chunk, (0, 0, 0), window_lines=4096)
    with pytest.raises(ValueError):
        sc.ScanBatchDevice(None, [0], [], window_lines=4096)
    with pytest.raises(ValueError):
        sc.ScanLayersCompressedDevice([], window_lines=4096)
    with pytest.raises(ValueError):
        sc.ScanLayersGzipDevice([], window_lines=4096)
