#!/usr/bin/env python
"""The device-only scan beside the resident scan on one batch (tooling; not a
bench.py leg).

  python tools/device_scan_probe.py [--config 1|2] [--gb 1] [--steps 3] [--seed N]
                                    [--windows 512,2048,8192] [--min-file 65536] [--line-cap 16384]
                                    [--model [--chunk 2048]]

For a config-1-shaped (lognormal source files) or config-2-shaped (log-uniform
64 B - 64 MB files) batch of workload/synth.py held in HBM it prints one JSON
line: the resident rate (tsg_scan_batch_resident, with the host copy), the
device-only rate (tsg_scan_batch_device, without), whether the findings are
equal, the gather's files / bytes / runs / kernel ms, and the time of one
hipMemcpyAsync of gather_bytes from device memory into pinned host memory on
the same box -- the yardstick for the gather's direct stores.  With --windows
the device-only scan is also run with windows of each given size on either
side of a candidate (tsg_scan_batch_device_opts, files below --min-file whole):
"windows" then holds, per size, the step times and rate, whether the findings
equal the resident scan's, the gathered bytes, the windowed files and runs, and
the files and bytes of the fallback round.  With --line-cap N every window
size is run twice, the byte windows and then the same with the line cap
(tsg_scan_batch_device_opts2), in that order size by size: the line rows carry
"line_cap", the candidates widened and capped and the line pass's own kernel
time per step and per piece.

--model runs no GPU code: the same rows from the whole-mode CPU model
(tsg_scan_device_model_opts2: the table model's candidates, the layout, the
windowed confirmation, the fallback round) on one segment with K1 chunks of
--chunk bytes -- windowed files, fallbacks and gathered bytes per setting."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trivy_amd import _lib  # noqa: E402
from trivy_amd import secret as S  # noqa: E402
from workload import synth  # noqa: E402


def d2h_copy_ms(nbytes, reps=5):
    """One async D2H copy of nbytes from device memory into pinned memory: best of reps, ms."""
    import torch
    if nbytes == 0:
        return 0.0
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src, non_blocking=True)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def model_rows(a, L, sc, corpus, off, paths, lens, settings):
    """--model: one JSON line of the CPU model's counts per setting."""
    nfiles = len(corpus.paths)
    data = np.ascontiguousarray(corpus.data)
    rows, want = [], None
    for w, cap in [(None, None)] + settings:
        res = ctypes.c_void_p()
        t0 = time.perf_counter()
        opts = _lib.scan_opts2((w or 0, w or 0, a.min_file), cap or 0)
        _lib.check(L.tsg_scan_device_model_opts2(sc._rs, data.ctypes.data, off.ctypes.data, nfiles, paths, lens, None,
                                                 a.chunk, ctypes.byref(opts), None, None, ctypes.byref(res)))
        js = _lib.result_json(res)
        gs = _lib.result_gather_stats(res)
        gs.update(_lib.result_gather_window_stats(res))
        gs.update(_lib.result_gather_line_stats(res))
        L.tsg_result_free(res)
        if want is None:
            want = js
        rows.append({"before": w, "after": w, "line_cap": cap, "findings_equal": js == want,
                     "gather_files": gs["gather_files"], "gather_bytes": gs["gather_bytes"],
                     "gather_share_of_batch": round(gs["gather_bytes"] / max(corpus.nbytes, 1), 4),
                     "window_files": gs["window_files"], "window_runs": gs["window_runs"], "window_bytes": gs["window_bytes"],
                     "fallback_files": gs["fallback_files"], "fallback_bytes": gs["fallback_bytes"],
                     "line_widened": gs["line_widened"], "line_capped": gs["line_capped"],
                     "model_s": round(time.perf_counter() - t0, 1)})
    print(json.dumps({"probe": "device_scan_model", "config": a.config, "bytes": corpus.nbytes, "files": nfiles,
                      "chunk": a.chunk, "min_file": a.min_file, "rows": rows}), flush=True)
    return 0 if all(r["findings_equal"] for r in rows) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=[1, 2])
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x71215EC7)
    ap.add_argument("--windows", default="", help="window sizes in bytes (each side of a candidate), comma separated")
    ap.add_argument("--min-file", type=int, default=65536, help="files below this many bytes are gathered whole")
    ap.add_argument("--line-cap", type=int, default=0, help="also run every window size with this line cap (bytes)")
    ap.add_argument("--model", action="store_true", help="the CPU model's counts instead of a GPU run")
    ap.add_argument("--chunk", type=int, default=2048, help="K1 chunk bytes for --model")
    a = ap.parse_args()
    L = _lib.lib()
    corpus = synth.generate(int(a.gb * 1e9), seed=a.seed, sizes="lognormal" if a.config == 1 else "loguniform")
    nfiles, nbytes = len(corpus.paths), corpus.nbytes
    data = corpus.data
    off = np.ascontiguousarray(corpus.offsets, dtype=np.uint64)
    sc = S.Scanner(None)
    paths, lens, _keep = _lib.pack_paths(corpus.paths)
    sizes = [int(x) for x in a.windows.split(",") if x]
    settings = []                                        # (window size, line cap or None), plain and line rows alternating
    for w in sizes:
        settings.append((w, None))
        if a.line_cap:
            settings.append((w, a.line_cap))
    if a.model:
        return model_rows(a, L, sc, corpus, off, paths, lens, settings)
    import torch
    d = torch.from_numpy(data).to("cuda:0")
    torch.cuda.synchronize()
    eng = sc.engine()

    def scan(device_only, window=None, cap=None):
        res = ctypes.c_void_p()
        t0 = time.perf_counter()
        if cap is not None:
            opts = _lib.scan_opts2(window, cap)
            _lib.check(L.tsg_scan_batch_device_opts2(eng, ctypes.c_void_p(d.data_ptr()), off.ctypes.data, nfiles, paths,
                                                     lens, None, ctypes.byref(opts), ctypes.byref(res)))
        elif window is not None:
            opts = _lib.scan_opts(window)
            _lib.check(L.tsg_scan_batch_device_opts(eng, ctypes.c_void_p(d.data_ptr()), off.ctypes.data, nfiles, paths,
                                                    lens, None, ctypes.byref(opts), ctypes.byref(res)))
        elif device_only:
            _lib.check(L.tsg_scan_batch_device(eng, ctypes.c_void_p(d.data_ptr()), off.ctypes.data, nfiles, paths,
                                               lens, None, ctypes.byref(res)))
        else:
            _lib.check(L.tsg_scan_batch_resident(eng, ctypes.c_void_p(d.data_ptr()), data.ctypes.data, off.ctypes.data,
                                                 nfiles, paths, lens, None, ctypes.byref(res)))
        return res, (time.perf_counter() - t0) * 1e3

    out = {}
    runs = [("resident", False, None, None), ("device_only", True, None, None)]
    runs += [("window_%d_%s" % (w, cap), True, (w, w, a.min_file), cap) for w, cap in settings]
    for name, dev, window, cap in runs:
        times, js, st, gs = [], None, None, None
        for k in range(a.steps + 1):                    # the first step warms the lanes and buffers up
            res, ms = scan(dev, window, cap)
            if k:
                times.append(ms)
            if k == a.steps:
                js = _lib.result_json(res)
                st = _lib.result_stats(res)
                gs = _lib.result_gather_stats(res)
                gs.update(_lib.result_gather_window_stats(res))
                gs.update(_lib.result_gather_line_stats(res))
            L.tsg_result_free(res)
        out[name] = (times, js, st, gs)
    tr, jr, sr, _ = out["resident"]
    td, jd, sd, gd = out["device_only"]
    copy_ms = d2h_copy_ms(int(gd["gather_bytes"]))
    gb = nbytes / 1e9
    line = {
        "probe": "device_scan", "config": a.config, "bytes": nbytes, "files": nfiles, "steps": a.steps,
        "resident_ms": [round(x, 3) for x in tr], "device_only_ms": [round(x, 3) for x in td],
        "resident_gbps": round(gb / (min(tr) / 1e3), 1), "device_only_gbps": round(gb / (min(td) / 1e3), 1),
        "findings_equal": jr == jd, "findings": int(sd["findings"]),
        "confirm_files": int(sd["confirm_files"]), "pieces": int(sd["pieces"]),
        "gather_files": gd["gather_files"], "gather_bytes": gd["gather_bytes"], "gather_runs": gd["gather_runs"],
        "gather_ms": round(gd["gather_ms"], 3), "gather_retries": gd["gather_retries"],
        "gather_share_of_batch": round(gd["gather_bytes"] / max(nbytes, 1), 4),
        "gather_gbps": round(gd["gather_bytes"] / 1e6 / gd["gather_ms"], 1) if gd["gather_ms"] else None,
        "d2h_copy_ms": round(copy_ms, 3),
        "d2h_copy_gbps": round(gd["gather_bytes"] / 1e6 / copy_ms, 1) if copy_ms else None,
        "gather_over_copy": round(gd["gather_ms"] / copy_ms, 2) if copy_ms else None,
    }
    line["windows"] = []
    for w, cap in settings:
        tw, jw, sw, gw = out["window_%d_%s" % (w, cap)]
        row = {}
        if cap is not None:
            row = {"line_cap": cap, "line_widened": gw["line_widened"], "line_capped": gw["line_capped"],
                   "line_ms": round(gw["line_ms"], 4), "line_ms_per_piece": round(gw["line_ms"] / max(int(sw["pieces"]), 1), 4)}
        line["windows"].append({
            **row, "chunk_bytes": int(sw["chunk_bytes"]), "pieces": int(sw["pieces"]),
            "before": w, "after": w, "min_file": a.min_file, "ms": [round(x, 3) for x in tw],
            "gbps": round(gb / (min(tw) / 1e3), 1), "findings_equal": jw == jr,
            "gather_files": gw["gather_files"], "gather_bytes": gw["gather_bytes"], "gather_runs": gw["gather_runs"],
            "gather_share_of_batch": round(gw["gather_bytes"] / max(nbytes, 1), 4), "gather_ms": round(gw["gather_ms"], 3),
            "window_files": gw["window_files"], "window_runs": gw["window_runs"], "window_bytes": gw["window_bytes"],
            "fallback_files": gw["fallback_files"], "fallback_bytes": gw["fallback_bytes"],
            "fallback_share_of_windowed": round(gw["fallback_files"] / max(gw["fallback_files"] + gw["window_files"], 1), 4)})
    print(json.dumps(line), flush=True)
    return 0 if line["findings_equal"] and all(x["findings_equal"] for x in line["windows"]) else 1


if __name__ == "__main__":
    sys.exit(main())
