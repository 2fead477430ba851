#!/usr/bin/env python
"""A layer tar in HBM to findings: the device walk beside the route a caller
has without it (tooling; not a bench.py leg).

  python tools/tar_device_probe.py [--gb 1] [--steps 3] [--seed N]

One config-3-shaped layer (workload/synth.py's image files, written as one PAX
tar) is held in HBM.  Timed on the same box, per step:
  device   tsg_prepare_layer_tar_device -> tsg_scan_batch_device
  host     D2H copy of the whole tar into pinned memory ->
           tsg_prepare_layer_tar_opts(pinned) -> tsg_scan_batch
It prints one JSON line: both routes' wall times and rates over the tar's
bytes, their parts, the device walk's blocks / marked blocks / gathered bytes /
fallback reads / retries, the kernel times of the mark-compact pass and of the
content pass's four passes, and whether the findings are equal (exit 1 if not)."""
import argparse
import ctypes
import json
import os
import sys
import tarfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trivy_amd import _lib  # noqa: E402
from trivy_amd import secret as S  # noqa: E402
from workload import synth  # noqa: E402


def layer_tar(corpus):
    """The corpus' files as one PAX tar (tarfile's headers, numpy's copies)."""
    heads, total = [], 0
    for i, p in enumerate(corpus.paths):
        ti = tarfile.TarInfo(p.lstrip("/"))
        ti.size = int(corpus.offsets[i + 1] - corpus.offsets[i])
        ti.mode = 0o644
        h = ti.tobuf(tarfile.PAX_FORMAT)
        heads.append(h)
        total += len(h) + (ti.size + 511) // 512 * 512
    tar = np.zeros(total + 1024, np.uint8)
    pos = 0
    for i, h in enumerate(heads):
        tar[pos:pos + len(h)] = np.frombuffer(h, np.uint8)
        pos += len(h)
        a, b = int(corpus.offsets[i]), int(corpus.offsets[i + 1])
        tar[pos:pos + b - a] = corpus.data[a:b]
        pos += (b - a + 511) // 512 * 512
    return tar


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x71215EC7)
    a = ap.parse_args()
    L = _lib.lib()
    corpus = synth.generate(int(a.gb * 1e9), seed=a.seed, sizes="small", layout="image")
    tar = layer_tar(corpus)
    n = len(tar)
    d_tar = torch.from_numpy(tar).to("cuda:0")
    d_dst = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    h_tar = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    torch.cuda.synchronize()
    sc = S.Scanner(None)
    eng = sc.engine()
    o_dev, keep1 = _lib.feed_opts()
    o_host, keep2 = _lib.feed_opts(pinned=True)

    def paths_of(h):
        pp, pl = ctypes.POINTER(ctypes.c_char_p)(), ctypes.POINTER(ctypes.c_uint32)()
        _lib.check(L.tsg_prepared_paths(h, ctypes.byref(pp), ctypes.byref(pl)))
        return pp, ctypes.cast(pl, ctypes.c_void_p)

    def view_of(h):
        d, o, ix, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nk = ctypes.c_uint32()
        _lib.check(L.tsg_prepared_view(h, ctypes.byref(d), ctypes.byref(o), ctypes.byref(ix), ctypes.byref(b),
                                       ctypes.byref(nk)))
        return d, o, b, nk.value

    def device_route(last):
        h, ms, res = ctypes.c_void_p(), ctypes.c_double(), ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib.check(L.tsg_prepare_layer_tar_device(eng, ctypes.c_void_p(d_tar.data_ptr()), n, ctypes.byref(o_dev),
                                                  ctypes.c_void_p(d_dst.data_ptr()), n + 64, ctypes.byref(h),
                                                  ctypes.byref(ms)))
        t1 = time.perf_counter()
        _d, o, b, nk = view_of(h)
        pp, pl = paths_of(h)
        _lib.check(L.tsg_scan_batch_device(eng, ctypes.c_void_p(d_dst.data_ptr()), o, nk, pp, pl, b, ctypes.byref(res)))
        t2 = time.perf_counter()
        info = None
        if last:
            blocks, marked, gbytes = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            fb, retries, scan_ms = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
            _lib.check(L.tsg_prepared_tar_stats(h, ctypes.byref(blocks), ctypes.byref(marked), ctypes.byref(gbytes),
                                                ctypes.byref(fb), ctypes.byref(retries), ctypes.byref(scan_ms)))
            passes = (ctypes.c_double * 4)()
            _lib.check(L.tsg_prepared_pass_ms(h, passes))
            info = dict(kept=nk, blocks=blocks.value, marked=marked.value, gathered_bytes=gbytes.value,
                        fallback_reads=fb.value, retries=retries.value, tar_scan_kernel_ms=round(scan_ms.value, 3),
                        content_pass_kernel_ms=[round(x, 3) for x in passes], findings=_lib.result_json(res),
                        gather=_lib.result_gather_stats(res))
        L.tsg_result_free(res)
        L.tsg_prepared_free(h)
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, info

    def host_route(last):
        h, res = ctypes.c_void_p(), ctypes.c_void_p()
        t0 = time.perf_counter()
        h_tar.copy_(d_tar, non_blocking=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _lib.check(L.tsg_prepare_layer_tar_opts(sc._rs, ctypes.c_void_p(h_tar.data_ptr()), n, ctypes.byref(o_host),
                                                ctypes.byref(h)))
        t2 = time.perf_counter()
        d, o, b, nk = view_of(h)
        pp, pl = paths_of(h)
        _lib.check(L.tsg_scan_batch(eng, d, o, nk, pp, pl, b, ctypes.byref(res)))
        t3 = time.perf_counter()
        js = _lib.result_json(res) if last else None
        L.tsg_result_free(res)
        L.tsg_prepared_free(h)
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, js

    dev, host = [], []
    info = hjs = None
    for k in range(a.steps + 1):                        # the first step warms the lanes and buffers up
        r = device_route(k == a.steps)
        if k:
            dev.append(r[:2])
        info = r[2]
    for k in range(a.steps + 1):
        r = host_route(k == a.steps)
        if k:
            host.append(r[:3])
        hjs = r[3]
    del keep1, keep2
    djs = info.pop("findings")
    gs = info.pop("gather")
    best_dev = min(dev, key=sum)
    best_host = min(host, key=sum)
    gb = n / 1e9
    line = {
        "probe": "tar_device", "tar_bytes": n, "files": len(corpus.paths), "steps": a.steps,
        "device_ms": round(sum(best_dev), 3), "device_parts_ms": {"walk_prepare": round(best_dev[0], 3),
                                                                  "scan_device": round(best_dev[1], 3)},
        "host_ms": round(sum(best_host), 3), "host_parts_ms": {"d2h_copy": round(best_host[0], 3),
                                                               "prepare_layer_tar_pinned": round(best_host[1], 3),
                                                               "scan_batch": round(best_host[2], 3)},
        "device_gbps": round(gb / (sum(best_dev) / 1e3), 2), "host_gbps": round(gb / (sum(best_host) / 1e3), 2),
        "findings_equal": djs == hjs, "findings": sum(len(s["Findings"]) for s in djs),
        "marked_share_of_blocks": round(info["marked"] / max(info["blocks"], 1), 5),
        "confirm_gather_bytes": gs["gather_bytes"],
    }
    line.update(info)
    print(json.dumps(line), flush=True)
    return 0 if line["findings_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
