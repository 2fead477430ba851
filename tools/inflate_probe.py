#!/usr/bin/env python
"""Gzip layers inflated on the GPU: rates of tsg_inflate_gzip_device and the
chain behind it beside the route a caller has without it (tooling; not a
bench.py leg).

  python tools/inflate_probe.py [--mb 8] [--steps 2] [--streams 1,16,256,1024]
                                [--layers 1,4,16,64] [--out profiles/inflate_probe_X.json]

One config-3-shaped layer (workload/synth.py's image files as one PAX tar) is
gzipped at level 6.  Measured on the same box:
  inflate   N equal streams of it in one tsg_inflate_gzip_device call, N from
            --streams: kernel time (device events) of the inflate and the
            checksum kernel, wall time of the call, MB/s of output per stream
            and GB/s of output over all -- after a warm-up call at every N
  zlib      Python's zlib.decompress of the same blob on one thread
  chains    for N layers from --layers, wall time to findings of
              new       ScanLayersGzipDevice: upload of the compressed bytes ->
                        inflate -> PrepareLayerTarDevice -> ScanBatchDevice
              existing  per layer zlib.decompress on the host -> upload of the
                        tar -> PrepareLayerTarDevice -> ScanBatchDevice
            with the bytes each sends over the link, and whether the findings
            are equal (exit 1 if not).
It prints one JSON line and writes it to --out."""
import argparse
import ctypes
import gzip
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from trivy_amd import _lib  # noqa: E402
from trivy_amd import secret as S  # noqa: E402
from workload import synth  # noqa: E402
from tar_device_probe import layer_tar  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=8.0)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--streams", default="1,16,256,1024")
    ap.add_argument("--layers", default="1,4,16,64")
    ap.add_argument("--seed", type=int, default=0x71215EC7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = _lib.lib()
    corpus = synth.generate(int(a.mb * 1e6), seed=a.seed, sizes="small", layout="image")
    tar = layer_tar(corpus).tobytes()
    blob = gzip.compress(tar, 6, mtime=0)
    n, z = len(tar), len(blob)
    sc = S.Scanner(None)
    eng = sc.engine()
    line = {"probe": "inflate", "tar_bytes": n, "gz_bytes": z, "ratio": round(n / z, 3), "files": len(corpus.paths),
            "steps": a.steps}

    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        assert len(zlib.decompress(blob, 31)) == n
        t.append(time.perf_counter() - t0)
    line["zlib_one_thread_mbps"] = round(n / 1e6 / min(t), 1)

    d_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to("cuda:0")
    cap = (n + 15) & ~15
    rates = []
    for ns in [int(x) for x in a.streams.split(",")]:
        d_gz = torch.cat([d_blob.repeat(ns), torch.zeros(16, dtype=torch.uint8, device="cuda:0")])
        dst = torch.empty(ns * cap + 16, dtype=torch.uint8, device="cuda:0")
        go = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(z))
        do = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(cap))
        out_lens, status = np.zeros(ns, np.uint64), np.zeros(ns, np.int32)
        torch.cuda.synchronize()
        runs = []
        for k in range(a.steps + 1):             # the first call warms up
            ms = ctypes.c_double()
            t0 = time.perf_counter()
            _lib.check(L.tsg_inflate_gzip_device(eng, ctypes.c_void_p(d_gz.data_ptr()), go.ctypes.data, ns,
                                                 ctypes.c_void_p(dst.data_ptr()), do.ctypes.data, out_lens.ctypes.data,
                                                 status.ctypes.data, ctypes.byref(ms)))
            wall = (time.perf_counter() - t0) * 1e3
            ims, cms = ctypes.c_double(), ctypes.c_double()
            L.tsg_test_inflate_last_stats(ctypes.byref(ims), ctypes.byref(cms), None, None)
            if k:
                runs.append((wall, ims.value, cms.value))
        assert (out_lens == n).all()
        first = dst[:n].cpu().numpy().tobytes() == tar and dst[(ns - 1) * cap:(ns - 1) * cap + n].cpu().numpy().tobytes() == tar
        best = min(runs)
        rates.append({"streams": ns, "output_correct": bool(first), "wall_ms": round(best[0], 3),
                      "inflate_kernel_ms": round(best[1], 3), "crc_kernel_ms": round(best[2], 3),
                      "per_stream_mbps": round(n / 1e6 / (best[1] / 1e3), 2),
                      "aggregate_gbps_kernel": round(ns * n / 1e9 / (best[1] / 1e3), 3),
                      "aggregate_gbps_wall": round(ns * n / 1e9 / (best[0] / 1e3), 3),
                      "all_wall_ms": [round(r[0], 3) for r in runs]})
        del d_gz, dst
    line["inflate"] = rates

    chains, equal = [], True
    h_tar = torch.empty(n + 16, dtype=torch.uint8).pin_memory()
    for nl in [int(x) for x in a.layers.split(",")]:
        blobs = [blob] * nl
        new_t, old_t, new_f, old_f = [], [], None, None
        for k in range(a.steps + 1):
            t0 = time.perf_counter()
            layers = sc.ScanLayersGzipDevice(blobs)
            t1 = time.perf_counter()
            old = []
            for b in blobs:
                raw = zlib.decompress(b, 31)
                h_tar.numpy()[:n] = np.frombuffer(raw, np.uint8)
                d_tar = h_tar.to("cuda:0", non_blocking=True)
                p_dst, offs, paths, binf, _walk, _ms = sc.PrepareLayerTarDevice(d_tar, n)
                old.append(sc.ScanBatchDevice(p_dst, offs, paths, binf))
            t2 = time.perf_counter()
            if k:
                new_t.append((t1 - t0) * 1e3)
                old_t.append((t2 - t1) * 1e3)
            new_f, old_f = [l[2] for l in layers], old
        equal = equal and new_f == old_f
        chains.append({"layers": nl, "new_ms": round(min(new_t), 2), "existing_ms": round(min(old_t), 2),
                       "new_link_bytes_up": nl * z, "existing_link_bytes_up": nl * n,
                       "findings": sum(len(s["Findings"]) for l in new_f for s in l),
                       "all_new_ms": [round(x, 2) for x in new_t], "all_existing_ms": [round(x, 2) for x in old_t]})
    line["chains"] = chains
    line["findings_equal"] = equal
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if equal and all(r["output_correct"] for r in rates) else 1


if __name__ == "__main__":
    sys.exit(main())
