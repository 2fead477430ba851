#!/usr/bin/env python
"""Zstd layers decoded on the GPU: rates of tsg_inflate_zstd_device and the
chain behind it beside the route a caller has without it (tooling; not a
bench.py leg).

  python tools/zstd_probe.py [--mb 8] [--steps 2] [--levels 3,19] [--streams 1,16,256,1024]
                             [--layers 1,4,16,64] [--blobs DIR] [--out profiles/zstd_probe_X.json]

tools/inflate_probe.py's layer (workload/synth.py's image files as one PAX
tar) is compressed by the system libzstd at every level of --levels, with the
checksum flag.  --blobs DIR keeps the compressed layers (layer_l<level>.zst)
and reuses them, for a machine without libzstd.  Measured on the same box:
  decode    N equal streams of it in one tsg_inflate_zstd_device call, N from
            --streams: kernel time (device events) of the decode and the hash
            kernel, wall time of the call, MB/s of output per stream and GB/s
            of output over all -- after a warm-up call at every N
  libzstd   ZSTD_decompress of the same blob on one thread
  chains    for N layers from --layers (the first level's blob), wall time to
            findings of
              new       ScanLayersCompressedDevice: upload of the compressed
                        bytes -> decode -> PrepareLayerTarDevice -> ScanBatchDevice
              existing  per layer ZSTD_decompress on the host -> upload of the
                        tar -> PrepareLayerTarDevice -> ScanBatchDevice
            with the bytes each sends over the link, and whether the findings
            are equal (exit 1 if not).
It prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from trivy_amd import _lib  # noqa: E402
from trivy_amd import secret as S  # noqa: E402
from workload import synth  # noqa: E402
from tar_device_probe import layer_tar  # noqa: E402
import gen_zstd_corpus as GZ  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=8.0)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--levels", default="3,19")
    ap.add_argument("--streams", default="1,16,256,1024")
    ap.add_argument("--layers", default="1,4,16,64")
    ap.add_argument("--seed", type=int, default=0x71215EC7)
    ap.add_argument("--blobs", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = _lib.lib()
    try:
        z = GZ.libzstd()
    except OSError:
        z = None
    corpus = synth.generate(int(a.mb * 1e6), seed=a.seed, sizes="small", layout="image")
    tar = layer_tar(corpus).tobytes()
    n = len(tar)
    sc = S.Scanner(None)
    eng = sc.engine()
    line = {"probe": "zstd", "tar_bytes": n, "files": len(corpus.paths), "steps": a.steps, "libzstd": z is not None}
    levels = [int(x) for x in a.levels.split(",")]
    blobs = {}
    for lv in levels:
        path = os.path.join(a.blobs, "layer_l%d.zst" % lv) if a.blobs else ""
        if path and os.path.exists(path):
            blobs[lv] = open(path, "rb").read()
        else:
            blobs[lv] = GZ.compress(z, tar, level=lv, checksum=1)
            if path:
                os.makedirs(a.blobs, exist_ok=True)
                with open(path, "wb") as f:
                    f.write(blobs[lv])
    cap = (n + 64 + 15) & ~15
    ok = True
    per_level = []
    for lv in levels:
        blob = blobs[lv]
        zl = len(blob)
        bound, exact, clean = S.Scanner.ZstdSizeBound(blob)
        entry = {"level": lv, "zstd_bytes": zl, "ratio": round(n / zl, 3), "size_bound": bound, "bound_exact": exact and clean}
        if z is not None:
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                assert len(GZ.decompress(z, blob, n)) == n
                t.append(time.perf_counter() - t0)
            entry["libzstd_one_thread_mbps"] = round(n / 1e6 / min(t), 1)
        d_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to("cuda:0")
        rates = []
        for ns in [int(x) for x in a.streams.split(",")]:
            d_z = torch.cat([d_blob.repeat(ns), torch.zeros(16, dtype=torch.uint8, device="cuda:0")])
            dst = torch.empty(ns * cap + 16, dtype=torch.uint8, device="cuda:0")
            zo = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(zl))
            do = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(cap))
            out_lens, status = np.zeros(ns, np.uint64), np.zeros(ns, np.int32)
            torch.cuda.synchronize()
            runs = []
            for k in range(a.steps + 1):         # the first call warms up
                ms = ctypes.c_double()
                t0 = time.perf_counter()
                _lib.check(L.tsg_inflate_zstd_device(eng, ctypes.c_void_p(d_z.data_ptr()), zo.ctypes.data, ns,
                                                     ctypes.c_void_p(dst.data_ptr()), do.ctypes.data, out_lens.ctypes.data,
                                                     status.ctypes.data, ctypes.byref(ms)))
                wall = (time.perf_counter() - t0) * 1e3
                dms, hms = ctypes.c_double(), ctypes.c_double()
                frames, blocks = ctypes.c_uint64(), ctypes.c_uint64()
                L.tsg_test_zstd_last_stats(ctypes.byref(dms), ctypes.byref(hms), ctypes.byref(frames), ctypes.byref(blocks))
                if k:
                    runs.append((wall, dms.value, hms.value))
            assert (out_lens == n).all()
            first = dst[:n].cpu().numpy().tobytes() == tar and dst[(ns - 1) * cap:(ns - 1) * cap + n].cpu().numpy().tobytes() == tar
            ok = ok and first
            best = min(runs)
            rates.append({"streams": ns, "output_correct": bool(first), "wall_ms": round(best[0], 3),
                          "decode_kernel_ms": round(best[1], 3), "hash_kernel_ms": round(best[2], 3),
                          "blocks_per_stream": blocks.value // ns,
                          "per_stream_mbps": round(n / 1e6 / (best[1] / 1e3), 2),
                          "aggregate_gbps_kernel": round(ns * n / 1e9 / (best[1] / 1e3), 3),
                          "aggregate_gbps_wall": round(ns * n / 1e9 / (best[0] / 1e3), 3),
                          "all_wall_ms": [round(r[0], 3) for r in runs]})
            del d_z, dst
        entry["decode"] = rates
        per_level.append(entry)
    line["levels"] = per_level

    chains, equal = [], True
    blob = blobs[levels[0]]
    h_tar = torch.empty(n + 16, dtype=torch.uint8).pin_memory()
    for nl in [int(x) for x in a.layers.split(",")]:
        many = [blob] * nl
        new_t, old_t, new_f, old_f = [], [], None, None
        for k in range(a.steps + 1):
            t0 = time.perf_counter()
            layers = sc.ScanLayersCompressedDevice(many)
            t1 = time.perf_counter()
            old = []
            if z is not None:
                for b in many:
                    raw = GZ.decompress(z, b, n)
                    h_tar.numpy()[:n] = np.frombuffer(raw, np.uint8)
                    d_tar = h_tar.to("cuda:0", non_blocking=True)
                    p_dst, offs, paths, binf, _walk, _ms = sc.PrepareLayerTarDevice(d_tar, n)
                    old.append(sc.ScanBatchDevice(p_dst, offs, paths, binf))
            t2 = time.perf_counter()
            if k:
                new_t.append((t1 - t0) * 1e3)
                old_t.append((t2 - t1) * 1e3)
            new_f, old_f = [l[2] for l in layers], old
        if z is not None:
            equal = equal and new_f == old_f
        chains.append({"layers": nl, "level": levels[0], "new_ms": round(min(new_t), 2),
                       "existing_ms": round(min(old_t), 2) if z is not None else None,
                       "new_link_bytes_up": nl * len(blob), "existing_link_bytes_up": nl * n,
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
    return 0 if equal and ok else 1


if __name__ == "__main__":
    sys.exit(main())
