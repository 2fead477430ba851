#!/usr/bin/env python
"""Time the device-side content preparation (tsg_prepare_batch_device) on two
device batches, per pass and in total (tooling):

  text   all text at CRLF density (one '\\r' per 40 bytes), next to
         tsg_strip_cr_device on the same batch -- the yardstick: the
         preparation does the same compaction plus the classify pass;
  mixed  70% of the files text, 20% binaries to drop, 10% binary .pyc.

  python tools/prep_probe.py [--gb 4] [--files 2000] [--reps 5]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trivy_amd import secret as S  # noqa: E402

PASSES = ("classify", "count", "scan", "compact")


def batch(n, nfiles, mixed, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    src = torch.randint(32, 127, (n + 64,), dtype=torch.uint8, device="cuda:0", generator=g)
    src[39:n:40] = 13
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n, 997), nfiles - 1, replace=False)).astype(np.int64)
    off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    paths = ["t/%d.c" % k for k in range(nfiles)]
    if mixed:
        kinds = rng.choice(3, nfiles, p=[0.7, 0.2, 0.1])
        for k in np.flatnonzero(kinds):
            a, b = int(off[k]), int(off[k + 1])
            body = torch.randint(0, 256, (b - a,), dtype=torch.uint8, device="cuda:0", generator=g)
            body[torch.rand(b - a, device="cuda:0", generator=g) < 0.5] = ord("p")
            body[0] = 0
            src[a:b] = body
            paths[k] = "b/%d.%s" % (k, "dat" if kinds[k] == 1 else "pyc")
    return src, off, paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=4)
    ap.add_argument("--files", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = int(a.gb * 1e9) // 16 * 16
    sc = S.Scanner(None)
    for name, mixed in (("text", False), ("mixed", True)):
        src, off, paths = batch(n, a.files, mixed, 1 if not mixed else 2)
        if not mixed:
            d_off = torch.from_numpy(off).to("cuda:0")
            ms = []
            for _ in range(a.reps + 1):
                dst, noff, stripped, kms = sc.StripCR(src, d_off, a.files, n)
                ms.append(kms)
                del dst, noff
            ms = ms[1:]
            print("%s %.2f GB %d files: tsg_strip_cr_device %s ms -> mean %.3f ms, spread (max - min) %.3f ms, "
                  "%.0f GB/s N+N'" % (name, n / 1e9, a.files, " ".join("%.3f" % x for x in ms), np.mean(ms),
                                      max(ms) - min(ms), (n + stripped) / np.mean(ms) / 1e6), flush=True)
        tot, per = [], []
        for _ in range(a.reps + 1):
            dst, offs, _sp, idx, binf, kms, passes = sc.PrepareBatchDevice(src, off, paths, with_passes=True)
            tot.append(kms)
            per.append(passes)
            prepared = int(offs[-1])
            del dst
        tot, per = tot[1:], np.array(per[1:])
        print("%s %.2f GB %d files (%d kept, %d binary .pyc): tsg_prepare_batch_device %s ms -> mean %.3f ms, "
              "%.0f GB/s N+N' (N' = %.2f GB)" % (name, n / 1e9, a.files, len(idx), sum(binf),
                                                 " ".join("%.3f" % x for x in tot), np.mean(tot),
                                                 (n + prepared) / np.mean(tot) / 1e6, prepared / 1e9), flush=True)
        print("  per pass (mean ms): " + ", ".join("%s %.3f" % (p, m) for p, m in zip(PASSES, per.mean(axis=0))),
              flush=True)
        del src


if __name__ == "__main__":
    main()
