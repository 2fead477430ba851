#!/usr/bin/env python
"""Sanitizer run (ASan + UBSan) of the line windows' host code, on the CPU.

Builds tools/line_window_check.cpp -- a program with its own main -- against
the host sources of libtrivysecret compiled with g++
-fsanitize=address,undefined (no recovery), linked with the unsanitized HIP
objects of trivy_amd/_build (no kernel runs: the program calls the layout hook
tsg_test_plan_gather_lines and the CPU model tsg_scan_device_model_opts2),
dumps every corpus of tests/_line_window_corpus.py -- at its own chunk, window
and cap, and again at other chunks, windows and caps -- with the table model's
candidates, the findings of the plain model and the insufficient files, and
runs the program over the dump.  The batch lies in an allocation of exactly
its size while the layout walks its lines, every gathered run in one of
exactly its bytes, and the batch is freed before the confirmation.

  python tools/line_window_check.py [--out profiles/line_window_asan.log]
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from trivy_amd import build as B  # noqa: E402
from trivy_amd import secret as S  # noqa: E402
import _line_window_corpus as LC  # noqa: E402
from window_confirm_check import SAN, raw_json, s_  # noqa: E402

# beside each corpus's own setting (where its insufficient set is stated): (chunk, window, cap)
OTHERS = [(256, (8, 40, 0), 777), (512, (700, 700, 0), 4096), (1024, (3, 3, 0), 100000), (128, (64, 64, 0), 1),
          (128, (0, 1, 0), 50)]


def build_program(outdir):
    B.build()                                        # HIP objects in trivy_amd/_build
    common = ["-std=c++17", "-fPIC", "-I", B.CSRC, "-I", os.path.join(ROOT, "include")] + SAN
    objs, jobs = [], []
    for s in B.HOST_SRCS:
        o = os.path.join(outdir, s + ".asan.o")
        jobs.append(subprocess.Popen(["g++", "-c", os.path.join(B.CSRC, s), "-o", o, "-march=x86-64-v2"] + common))
        objs.append(o)
    for j in jobs:
        if j.wait() != 0:
            raise SystemExit("sanitizer compile failed")
    exe = os.path.join(outdir, "line_window_check")
    hip_objs = [os.path.join(B.OBJ, s + ".o") for s in B.HIP_SRCS]
    subprocess.check_call(["g++", "-o", exe, os.path.join(ROOT, "tools", "line_window_check.cpp")] + objs + hip_objs +
                          common + ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return exe


def dump(path):
    entries = []
    for name in LC.NAMES + ["combined", "combined_reversed"]:
        c = LC.corpus(name) if name in LC.NAMES else LC.combined(name.endswith("reversed"))
        sc = S.Scanner(c.cfg)
        want = raw_json(sc, c.args)
        cands, info = S.prefilter_table_model(sc, c.args, with_info=True)
        rows, _ = S.windowable_rows(sc)
        flat = [(f, r, int(s)) for (f, r), v in cands.items() for s in v]
        settings = [(c.chunk, c.window, c.cap)] + (OTHERS if name in LC.NAMES else [])
        for chunk, window, cap in settings:
            _, rec, _, _ = S.scan_device_model_windows(sc, c.args, chunk, window, window_lines=cap)
            short = rec["insufficient"]
            if (chunk, window, cap) == (c.chunk, c.window, c.cap) and name in LC.NAMES:
                assert short == c.insufficient, (name, short)
            e = s_(name.encode()) + s_(json.dumps(c.cfg).encode() if c.cfg is not None else b"")
            e += struct.pack("<IIIIQI", chunk, window[0], window[1], cap, window[2], len(c.args))
            for a in c.args:
                e += s_(a.FilePath.encode()) + struct.pack("<B", 1 if a.Binary else 0) + s_(a.Content)
            e += struct.pack("<I", len(short)) + b"".join(struct.pack("<I", f) for f in short) + s_(want)
            e += struct.pack("<I", len(flat)) + b"".join(struct.pack("<IIQ", f, r, s) for f, r, s in flat)
            e += b"".join(struct.pack("<I", int(x)) for x in info["special"])
            e += struct.pack("<I", len(rows)) + bytes(bytearray(int(x) for x in rows))
            entries.append(e)
    with open(path, "wb") as f:
        f.write(b"LWC1" + struct.pack("<I", len(entries)) + b"".join(entries))
    return len(entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_window_asan.log"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        exe = build_program(d)
        n = dump(os.path.join(d, "corpora.bin"))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, os.path.join(d, "corpora.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env,
                           timeout=1800)
    text = ("g++ %s: host sources %s; tools/line_window_check.cpp; %d corpus runs\n"
            % (" ".join(SAN), " ".join(B.HOST_SRCS), n)) + p.stdout.decode("utf-8", "replace") + "exit status %d\n" % p.returncode
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
