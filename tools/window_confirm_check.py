#!/usr/bin/env python
"""Sanitizer run (ASan + UBSan) of the windowed confirmation of the device-only
scan, on the CPU.

Builds tools/window_confirm_check.cpp -- a program with its own main -- against
the host sources of libtrivysecret compiled with g++
-fsanitize=address,undefined (no recovery), linked with the unsanitized HIP
objects of trivy_amd/_build (no kernel runs: the program calls the CPU model,
tsg_scan_device_model_opts), dumps every corpus of tests/_window_corpus.py --
at its own chunk and window, and again at other chunks and windows -- with the
findings of the plain table model and the insufficient files each corpus
names, and runs the program over the dump.  The model keeps every gathered run
in an allocation of exactly its bytes and frees the batch before it confirms,
so a read into a hole is a read outside an allocation.

  python tools/window_confirm_check.py [--out profiles/window_confirm_asan.log]
"""
import argparse
import ctypes
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from trivy_amd import _lib  # noqa: E402
from trivy_amd import build as B  # noqa: E402
from trivy_amd import secret as S  # noqa: E402
import _window_corpus as WC  # noqa: E402

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
# beside each corpus's own setting (where its insufficient set is stated): the findings alone under these
OTHERS = [(256, (8, 40, 0)), (512, (700, 700, 0)), (1024, (3, 3, 100000)), (128, (4000, 4000, 0)), (128, (0, 1, 0))]


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
    exe = os.path.join(outdir, "window_confirm_check")
    hip_objs = [os.path.join(B.OBJ, s + ".o") for s in B.HIP_SRCS]
    subprocess.check_call(["g++", "-o", exe, os.path.join(ROOT, "tools", "window_confirm_check.cpp")] + objs + hip_objs +
                          common + ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return exe


def raw_json(sc, args):
    """tsg_result_json of the table model's scan, as the program will compare it."""
    import numpy as np
    L = _lib.lib()
    data, offsets = S.pack(args)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args])
    binary = np.array([1 if a.Binary else 0 for a in args] or [0], dtype=np.uint8)
    res = ctypes.c_void_p()
    _lib.check(L.tsg_scan_device_model(sc._rs, data.ctypes.data, offsets.ctypes.data, len(args), paths, lens,
                                       binary.ctypes.data, 512, ctypes.byref(res)))
    buf, n = ctypes.c_void_p(), ctypes.c_size_t()
    try:
        _lib.check(L.tsg_result_json(res, ctypes.byref(buf), ctypes.byref(n)))
        raw = ctypes.string_at(buf, n.value)
        L.tsg_free(buf)
    finally:
        L.tsg_result_free(res)
    return raw


def s_(b):
    return struct.pack("<Q", len(b)) + b


def dump(path):
    entries = []
    for name in WC.NAMES:
        c = WC.corpus(name)
        sc = S.Scanner(c.cfg)
        want = raw_json(sc, c.args)
        settings = [(c.chunk, c.window, c.insufficient)]
        if name != "large_sparse":
            for chunk, window in OTHERS:
                _, rec, _, _ = S.scan_device_model_windows(sc, c.args, chunk, window)
                settings.append((chunk, window, rec["insufficient"]))
        for chunk, window, short in settings:
            e = s_(name.encode()) + s_(json.dumps(c.cfg).encode() if c.cfg is not None else b"")
            e += struct.pack("<IIIQI", chunk, window[0], window[1], window[2], len(c.args))
            for a in c.args:
                e += s_(a.FilePath.encode()) + struct.pack("<B", 1 if a.Binary else 0) + s_(a.Content)
            e += struct.pack("<I", len(short)) + b"".join(struct.pack("<I", f) for f in short) + s_(want)
            entries.append(e)
    with open(path, "wb") as f:
        f.write(b"WCC1" + struct.pack("<I", len(entries)) + b"".join(entries))
    return len(entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_confirm_asan.log"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        exe = build_program(d)
        n = dump(os.path.join(d, "corpora.bin"))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, os.path.join(d, "corpora.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env,
                           timeout=1200)
    text = ("g++ %s: host sources %s; tools/window_confirm_check.cpp; %d corpus runs\n"
            % (" ".join(SAN), " ".join(B.HOST_SRCS), n)) + p.stdout.decode("utf-8", "replace") + "exit status %d\n" % p.returncode
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
