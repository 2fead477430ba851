"""Host-code sanitizer run (ASan + UBSan) of the zstd decode's CPU side.

Builds tools/zstd_asan.cpp -- a stand-alone program with its own main over the
header-only trivy_amd/csrc/zstdec.h -- with g++ -fsanitize=address,undefined
(no recovery), writes every stream of tests/_zstd_corpus.py to files and runs
the program over them: zstd_model, the decoder the device kernel runs behind
another Io policy, on exact-size heap copies -- the corpus with its statuses,
a slot one byte short, the size bound, and every single-byte corruption and
truncation of the small streams.  CPU only; no kernel runs, nothing is loaded
into python.

  python tools/zstd_asan_check.py [--out profiles/zstd_model_asan.log]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _zstd_corpus as G  # noqa: E402

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "zstd_asan")
        subprocess.check_call(["g++", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "zstd_asan.cpp"),
                               "-I", os.path.join(ROOT, "trivy_amd", "csrc")] + SAN)
        cases = os.path.join(td, "cases")
        os.makedirs(cases)
        with open(os.path.join(cases, "index.txt"), "w") as idx:
            for name, c in G.corpus().items():
                with open(os.path.join(cases, name + ".zst"), "wb") as f:
                    f.write(c.z)
                if c.status == G.OK:
                    with open(os.path.join(cases, name + ".out"), "wb") as f:
                        f.write(c.payload)
                idx.write("%s %d %d\n" % (name, c.status, G.default_cap(c)))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe, cases], capture_output=True, text=True, env=env)
    text = "sanitizers: %s\nzstd rc=%d %s%s" % (" ".join(SAN), p.returncode, p.stdout, p.stderr[-4000:])
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
