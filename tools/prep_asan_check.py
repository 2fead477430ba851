"""Host-code sanitizer run (ASan + UBSan) of the device preparation's CPU side.

Builds tools/prep_asan.cpp -- a stand-alone program -- against the host
sources of libtrivysecret compiled with g++ -fsanitize=address,undefined (no
recovery), linked with the unsanitized HIP objects of trivy_amd/_build (no
kernel runs), writes the corpora of tests/_prep_corpus.py to files and runs
the program over them: plan_prep (the device pass's CPU model) and
prepare_core (the host feed) on exact-size heap copies, compared.

  python tools/prep_asan_check.py [--out profiles/prep_asan.log]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _prep_corpus as PC  # noqa: E402
from trivy_amd import build as B  # noqa: E402
from trivy_amd import secret as S  # noqa: E402

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def build_driver(outdir):
    B.build()                                        # HIP objects in trivy_amd/_build
    common = ["-std=c++17", "-fPIC", "-I", B.CSRC, "-I", os.path.join(ROOT, "include")] + SAN
    jobs, objs = [], []
    for s in B.HOST_SRCS:
        o = os.path.join(outdir, s + ".asan.o")
        jobs.append(subprocess.Popen(["g++", "-c", os.path.join(B.CSRC, s), "-o", o, "-march=x86-64-v2"] + common))
        objs.append(o)
    for j in jobs:
        if j.wait() != 0:
            raise SystemExit("sanitizer compile failed")
    exe = os.path.join(outdir, "prep_asan")
    hip_objs = [os.path.join(B.OBJ, s + ".o") for s in B.HIP_SRCS]
    subprocess.check_call(["g++", "-o", exe, os.path.join(ROOT, "tools", "prep_asan.cpp")] + objs + hip_objs +
                          common + ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return exe


def write_cases(d):
    names = []
    for name, c in PC.corpora().items():
        cd = os.path.join(d, name)
        os.makedirs(cd)
        with open(os.path.join(cd, "config.json"), "w") as f:
            f.write(json.dumps(S.ParseConfig(c.config_path)) if c.config_path else "")
        np.frombuffer(b"".join(b for _, b in c.raw_files), np.uint8).tofile(os.path.join(cd, "data.bin"))
        off = np.zeros(len(c.files) + 1, np.uint64)
        off[1:] = np.cumsum([len(b) for _, b in c.raw_files])
        off.tofile(os.path.join(cd, "offsets.bin"))
        with open(os.path.join(cd, "paths.txt"), "w") as f:
            f.write("".join(p + "\n" for p, _ in c.raw_files))
        with open(os.path.join(cd, "opts.txt"), "w") as f:
            f.write("".join(x + "\n" for x in (os.path.basename(c.config_path),) + c.file_patterns))
        names.append(name)
    with open(os.path.join(d, "index.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        write_cases(os.path.join(td, "cases"))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe, os.path.join(td, "cases")], capture_output=True, text=True, env=env)
    text = "sanitizers: %s\nprep rc=%d %s%s" % (" ".join(SAN), p.returncode, p.stdout, p.stderr[-4000:])
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
