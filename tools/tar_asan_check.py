"""Host-code sanitizer run (ASan + UBSan) of the device tar walk's CPU side.

Builds tools/tar_asan.cpp -- a stand-alone program -- against the host sources
of libtrivysecret compiled with g++ -fsanitize=address,undefined (no recovery),
linked with the unsanitized HIP objects of trivy_amd/_build (no kernel runs),
writes every tar of tests/_tar_corpus.py with each option set to files and runs
the program over them: plan_tar_marks, SparseTarInput, walk_layer and the model
of tsg_prepare_layer_tar_device on exact-size heap copies, compared with
tsg_prepare_layer_tar_opts.

  python tools/tar_asan_check.py [--out profiles/tar_asan.log]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tar_corpus as TC  # noqa: E402
from trivy_amd import build as B  # noqa: E402

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
    exe = os.path.join(outdir, "tar_asan")
    hip_objs = [os.path.join(B.OBJ, s + ".o") for s in B.HIP_SRCS]
    subprocess.check_call(["g++", "-o", exe, os.path.join(ROOT, "tools", "tar_asan.cpp")] + objs + hip_objs +
                          common + ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return exe


def write_cases(d):
    names = []
    os.makedirs(d)
    for name, t in TC.corpus().items():
        for k, opts in enumerate(TC.OPTIONS):
            cd = os.path.join(d, "%s.%d" % (name, k))
            os.makedirs(cd)
            with open(os.path.join(cd, "tar.bin"), "wb") as f:
                f.write(t.data)
            with open(os.path.join(cd, "opts.txt"), "w") as f:
                f.write(opts.get("config_path", "") + "\n")
                f.write("".join("F %s\n" % x for x in opts.get("skip_files", ())))
                f.write("".join("D %s\n" % x for x in opts.get("skip_dirs", ())))
                f.write("".join("P %s\n" % x for x in opts.get("file_patterns", ())))
            names.append("%s.%d" % (name, k))
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
    text = "sanitizers: %s\ntar rc=%d %s%s" % (" ".join(SAN), p.returncode, p.stdout, p.stderr[-4000:])
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
