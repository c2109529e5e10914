"""Test helper: a stand-alone C program of tests/c (with its own main) and the library sources it
calls, compiled under AddressSanitizer + UndefinedBehaviorSanitizer, linked with g++ and run -- once
per session and program.  Nothing is preloaded: the sanitizers' runtimes are linked into the program."""
import os
import shutil
import subprocess

from conftest import PKG, REPO

HAVE_CC = shutil.which("gcc") is not None and shutil.which("g++") is not None
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
       "-g", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(REPO, "include")]
_HOST = os.path.join(PKG, "host")
# the host layer without a GPU: host/*.c, the stubs of the device entry points, the host plan and the
# host scan writer
HOST_LAYER = sorted(os.path.join(_HOST, f) for f in os.listdir(_HOST) if f.endswith(".c")) + [
    os.path.join(REPO, "tests", "c", "san_nogpu.c"),
    os.path.join(PKG, "csrc", "jpgx_plan.cpp"),
    os.path.join(PKG, "csrc", "jpgx_jfif_write.cpp")]
_results = {}


def run(name, libs=HOST_LAYER, timeout=300):
    """Builds tests/c/<name>.c with the sources `libs` and runs it; (returncode, stdout, stderr)."""
    if name in _results:
        return _results[name]
    bdir = os.path.join(REPO, "tests", "c", "_build", name)
    os.makedirs(bdir, exist_ok=True)
    objs = []
    for src in [os.path.join(REPO, "tests", "c", name + ".c")] + list(libs):
        cc = ["g++", "-std=c++17"] if src.endswith(".cpp") else \
            ["gcc", "-std=c99" if os.path.dirname(src) == _HOST else "-std=c11"]
        obj = os.path.join(bdir, os.path.basename(src) + ".o")
        b = subprocess.run(cc + SAN + ["-c", src, "-o", obj], capture_output=True, text=True, timeout=600)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(obj)
    exe = os.path.join(bdir, name)
    b = subprocess.run(["g++"] + SAN + objs + ["-o", exe, "-lm", "-lpthread"], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=timeout, env=env)
    _results[name] = (r.returncode, r.stdout, r.stderr)
    return _results[name]
