"""The product's kernels under the HIP emulator AND AddressSanitizer: a wrong index that the GPU would turn into a memory
fault (or silently read) is reported on the CPU with file and line.  The sanitizer build goes to a directory outside the
source tree, keyed by the sources it is made of: no sanitizer object ever sits in the tree (nor travels with it)."""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _libasan():
    try:
        p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    except OSError:
        return None
    return p if p and os.path.isabs(p) and os.path.exists(p) else None


def _asan_build_dir():
    h = hashlib.sha256()
    srcs = sorted(glob.glob(os.path.join(ROOT, "youtokentome_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*.h")) +
                  [os.path.join(HERE, "hipsim", f) for f in ("Makefile", "hipsim.cpp", os.path.join("include", "hip", "hip_runtime.h"))])
    for f in srcs:
        if os.path.isfile(f) and f.endswith((".hip", ".cpp", ".h", "Makefile")):
            h.update(os.path.relpath(f, ROOT).encode() + b"\0" + open(f, "rb").read())
    return os.path.join(tempfile.gettempdir(), "yttm_hipsim_asan_" + h.hexdigest()[:16])


@pytest.mark.skipif(_libasan() is None, reason="libasan not available")
def test_kernels_under_address_sanitizer():
    out = _asan_build_dir()
    r = subprocess.run(["make", "-C", os.path.join(HERE, "hipsim"), "-j8", "asan", "OUT=" + out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ)
    env["LD_PRELOAD"] = _libasan()
    env["ASAN_OPTIONS"] = "detect_leaks=0:halt_on_error=1"
    env["YTTM_AMD_LIB"] = os.path.join(out, "libyttm_sim_asan.so")
    r = subprocess.run([sys.executable, os.path.join(HERE, "asan_scenarios.py")], capture_output=True, text=True, env=env, timeout=900)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0 and "ASAN_SCENARIOS_OK" in r.stdout, tail


def test_no_sanitizer_objects_in_the_tree():
    """Objects and libraries built with AddressSanitizer must not sit in the repository tree (they would travel with it to machines where
    they do not belong): no *.o or *.so under it may reference __asan_init."""
    found = []
    for base, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d != ".git"]
        for f in files:
            if f.endswith((".o", ".so")):
                p = os.path.join(base, f)
                with open(p, "rb") as fh:
                    if b"__asan_init" in fh.read():
                        found.append(os.path.relpath(p, ROOT))
    assert not found, found
