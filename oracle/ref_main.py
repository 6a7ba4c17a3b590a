"""Recipe of oracle/_ref/main.cpp: the reference's own Cython module (corintho_ai/python/main.pyx), with nothing
changed but the path of its `cdef extern from "../cpp/src/trainer.cpp"` (main.pyx:17), which becomes
"trainer.cpp" -- resolved against corintho_ai_amd/cpp/ when tests/test_boundary_cxx.py compiles the result with
this repository's Trainer.  oracle/_ref/ is a build product and stays out of git.

The reference checkout is $CORINTHO_REFERENCE, else a directory named `reference` beside this repository or beside
one of its parent directories.  Without one (or without Cython) nothing is built and an existing main.cpp is kept.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_ref", "main.cpp")
PYX = os.path.join("corintho_ai", "python", "main.pyx")


def find_reference():
    cands = [os.environ["CORINTHO_REFERENCE"]] if os.environ.get("CORINTHO_REFERENCE") else []
    d = ROOT
    while os.path.dirname(d) != d:
        d = os.path.dirname(d)
        cands.append(os.path.join(d, "reference"))
    for c in cands:
        if os.path.isfile(os.path.join(c, PYX)):
            return c
    return None


def build():
    """-> path of oracle/_ref/main.cpp, or None when it could not be made here"""
    ref = find_reference()
    if ref is None:
        print("oracle/_ref/main.cpp: no reference checkout found, not built", flush=True)
        return OUT if os.path.exists(OUT) else None
    try:
        import Cython  # noqa: F401
    except ImportError:
        print("oracle/_ref/main.cpp: Cython not installed, not built", flush=True)
        return OUT if os.path.exists(OUT) else None
    pyx = os.path.join(ref, PYX)
    if os.path.exists(OUT) and os.path.getmtime(OUT) >= os.path.getmtime(pyx):
        return OUT
    with open(pyx) as f:
        patched, n = re.subn(r'cdef extern from "\.\./cpp/src/trainer\.cpp"', 'cdef extern from "trainer.cpp"', f.read())
    if n != 1:
        raise RuntimeError("%s: the extern declaration of trainer.cpp was not found once (%d)" % (pyx, n))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "main.pyx"), "w") as f:
            f.write(patched)
        subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", "main.pyx"], cwd=tmp)
        shutil.move(os.path.join(tmp, "main.cpp"), OUT)
    return OUT


if __name__ == "__main__":
    print(build())
