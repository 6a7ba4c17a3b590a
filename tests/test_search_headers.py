"""The search kernel's headers (csrc/mcts.h and the csrc/search_*.h layers it includes) each include what they use: a
translation unit that holds nothing but `#include "<header>"` compiles in the emulation dialect.  A header that leans on
what mcts.h happened to include in front of it fails here."""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corintho_ai_amd", "csrc")


def _compile_alone(header):
    r = subprocess.run(["g++", "-std=c++17", "-DCO_EMU", "-fsyntax-only", "-I", CSRC, "-x", "c++", "-"],
                       input='#include "%s"\n' % header, capture_output=True, text=True)
    return header, r.returncode, r.stderr


def test_every_search_header_compiles_on_its_own():
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "search_*.h"))) + ["mcts.h"]
    assert len(headers) == 10, headers  # the nine layers and their entry
    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(_compile_alone, headers))
    failed = ["%s:\n%s" % (h, err[-1500:]) for h, rc, err in results if rc != 0]
    assert not failed, "not self-contained:\n" + "\n".join(failed)
