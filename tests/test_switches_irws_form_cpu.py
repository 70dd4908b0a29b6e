"""M2S_IR_WS has three values (csrc/switches.hpp): "0" turns the persistent IR front half off, "handoff" keeps it on
in the handed-off form on every shape, anything else (and unset) is on with the per-wave form where it applies.  The
variable is still named once in the table, so tests/test_switches_cpu.py's lists hold unchanged."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mri-to-speech_amd", "csrc")
SRC = r'''
#include <cstdio>
#include "switches.hpp"
int main() {
  int named = 0;
  const m2s::Switches w = m2s::Switches::from_env([&](const char* n) { named += std::strcmp(n, "M2S_IR_WS") == 0; });
  std::printf("%d %d %d\n", (int)w.ir_ws, (int)w.irws_handoff, named);
}
'''


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def form(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host compiler and no hipcc")
    d = tmp_path_factory.mktemp("irws_form")
    src, exe = str(d / "form.cpp"), str(d / "form")
    with open(src, "w") as fh:
        fh.write(SRC)
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], check=True)
    base = {k: v for k, v in os.environ.items() if not k.startswith("M2S_")}

    def run(text):
        env = dict(base) if text is None else dict(base, M2S_IR_WS=text)
        return tuple(int(v) for v in subprocess.run([exe], env=env, check=True, capture_output=True, text=True).stdout.split())

    return run


@pytest.mark.parametrize("text,ir_ws,handoff", [(None, 1, 0), ("1", 1, 0), ("", 1, 0), ("0", 0, 0), ("handoff", 1, 1),
                                                ("Handoff", 1, 0), ("handoff ", 1, 0)])
def test_ir_ws_values(form, text, ir_ws, handoff):
    assert form(text) == (ir_ws, handoff, 1)  # and the variable is named exactly once
