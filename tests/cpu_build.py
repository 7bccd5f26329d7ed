"""The one compile line of the CPU restatements under tests/cpu_*/: no contraction and no fast-math, so every spelled
operation rounds once -- these flags are what makes a restatement a restatement."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-std=c11"]


def build(source, out_dir, defines=()) -> ctypes.CDLL:
    """source (relative to tests/) compiled into out_dir as lib<its name>.so, and loaded; `defines` are macro
    names passed as -D (an instrumented build: give it an out_dir of its own)"""
    out = os.path.join(str(out_dir), "lib" + os.path.splitext(os.path.basename(source))[0] + ".so")
    subprocess.check_call(["cc", *FLAGS, *("-D" + d for d in defines), "-o", out, os.path.join(HERE, source), "-lm"])
    return ctypes.CDLL(out)
