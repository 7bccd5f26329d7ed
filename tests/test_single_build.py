"""The kernel sources compile exactly one library: no conditional compilation, no build options, no
environment lookups in node2vec_amd/csrc.  (Variants are measured on a branch and recorded in DESIGN.md.)"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "node2vec_amd", "csrc")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def _lines(path):
    with open(path) as f:
        return [(f"{os.path.basename(path)}:{i}", line) for i, line in enumerate(f, 1)]


def test_no_conditional_compilation():
    assert SOURCES
    directive = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b")
    assert [where for p in SOURCES for where, line in _lines(p) if directive.match(line)] == []


def test_no_build_options_in_the_makefile():
    option = re.compile(r"^\s*(ifdef|ifndef|ifeq|ifneq)\b")
    assert [where for where, line in _lines(os.path.join(CSRC, "Makefile")) if option.match(line)] == []


def test_no_environment_lookups():
    assert [where for p in SOURCES for where, line in _lines(p) if "getenv" in line] == []


def test_dead_forms_of_the_wedge_step_are_gone():
    gone = re.compile(r"\b(kJumpOnly|wedge_step_wide|jump_listed|lds_list)\b")
    assert [where for p in SOURCES for where, line in _lines(p) if gone.search(line)] == []


def test_workspace_pass_variant_is_gone():
    assert not os.path.exists(os.path.join(CSRC, "n2v_walk_wedge2.hip"))
