"""The decisions of vrc_render that depend on options and facts alone (libre_amd/csrc/vrc_plan.h), no GPU needed.

vrc_plan_mode (which frame a pass renders, and the refusals of the extension modes and of options changed inside a frame)
and vrc_plan_form (which kernel form marches it, the packed wish, vrc_plan_use_lds) replaced two blocks of vrc_render.
tests/cpu_harness/render_plan_harness.cpp keeps a verbatim copy of those blocks; over the full product of the inputs that
either reads -- and, for the mode, a million seeded draws over the unrestricted latch space -- old and new must return
the same code and the same message, call pool_enable_packed in the same cases and, where the pass is served, derive the
same flags.  Which refusal wins when several apply is thereby the old text's order.  Every message literal of the copied
text must be returned at least once: their number is counted in the copy, not taken from the new code.  Run plain, and as
a stand-alone program under the address and undefined-behaviour sanitizers on a tenth of the cases."""
import ctypes as C
import os
import re
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "render_plan_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "librender_plan_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "render_plan_san")
DEPS = [SRC, os.path.join(orc.ROOT, "libre_amd", "csrc", "vrc_plan.h"), os.path.join(orc.ROOT, "include", "vrc_hip.h")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]

CASES, REFUSED, BAD, ENABLE_CALLS, MESSAGES = range(5)
MODE_PRODUCT = 5 * 3 * 3 * 3 * 2 ** 10  # kernel, projection, fold, element bytes, ten two-valued inputs
FORM_PRODUCT = 5 * 5 * 3 * 2 ** 16      # kernel, mode kind, element bytes, sixteen two-valued inputs
LATCH_STATES = 12                       # all unset, all equal to the options, each of the ten alone differing
RANDOM = 10 ** 6


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _literals(block):
    """The message literals of a copied block: every message starts "vrc_render: ", its continuation lines do not."""
    text = open(SRC).read()
    body = text.split("/* BEGIN %s BLOCK */" % block)[1].split("/* END %s BLOCK */" % block)[0]
    return len(re.findall(r'"vrc_render: ', body))


def test_the_copied_text_has_the_literals_the_issue_counted():
    assert (_literals("MODE"), _literals("FORM")) == (29, 9)


def test_mode_and_form_decide_what_the_text_they_replaced_decided():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.render_plan_mode_run.restype = C.c_uint64
    H.render_plan_mode_run.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    H.render_plan_form_run.restype = C.c_uint64
    H.render_plan_form_run.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    mode = (C.c_uint64 * 5)()
    bad = H.render_plan_mode_run(2024, RANDOM, 1, mode)
    assert bad == 0 and mode[BAD] == 0, list(mode)
    assert mode[CASES] == MODE_PRODUCT * LATCH_STATES + RANDOM
    assert 0 < mode[REFUSED] < mode[CASES]  # passes served and passes refused
    assert mode[MESSAGES] == _literals("MODE"), list(mode)  # every refusal of the copied text was reached
    form = (C.c_uint64 * 5)()
    bad = H.render_plan_form_run(1, form)
    assert bad == 0 and form[BAD] == 0, list(form)
    assert form[CASES] == FORM_PRODUCT
    assert 0 < form[REFUSED] < form[CASES]
    assert form[ENABLE_CALLS] > 0  # the packed atlas was asked for, required and wanted
    assert form[MESSAGES] == _literals("FORM"), list(form)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DRENDER_PLAN_MAIN"])
    r = subprocess.run([exe, "10"], capture_output=True, text=True, timeout=300)  # every tenth case
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    rows = {ln.split()[0]: [int(v) for v in ln.split()[2::2]] for ln in r.stdout.splitlines()}
    assert rows["mode"][CASES] == -(-MODE_PRODUCT * LATCH_STATES // 10) + RANDOM // 10 and rows["mode"][BAD] == 0
    assert rows["form"][CASES] == -(-FORM_PRODUCT // 10) and rows["form"][BAD] == 0
    assert rows["mode"][REFUSED] > 0 and rows["form"][REFUSED] > 0 and rows["form"][ENABLE_CALLS] > 0
