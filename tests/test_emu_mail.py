"""PhzMail (phaser_amd/csrc/phz_internal.h: the gathered read-back of a stage's small values) as a unit, in the emulated build: it holds 16 values, and queueing a
17th must fail the send with PHZ_E_ARG -- add() returns -1 then, and a caller that went on would read its value through offset [-1]."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import REPO
from helpers import EmuContext, emu_library
from phaser_amd import _lib


def mail_unit():
    """tests/hipemu/mail_unit.cpp compiled against the emulation and linked to the emulation library (built on first use, like the library itself)"""
    here = os.path.join(REPO, "tests", "hipemu")
    lib = emu_library()
    src = os.path.join(here, "mail_unit.cpp"); out = os.path.join(here, "_build", "mail_unit.so")
    emu = lib._name
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(emu)):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(here, "include"), "-I" + os.path.join(REPO, "include"),
                               "-I" + os.path.join(REPO, "phaser_amd", "csrc"), "-x", "c++", src, "-x", "none", emu, "-Wl,-rpath," + os.path.dirname(emu), "-o", tmp])
        os.replace(tmp, out)
    unit = C.CDLL(out)
    unit.mail_unit_queue.restype = C.c_int
    unit.mail_unit_queue.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib, unit


def test_mail_refuses_a_seventeenth_value():
    lib, unit = mail_unit()
    ctx = EmuContext(lib)
    back = np.zeros(32, np.uint32)
    for n in (1, 16):          # up to its capacity every value arrives
        back[:] = 0
        assert unit.mail_unit_queue(ctx.h, n, C.c_void_p(back.ctypes.data)) == _lib.PHZ_OK
        assert np.array_equal(back[:n], 1000 + np.arange(n)) and not back[n:].any()
    back[:] = 0
    assert unit.mail_unit_queue(ctx.h, 17, C.c_void_p(back.ctypes.data)) == _lib.PHZ_E_ARG
    assert not back.any() and b"PhzMail" in lib.phz_last_error(ctx.h)
    assert unit.mail_unit_queue(ctx.h, 3, C.c_void_p(back.ctypes.data)) == _lib.PHZ_OK          # the ctx stays usable
