"""The host build of the CPU tests: tests/<name>_host.cpp wraps a kernel header of solo_amd/csrc, compiled with SOLO_HOST_EMU (the 1-lane
forms of solo_wave.h) into a shared library that a test loads with ctypes.  The flags are those of tests/emu/Makefile plus -Wno-unknown-pragmas;
this is the one place that states them.  A library is built once per process, by whoever asks first, into a directory that goes when the
process ends; every module declares the argtypes of the functions it calls itself."""
import ctypes
import os
import subprocess
import tempfile

TESTS = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
         "-DSOLO_HOST_EMU"]
_libs = {}
_dir = None


def source(name):
    return os.path.join(TESTS, name + "_host.cpp")


def host_lib(name):
    """the ctypes.CDLL of tests/<name>_host.cpp, compiled with $CXX (default g++)"""
    global _dir
    if name not in _libs:
        if _dir is None:
            _dir = tempfile.TemporaryDirectory(prefix="solo_host_")
        out = os.path.join(_dir.name, "lib%s_host.so" % name)
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [source(name), "-o", out])
        _libs[name] = ctypes.CDLL(out)
    return _libs[name]
