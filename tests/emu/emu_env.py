"""TEST INFRASTRUCTURE ONLY -- build and bind the CPU-emulated build of the product kernels (tests/emu/libwrsn_emu.so); tests/sides.py
(EmuSide) drives it through the same C-ABI binding the product uses, with numpy arrays standing in for device memory."""
import ctypes as C
import os
import subprocess

from multi_agent_rl_wrsn_amd import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = None


def emu_lib():
    """The emulated library, built on demand -- or, as WRSN_HIP_LIB does for the product library, the build that WRSN_EMU_LIB names
    (tools/emu_coverage.py points it at an instrumented one); a named build that is missing is an error, never a rebuild."""
    global _EMU
    if _EMU is None:
        path = os.environ.get("WRSN_EMU_LIB")
        if not path:
            subprocess.check_call(["make", "-s", "-C", _HERE, "libwrsn_emu.so"])
            path = os.path.join(_HERE, "libwrsn_emu.so")
        _EMU = _lib.bind(C.CDLL(path))
    return _EMU
