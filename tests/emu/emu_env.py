"""TEST INFRASTRUCTURE ONLY -- build and bind the CPU-emulated build of the product kernels (tests/emu/libwrsn_emu.so); tests/sides.py
(EmuSide) drives it through the same C-ABI binding the product uses, with numpy arrays standing in for device memory."""
import ctypes as C
import os
import subprocess

from multi_agent_rl_wrsn_amd import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        subprocess.check_call(["make", "-s", "-C", _HERE, "libwrsn_emu.so"])
        _EMU = _lib.bind(C.CDLL(os.path.join(_HERE, "libwrsn_emu.so")))
    return _EMU
