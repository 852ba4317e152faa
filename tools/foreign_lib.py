"""Load another build of libkws_hip.so for a same-box A/B (tools/benchab.py, tools/maskbench.py): use(path) points kws_amd.lib at it.
An older build lacks the entry points added since; kws_amd.lib binds every one of them, so the missing ones become stubs that refuse to
run -- the workload of an A/B only calls what both builds have."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))


class _Build(ctypes.CDLL):
    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if not name.startswith("kws_"):
                raise

            def missing(*args):
                raise RuntimeError("%s is not in this build of the library (%s)" % (name, self._name))
            setattr(self, name, missing)
            return missing


def use(path):
    import kws_amd.lib as L
    L.LIB_PATH = os.path.abspath(path)
    L.ctypes.CDLL = _Build
