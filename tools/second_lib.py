"""A second libocrk.so in the same process, for three-way A/B runs (`--parent PATH` of
bench_pp.py, bench_tn.py and bench_wgrad.py): the library of another commit is loaded beside the
tree's own, and inside `use(handle)` every wrapper of cnn_lstm_ctc_ocr_amd.kernels and every
options.set / override goes to it. Each library keeps its own option registry; both bind the HIP
runtime torch loaded, so tensors and streams are shared.
"""
import contextlib
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnn_lstm_ctc_ocr_amd import _lib  # noqa: E402


def load(path):
    _lib.lib()                                            # the tree's own library first
    handle = ctypes.CDLL(os.path.abspath(path))           # RTLD_LOCAL: no symbol of one binds in the other
    for name, argtypes in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.argtypes = argtypes
        fn.restype = _lib._RESTYPE.get(name, ctypes.c_int)
    return handle


@contextlib.contextmanager
def use(handle):
    """Route _lib.call to `handle` (None: the tree's own library)."""
    if handle is None:
        yield
        return
    prev, _lib._lib = _lib._lib, handle
    try:
        yield
    finally:
        _lib._lib = prev


def parent_from_argv():
    """(handle or None) for `--parent PATH`."""
    if "--parent" not in sys.argv:
        return None
    return load(sys.argv[sys.argv.index("--parent") + 1])


def variants(parent):
    """(name, library handle, GEMM_W4 mode) in the order they are interleaved."""
    v = [("old", None, 0)]
    if parent is not None:
        v.append(("parent", parent, 2))
    v.append(("w4", None, 2))
    return v
