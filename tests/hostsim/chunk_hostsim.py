"""ctypes driver of tests/hostsim/chunk_hostsim.cpp (TEST INFRASTRUCTURE: the chunk rules of the product's decoders run on the host)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SRC = os.path.join(_HERE, 'chunk_hostsim.cpp')
_CORE = os.path.join(_ROOT, 'l3c-pytorch_amd', 'csrc', 'ac_core.h')
_SO = os.path.join(_HERE, '_build', 'libchunk_hostsim.so')
_lib = None


def get():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(_SRC), os.path.getmtime(_CORE))
        if not os.path.isfile(_SO) or os.path.getmtime(_SO) < newest:
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-I', os.path.dirname(_CORE), '-o', _SO, _SRC])
        lib = ctypes.CDLL(_SO)
        ll = ctypes.c_longlong
        for name, n in (('hostsim_entry_step', 2), ('hostsim_entry_npix', 3), ('hostsim_entry_final_chunk', 2)):
            getattr(lib, name).restype = ll
            getattr(lib, name).argtypes = [ll] * n
        lib.hostsim_decode_chunks.restype = ll
        lib.hostsim_decode_chunks.argtypes = [ctypes.c_void_p, ll, ctypes.c_int, ctypes.c_void_p, ll, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p]
        _lib = lib
    return _lib


def decode_chunks(tab, data, chunk_len, final_chunk, fill=-7):
    """-> (symbols int16 (sum of chunk_len,), pre-filled with `fill`; records uint32 (n_chunks, 4) after every chunk; symbols written)."""
    tab = np.ascontiguousarray(tab).view(np.uint16)
    buf = np.frombuffer(data, np.uint8)
    lens = np.ascontiguousarray(chunk_len, dtype=np.int64)
    out = np.full(int(lens.sum()), fill, np.int16)
    rec = np.zeros((len(lens), 4), np.uint32)
    n = get().hostsim_decode_chunks(tab.ctypes.data, tab.shape[1], tab.shape[1], buf.ctypes.data if len(buf) else None, len(buf),
                                    lens.ctypes.data, len(lens), int(final_chunk), out.ctypes.data, rec.ctypes.data)
    return out, rec, int(n)
