"""The no-speech kernel alone (spt_debug_no_speech, csrc/capi_sample.cpp): softmax(raw logits)[nosp] of
each row on a numpy array, without an engine or a model.  Test infrastructure:
tests/test_gpu_nospeech_kernel.py compares it with tests/nospeech_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import TranscriptionError


def no_speech(logits, nosp: int, n_vocab=None, *, B=None, ldl=None, device: int = 0) -> np.ndarray:
    """logits [B][ldl] f32 (only columns < n_vocab are read; n_vocab defaults to ldl) -> prob [B] f32.
    B / ldl override the array's shape (argument checks); logits may be None for the same purpose."""
    lib = L.load()
    lg = None if logits is None else np.ascontiguousarray(logits, np.float32)
    rows, cols = (1, 1) if lg is None else lg.shape
    B = rows if B is None else B
    ldl = cols if ldl is None else ldl
    V = ldl if n_vocab is None else n_vocab
    prob = np.full(max(B, 1), np.nan, np.float32)
    err = C.create_string_buffer(512)
    fp = C.POINTER(C.c_float)
    st = lib.spt_debug_no_speech(device, None if lg is None else lg.ctypes.data_as(fp), B, V, ldl, int(nosp),
                                 prob.ctypes.data_as(fp), err, 512)
    if st != L.SPT_OK:
        raise TranscriptionError(st, err.value.decode())
    return prob
