"""Device plumbing shared by meshing, evaluation and bounds (torch side; ``_lib`` stays ctypes-only): the current stream's handle
and the workspace of a library call."""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def stream(device):
    """The raw handle of ``device``'s current stream, as the C ABI takes it."""
    return torch.cuda.current_stream(device).cuda_stream


def aligned(nbytes, device):
    """(tensor, pointer): ``nbytes`` of device memory from the 256-byte aligned pointer on; the tensor keeps them alive."""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


def workspace(lib, size_fn, device, *args):
    """(tensor, pointer, bytes): the workspace ``size_fn(*args, &bytes)`` (a ``vmapstep_*_workspace_bytes``) asks for."""
    nb = ctypes.c_size_t(0)
    _lib.check(size_fn(*args, ctypes.byref(nb)), lib)
    return (*aligned(nb.value, device), nb.value)
