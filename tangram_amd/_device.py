"""The host layer's device plumbing, stated once: which devices are accepted, the stream and the current device of a C-ABI call,
the row pitch of a tensor, and the query-then-allocate sequence of a workspace.  Every module that calls libtangram_hip.so outside
a `tg_mapper` handle goes through `call`; a handle is bound to its creation stream and hands over in `HipMapperEngine._call`."""
from __future__ import annotations

import ctypes as ct
from contextlib import nullcontext

import torch

from . import _capi


def check_device(device):
    """`device` as a torch.device with its index filled in; anything but a HIP device is refused (the emulated build of the CPU
    test-suite runs on "cpu")."""
    device = torch.device(device)
    if device.type != "cuda" and not _capi.is_emulated():
        raise RuntimeError(f"tangram_amd runs on a HIP device only (got device={device!r}); there is no CPU path")
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def stream(device):
    """The caller's current HIP stream on `device` as the C ABI takes it (None: the emulator has no streams)."""
    return ct.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == "cuda" else None


def current(device):
    """Context with `device` as the current HIP device (HIP rejects a stream that does not belong to it); nothing on the emulator."""
    return torch.cuda.device(device) if device.type == "cuda" else nullcontext()


def call(device, fn, *args):
    with current(device):
        return _capi.check(fn(*args))


def pitch(t):
    """Row stride of a 2-D tensor in elements; a one-row tensor (whose stride is arbitrary) counts as at least its width."""
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def workspace(query_fn, *shape_args, device, min_bytes=0):
    """uint8 tensor on `device` of the size `query_fn(*shape_args, &nbytes)` asks for, at least `min_bytes`."""
    nbytes = ct.c_size_t()
    _capi.check(query_fn(*shape_args, ct.byref(nbytes)))
    return torch.empty(max(int(nbytes.value), min_bytes), dtype=torch.uint8, device=device)
