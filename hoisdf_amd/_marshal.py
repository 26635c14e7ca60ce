"""What every binding module does before its C call: tensors -> pointers, the current stream, size queries, the small host-side
objects (queued counts, prepared blobs) the entries of include/hoisdf.h share.  Imports _lib and torch only - never ops: the family
modules (ops_eval, ops_mesh, ops_infer) sit on this one, and ops on them."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import lib


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _status_error(msg: str):
    return _lib.HoisdfError(-1, msg)


def _size(query: str, *args, error=ValueError) -> int:
    """what the size query ``query`` answers for ``args``; below zero the library refused them: ``error(its message)`` is raised"""
    n = getattr(lib(), query)(*args)
    if n < 0:
        raise error(lib().hoisdf_last_error().decode())
    return n


def _workspace(query: str, *dims_dev, least: int = 1):
    """_workspace("hoisdf_xxx_workspace_bytes", *dims, dev) -> (uint8 scratch tensor of at least `least` bytes, the size to pass on)"""
    *dims, dev = dims_dev
    n = _size(query, *dims, error=_status_error)
    return torch.empty(max(n, least), device=dev, dtype=torch.uint8), n


def _chk(*ts):
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda or t.dtype not in (torch.float32,):
            raise RuntimeError("hoisdf_amd ops need float32 CUDA/HIP tensors (no CPU fallback)")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:       # the C ABI launches on the calling thread's current device and stream
            raise RuntimeError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: one process per "
                               "GPU, call torch.cuda.set_device(local_rank) first")


def _rows(x: torch.Tensor) -> torch.Tensor:
    """view as (M, K) with unit inner stride and a uniform row stride"""
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
        x2 = x2.contiguous()
    return x2


def _counts(n, B: int, dev, what: str):
    """per-sample counts -> int32 (B,) on the device (None stays None)"""
    if n is None:
        return None
    n = torch.as_tensor(n).to(dev, torch.int32).contiguous()
    if n.shape != (B,):
        raise ValueError(f"{what} {tuple(n.shape)}: one count per sample ({B},)")
    return n


_PINNED_I32 = {}        # n -> free page-locked int32 buffers for the survivor counts (hipHostMalloc per call would cost more than the read)


class _QueuedCounts:
    """``n`` int32 words a kernel leaves on the device and copies into page-locked host memory: the device counts, a recycled host
    buffer and the event behind the copy.  ``launch(counts, host pointer)`` queues that kernel on the current stream; ``wait()``
    blocks the HOST until the copy has executed - the device never drains."""

    def __init__(self, n: int, device, launch):
        self.counts = torch.empty(n, device=device, dtype=torch.int32)
        free = _PINNED_I32.setdefault(n, [])
        self.host = free.pop() if free else torch.empty(n, dtype=torch.int32, pin_memory=True)
        launch(self.counts, C.c_void_p(self.host.data_ptr()))
        self.event = torch.cuda.Event()
        self.event.record()
        self._list = None

    def wait(self):
        if self._list is None:
            self.event.synchronize()
            self._list = self.host.tolist()
            _PINNED_I32[self.host.numel()].append(self.host)        # the values are copied out: the buffer can serve the next request
        return self._list


def _check_survivors(counts, num_points: int, what: str = "sdf_infer") -> None:
    """every sample must have num_points lattice survivors to select from; ``counts``: the host list of one field"""
    short = [b for b in range(len(counts)) if counts[b] < num_points]
    if short:
        raise ValueError(f"{what}: sample {short[0]} has only {counts[short[0]]} lattice points inside its bbox, fewer "
                         f"than num_points={num_points} (the reference fails at main/model.py:348)")


class _PreparedBlob:
    """``nbytes`` of device memory that ``build(blob)`` fills on the current stream for one (descriptor, weights) pair, the stream it
    was built on and the event behind the build.  ``version`` counts the builds of the owning model (tests pin that a second frame
    does not prepare again)."""

    def __init__(self, desc, version: int, nbytes: int, device, build):
        self.desc, self.version = desc, version
        self.blob = torch.empty(nbytes, device=device, dtype=torch.uint8)
        build(self.blob)
        self.stream = torch.cuda.current_stream(device)
        self.event = torch.cuda.Event()
        self.event.record(self.stream)


def _after_prepared(prepared: _PreparedBlob, device) -> None:
    """order the current stream behind the build of ``prepared`` (nothing to do on the stream that built it)"""
    cur = torch.cuda.current_stream(device)
    if prepared.stream != cur:
        cur.wait_event(prepared.event)
