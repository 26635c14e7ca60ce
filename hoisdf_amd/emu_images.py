"""Cache of the slab images the emulated GEMM reads its weights from (csrc/gemm_emu_b3.hip / gemm_emu_h2.hip, hoisdf_linear_emu_prepare): one image per
(weight view, orientation), rebuilt in place when the weight changes, singly at the next use or all at once after an optimizer step.
An image is built on one HIP stream and read on others (the object stack runs on a second one): every entry remembers the event of
its build and the streams that read it since."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, NamedTuple, Optional, Set, Tuple

import torch

from ._lib import EmuPrepItem, call, lib


class ImageKey(NamedTuple):
    """the f32 weight view an image was built from (data_ptr is part of it: an entry keeps its device pointer) and the orientation"""
    device: int
    ptr: int
    rows: int
    cols: int
    ld: int
    transpose: bool

    def end(self) -> int:
        """one past the last byte of the weight view"""
        return self.ptr + 4 * ((self.rows - 1) * self.ld + self.cols)


class _Entry:
    __slots__ = ("image", "version", "built", "build_stream", "owner", "readers")

    def __init__(self, image: torch.Tensor, owner):
        self.image = image
        self.version = None                  # (weight generation, torch version counter) of the build; None: never built / stale
        self.built: Optional[torch.cuda.Event] = None
        self.build_stream = None
        self.owner = owner                   # weakref of the tensor object the entry belongs to
        self.readers: Set[torch.cuda.Stream] = set()


class _BatchTable(NamedTuple):
    epoch: int
    keys: List[ImageKey]
    table: torch.Tensor
    count: int
    blocks: int


def prepare_batch_table(items, device) -> Tuple[torch.Tensor, int]:
    """[(W pointer, image pointer, N, K, ldw, transpose)] -> (the device table of hoisdf_linear_emu_prepare_batch, its block total)"""
    arr = (EmuPrepItem * len(items))()
    blocks = 0
    for it, (w_ptr, image_ptr, N, K, ldw, transpose) in zip(arr, items):
        it.W, it.image, it.first_block = w_ptr, image_ptr, blocks
        it.ldw, it.N, it.K, it.transpose = ldw, N, K, int(transpose)
        blocks += lib().hoisdf_linear_emu_prepare_blocks(N, K, int(transpose))
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device), blocks


def _wait_for_readers(entries, cur) -> None:
    """before images are overwritten on ``cur``: wait for every other stream that read the previous ones (the builder included)"""
    readers = set()
    for e in entries:
        readers |= e.readers
    for s in readers:
        if s != cur:
            cur.wait_stream(s)


def _record_build(built, cur) -> None:
    """after the build of [(entry, version)] was queued on ``cur``: one event for consumers on other streams; the building stream
    counts as a reader - a rebuild from another stream has to wait for this build too"""
    ev = torch.cuda.Event()
    ev.record(cur)
    for e, version in built:
        e.version, e.built, e.build_stream = version, ev, cur
        e.readers.clear()
        e.readers.add(cur)


class WeightImageCache:
    PURGE_AT = 4096

    def __init__(self):
        self.entries = {}                    # ImageKey -> _Entry
        self.graveyard = []                  # images of weights that no longer exist, kept for one more purge cycle (see purge)
        self.epoch = 0                       # bumped whenever an entry joins or leaves: the batch tables are rebuilt
        self.tables = {}                     # device index -> _BatchTable
        self.purge_at = self.PURGE_AT

    def __len__(self) -> int:
        return len(self.entries)

    def _bury(self, key: ImageKey) -> None:
        self.graveyard.append(self.entries.pop(key).image)
        self.epoch += 1

    def purge(self) -> None:
        """Drop the entries whose weight tensor is gone.  Never touches an entry whose owner is alive: callers (the coarse
        encoder / decoder layer entries) hold only the raw device pointer of an image for the duration of their C call, so an
        image must not be freed behind a live weight.  The purged images themselves are parked until the NEXT purge (thousands
        of lookups later), far beyond any kernel that may still read them on another stream."""
        self.graveyard.clear()
        for key in [k for k, e in self.entries.items() if e.owner() is None]:
            self._bury(key)

    def get(self, W: torch.Tensor, transpose: bool, generation: int) -> torch.Tensor:
        """the image of a weight, cached per (device, storage, shape, orientation) and rebuilt in place when the weight changed
        (torch's version counter, or ``generation``, which FusedAdamW bumps).  The build is recorded with an event: a consumer on
        another HIP stream waits for it, and is remembered as a reader - a rebuild waits for every stream that read the previous
        image before overwriting it."""
        N, K = W.shape
        key = ImageKey(W.device.index, W.data_ptr(), N, K, W.stride(0), bool(transpose))
        version = (generation, W._version)
        cur = torch.cuda.current_stream(W.device)
        ent = self.entries.get(key)
        # the entry belongs to ONE tensor object (the parameter, or the parameter a slice views): another tensor that the
        # allocator later placed at the same address must not hit it
        base = W._base if W._base is not None else W
        if ent is not None and ent.owner() is not base:
            ent.version, ent.owner = None, weakref.ref(base)
        if ent is None:
            nb = lib().hoisdf_linear_emu_image_bytes(K if transpose else N, N if transpose else K)
            ent = _Entry(torch.empty(nb, device=W.device, dtype=torch.uint8), weakref.ref(base))
            if len(self.entries) >= self.purge_at:       # weights that came and went (tests): do not grow without bound
                self.purge()
                self.purge_at = max(self.PURGE_AT, 2 * len(self.entries))
            self.entries[key] = ent
            self.epoch += 1
        if ent.version != version:
            _wait_for_readers([ent], cur)
            call("hoisdf_linear_emu_prepare", C.c_void_p(W.data_ptr()), W.stride(0), N, K, int(transpose), C.c_void_p(ent.image.data_ptr()),
                 C.c_void_p(cur.cuda_stream))
            _record_build([(ent, version)], cur)
        elif ent.build_stream != cur:
            cur.wait_event(ent.built)
        ent.readers.add(cur)
        return ent.image

    def refresh(self, generation: int) -> None:
        """After an optimizer step: rebuild EVERY cached image whose parameter is alive in one launch per device
        (hoisdf_linear_emu_prepare_batch) on the current stream, instead of ~170 few-microsecond launches strewn over the next
        step's critical path.  An entry keeps its device pointer (data_ptr is in the key), so the device-side table is built once
        per cache composition."""
        by_dev = {}
        for key, ent in list(self.entries.items()):
            base = ent.owner()
            if base is None:
                continue
            # the owner must still COVER the cached address: param.data = ..., module.to() / .float(), load_state_dict(assign=True)
            # keep the Parameter object alive but free its old storage - the batch kernel must never read that
            try:
                st = base.untyped_storage()
                lo = st.data_ptr()
                covered = base.is_cuda and base.device.index == key.device and lo <= key.ptr and key.end() <= lo + st.nbytes()
            except RuntimeError:
                covered = False
            if not covered:
                self._bury(key)
                continue
            by_dev.setdefault(key.device, []).append((key, ent))
        for dev, pairs in by_dev.items():
            keys, ents = [k for k, _ in pairs], [e for _, e in pairs]
            with torch.cuda.device(dev):
                cur = torch.cuda.current_stream(dev)
                tab = self.tables.get(dev)
                if tab is None or tab.epoch != self.epoch or tab.keys != keys:       # (a weight died: never read freed memory)
                    table, blocks = prepare_batch_table(
                        [(k.ptr, e.image.data_ptr(), k.rows, k.cols, k.ld, k.transpose) for k, e in pairs], f"cuda:{dev}")
                    tab = self.tables[dev] = _BatchTable(self.epoch, keys, table, len(pairs), blocks)
                _wait_for_readers(ents, cur)
                call("hoisdf_linear_emu_prepare_batch", C.c_void_p(tab.table.data_ptr()), tab.count, tab.blocks, C.c_void_p(cur.cuda_stream))
                alive = [(e, e.owner()) for e in ents]
                _record_build([(e, (generation, base._version)) for e, base in alive if base is not None], cur)
