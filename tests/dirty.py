"""Poisoned allocations: while ``poisoned(byte)`` is active, every DEVICE tensor that comes out of one of torch's uninitialised
allocators is filled with one byte pattern, on the current stream, before the caller sees it.

The package's design rule is "no zero-initialised workspace": outputs, saved statistics, packed-weight buffers and every workspace
are ``torch.empty``, and each kernel writes what it (or its caller) later reads.  A fresh process gets zero pages and the caching
allocator mostly hands back plausible finite values, so a kernel that adds into a partial it never cleared, or skips rows of an
output somebody reads, is right in a test and wrong in a long-running process.  Under the poison it is wrong in the test.

  byte   fp32         bf16        int32 / int64                       bool
  0x00   0            0           0                                   False     the control: wrong here = wrong at this shape
  0xFF   NaN          NaN         -1                                  "true"
  0x42   48.56        48.5        1,111,638,594 / 4.77e18             "true"    finite, far outside every bound of tests/shadow.py:
                                                                                fmaxf, ordered compares and counters swallow a NaN

Covered forms (``COVERED``): ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and ``Tensor.new_empty``, patched as
attributes of ``torch`` / ``torch.Tensor``, so ``(torch.zeros if x else torch.empty)(...)`` and the allocations of the checkers are
poisoned too (harmless: they write before they read).  tests/test_dirty_host.py scans the package's source: every allocation there that
yields uninitialised memory is one of these forms, reached through the ``torch`` module or a tensor at call time.

Host and pinned tensors are left alone (``is_device``: by default ``tensor.is_cuda``).  A freshly allocated tensor owns its whole
storage, so the fill covers the storage: strided and channels-last results, and the gaps between their elements, included.  While
the current stream is capturing a graph the allocators are passed through untouched: a fill would become a node of the graph.
Everything is restored on exit."""
from __future__ import annotations

import contextlib
from typing import Callable, Optional

import pytest
import torch

PATTERNS = (0x00, 0xFF, 0x42)
# (owner, attribute): the allocators the poison wraps
COVERED = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))
COVERED_NAMES = frozenset(name for _, name in COVERED)


def _is_cuda(t: torch.Tensor) -> bool:
    return t.is_cuda


def _capturing(t: torch.Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


class Poison:
    """What ``poisoned`` yields: ``byte``, and ``fills`` / ``bytes``, the number of tensors and of bytes filled so far."""

    def __init__(self, byte: int, is_device: Optional[Callable[[torch.Tensor], bool]] = None):
        if not 0 <= int(byte) <= 255:
            raise ValueError(f"a byte pattern, not {byte!r}")
        self.byte, self.is_device = int(byte), is_device or _is_cuda
        self.fills = self.bytes = 0
        self._raw = torch.Tensor.set_                          # looked up before anything is patched

    def fill(self, t):
        if not torch.is_tensor(t) or t.numel() == 0 or not self.is_device(t) or _capturing(t):
            return t
        with torch.no_grad():
            storage = t.untyped_storage()
            raw = self._raw(torch.tensor([], dtype=torch.uint8, device=t.device), storage)      # the storage as bytes
            raw.fill_(self.byte)
        self.fills += 1
        self.bytes += storage.nbytes()
        return t

    def wrap(self, fn):
        def allocate(*args, **kwargs):
            return self.fill(fn(*args, **kwargs))
        allocate.__wrapped__ = fn
        allocate.__name__ = getattr(fn, "__name__", "allocate")
        return allocate

    def install(self, monkeypatch) -> "Poison":
        for owner, name in COVERED:
            monkeypatch.setattr(owner, name, self.wrap(getattr(owner, name)))
        return self


def poison(monkeypatch, byte: int, is_device=None) -> Poison:
    """Fixture style: active until ``monkeypatch`` is undone."""
    return Poison(byte, is_device).install(monkeypatch)


@contextlib.contextmanager
def poisoned(byte: int, is_device=None):
    mp = pytest.MonkeyPatch()
    try:
        yield poison(mp, byte, is_device)
    finally:
        mp.undo()
