"""Guarded allocations: while ``guarded()`` is active, every DEVICE tensor that comes out of a covered allocator lives inside a
larger byte buffer of its own,

    [ front band | payload | back band ]

and ``Guard.check()`` says which bands a kernel wrote into.  The sibling of tests/dirty.py: that one catches a kernel that READS
memory it never wrote, this one a kernel that WRITES memory it does not own -- a row tile that stores its masked rows at a ragged
tail, a 16-byte vector store over a 2-byte remainder, a workspace one partial too short.  The caching allocator rounds every block
to 512 B and usually puts something unrelated behind it, so such a write corrupts a long-running process and no test.

Layout.  The bands hold ``BAND_BYTE`` = 0xA5, which is none of ``dirty.PATTERNS``.  The payload starts at a multiple of 256 B (the
ABI's 16-byte alignment checks behave as on a plain allocation) and the back band begins at the first byte after the payload's last
element, with no rounding: a 2-byte overrun hits the band.  The guard fills the payload itself: with 0x42 (``PAYLOAD_BYTE``, one of
dirty's patterns) for the uninitialised forms, with the values the original allocator gave for the value-filled ones.
``dirty.Poison.fill`` covers a whole storage and would erase the bands: installing the two together raises.

The tensor is ``torch.empty(0, dtype).set_(buffer.untyped_storage(), offset, size, stride)``, NOT a view of the byte buffer: its
``_base`` is None, as a fresh allocation's is (``msda_train_hm._SplitMergedProjection.backward`` tells its no-copy route by the
``_base`` of the gradients it is handed).  Size, stride, dtype, device and ``requires_grad`` are taken from the tensor the original
allocator returns for the same call, so a channels-last ``empty_like`` and the gaps of an ``empty_strided`` are kept (the span of
the payload runs to the last addressed element).

Covered forms (``COVERED``): the four of ``dirty.COVERED`` and the value-filled factories through which the package sizes tensors
that kernels write -- ``torch.zeros`` / ``torch.full`` (the label_query / box_query / noised_label of denoising.py, the cost table
of criterion.py) and ``torch.zeros_like`` (the exp_avg / exp_avg_sq of optim.py, which the AdamW kernel writes) -- with their
siblings ``ones``, ``ones_like``, ``full_like``, ``new_zeros``, ``new_ones`` and ``new_full``, so that no later call slips past.
tests/test_guard_host.py scans the package's source: every factory call there that sizes a tensor is one of these forms, reached as
``torch.<name>(...)`` or ``x.new_*(...)`` at call time.  (Factories that compute their content -- arange, rand*, tensor, eye -- are
torch's own launches; no kernel of the package is handed their result to write.)
Passed through untouched: host and pinned tensors, empty tensors, ``out=`` calls, and every allocation made while the current
stream is capturing a graph (the fills would become nodes of it).

Band size.  ``BAND`` is taken from the code, not chosen: the largest number of bytes one workgroup's row tile would store past a
ragged tail if it stored its masked rows, over all kernels of csrc/ = rows per tile x row bytes of its widest output.
  tile      csrc/ffn.hip: kFfnWaves (8) x kFfnRows (32) = 256 rows per workgroup; csrc/linear.hip (8 waves x kLinRows 32) and
            csrc/proj.hip (8 x 32) have the same 256 rows, every other kernel fewer (rowtail 32, mlp 32, qpos 16, layernorm 16)
  widest    ffn_k256_train_kernel / ffn_k256_backward write the hidden activation (hid, dH) [rows, d_ffn] in bf16, d_ffn <= 4096
            by contract (ffn_train.py, amp_train.py); the widest of linear.hip / proj.hip is encoder_proj's 480 columns
  256 rows x 4096 columns x 2 B = 2,097,152 B = 2 MiB, already a multiple of 4 KiB.
Both bands have this size.  A write that lands farther than one band from the payload is outside what this harness sees (it
lands in another allocation's band or payload, or in memory no test compares), and so is a write into the payload of ANOTHER
tensor; tests/shadow.py (``writes=True``) covers the operands of each call for the latter.

Registry.  The guard keeps a strong reference to every buffer until it is undone, with the payload span and the entry of
``Guard.active`` (tests/shadow.py pushes the name of the checked entry it is in) at allocation time.  ``check(allocations=None)``
returns one ``Damage`` per damaged band: the allocation's index and entry, "front" or "back", the signed byte offset, from the
payload's edge, of the damaged byte nearest the payload (-1 = the byte before its first, +0 = the byte after its last element),
and the number of changed bytes.  Everything is restored on exit."""
from __future__ import annotations

import contextlib
import dataclasses
from typing import Callable, Dict, Iterable, List, Optional

import pytest
import torch

import dirty

BAND = 256 * 4096 * 2            # bytes, both bands: the derivation is in the module docstring
BAND_BYTE = 0xA5
PAYLOAD_BYTE = 0x42
ALIGN = 256
assert BAND % 4096 == 0 and BAND_BYTE not in dirty.PATTERNS and PAYLOAD_BYTE in dirty.PATTERNS

# (owner, attribute, value-filled): the allocators the guard wraps
UNINITIALISED = dirty.COVERED
VALUE_FILLED = ((torch, "zeros"), (torch, "ones"), (torch, "full"), (torch, "zeros_like"), (torch, "ones_like"), (torch, "full_like"),
                (torch.Tensor, "new_zeros"), (torch.Tensor, "new_ones"), (torch.Tensor, "new_full"))
COVERED = tuple((o, n, False) for o, n in UNINITIALISED) + tuple((o, n, True) for o, n in VALUE_FILLED)
COVERED_NAMES = frozenset(name for _, name, _ in COVERED)


@dataclasses.dataclass
class Allocation:
    index: int
    buffer: torch.Tensor          # uint8, the whole [front | payload | back]
    front: int                    # bytes before the payload (BAND + what aligns the payload)
    span: int                     # bytes from the payload's first to one past its last addressed element
    back: int
    entry: Optional[str]          # the checked entry active when it was allocated
    form: str


@dataclasses.dataclass
class Damage:
    index: int
    entry: Optional[str]
    side: str                     # "front" | "back"
    offset: int                   # signed, from the payload's edge: front -1, -2, ...; back +0, +1, ...
    changed: int

    def __str__(self):
        return (f"{self.side} band of allocation {self.index} (allocated in {self.entry or 'no checked entry'}): {self.changed} bytes changed, "
                f"the nearest at {self.offset:+d}")


def span_elements(size, stride) -> int:
    """Elements from the first to one past the last one a (size, stride) geometry addresses; 0 for an empty tensor."""
    if any(s == 0 for s in size):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(size, stride))


class Guard:
    """What ``guarded`` yields.  ``allocations``: the registry; ``fills`` / ``bytes``: tensors guarded and payload bytes, as dirty.Poison
    counts them; ``byte``: the payload pattern; ``active``: the stack of entry names tests/shadow.py maintains."""

    def __init__(self, is_device: Optional[Callable[[torch.Tensor], bool]] = None, band: int = BAND):
        if band <= 0 or band % ALIGN:
            raise ValueError(f"a band of a positive multiple of {ALIGN} bytes, not {band!r}")
        self.band, self.is_device = int(band), is_device or dirty._is_cuda
        self.byte, self.fills, self.bytes = PAYLOAD_BYTE, 0, 0
        self.allocations: List[Allocation] = []
        self.by_storage: Dict[int, Allocation] = {}
        self.active: List[str] = []
        self.paused = 0
        self._set, self._empty = torch.Tensor.set_, torch.empty                # looked up before anything is patched

    # -------------------------------------------------------------------------------------------------------- allocation
    def rehouse(self, t, form: str, keep_values: bool):
        if (not torch.is_tensor(t) or self.paused or t.numel() == 0 or t.layout != torch.strided or not self.is_device(t)
                or dirty._capturing(t)):
            return t
        size, stride, item = tuple(t.shape), tuple(t.stride()), t.element_size()
        span = span_elements(size, stride) * item
        with torch.no_grad():
            buffer = self._empty(self.band + ALIGN + span + self.band, dtype=torch.uint8, device=t.device)
            front = self.band + (-(buffer.data_ptr() + self.band)) % ALIGN
            buffer = buffer[:front + span + self.band]
            buffer[:front].fill_(BAND_BYTE)
            buffer[front:front + span].fill_(PAYLOAD_BYTE)
            buffer[front + span:].fill_(BAND_BYTE)
            new = self._set(self._empty(0, dtype=t.dtype, device=t.device), buffer.untyped_storage(), front // item, size, stride)
            if keep_values:
                new.copy_(t)
        if t.requires_grad:
            new.requires_grad_(True)
        a = Allocation(len(self.allocations), buffer, front, span, self.band, self.active[-1] if self.active else None, form)
        self.allocations.append(a)
        self.by_storage[buffer.untyped_storage().data_ptr()] = a
        self.fills += 1
        self.bytes += span
        return new

    def wrap(self, fn, form: str, keep_values: bool):
        def allocate(*args, **kwargs):
            t = fn(*args, **kwargs)
            return t if kwargs.get("out") is not None else self.rehouse(t, form, keep_values)
        allocate.__wrapped__ = fn
        allocate.__name__ = getattr(fn, "__name__", "allocate")
        allocate.guard = self
        return allocate

    def install(self, monkeypatch) -> "Guard":
        for owner, name, _ in COVERED:
            if getattr(getattr(owner, name), "__wrapped__", None) is not None:
                raise RuntimeError(f"{owner.__name__}.{name} is already wrapped (dirty.poison or another guard): the poison's fill covers the "
                                   "whole storage and would erase the bands, the two must not be installed together")
        for owner, name, keep_values in COVERED:
            monkeypatch.setattr(owner, name, self.wrap(getattr(owner, name), name, keep_values))
        monkeypatch.setattr(dirty.Poison, "install", _refuse_poison)
        return self

    @contextlib.contextmanager
    def pause(self):
        """Allocations pass through untouched inside (the float64 references of a checker: no kernel writes them)."""
        self.paused += 1
        try:
            yield self
        finally:
            self.paused -= 1

    # ------------------------------------------------------------------------------------------------------------- checks
    def of(self, t) -> Optional[Allocation]:
        """The allocation whose storage ``t`` lives in, or None."""
        return self.by_storage.get(t.untyped_storage().data_ptr()) if torch.is_tensor(t) and t.layout == torch.strided else None

    def band_bytes(self, allocations: Optional[Iterable[Allocation]] = None) -> int:
        return sum(a.front + a.back for a in (self.allocations if allocations is None else allocations))

    def check(self, allocations: Optional[Iterable[Allocation]] = None) -> List[Damage]:
        todo = list(self.allocations if allocations is None else allocations)
        if not todo:
            return []
        with torch.no_grad(), self.pause():
            counts = []
            for a in todo:
                counts += [(a.buffer[:a.front] != BAND_BYTE).sum(), (a.buffer[a.front + a.span:] != BAND_BYTE).sum()]
            by_device: Dict[torch.device, List[int]] = {}
            for i, c in enumerate(counts):
                by_device.setdefault(c.device, []).append(i)
            values = [0] * len(counts)
            for idx in by_device.values():                                       # one read back per device, not per band
                for i, v in zip(idx, torch.stack([counts[i] for i in idx]).tolist()):
                    values[i] = int(v)
            found = []
            for k, a in enumerate(todo):
                if values[2 * k]:
                    hit = torch.nonzero(a.buffer[:a.front] != BAND_BYTE).reshape(-1)
                    found.append(Damage(a.index, a.entry, "front", int(hit.max()) - a.front, values[2 * k]))
                if values[2 * k + 1]:
                    hit = torch.nonzero(a.buffer[a.front + a.span:] != BAND_BYTE).reshape(-1)
                    found.append(Damage(a.index, a.entry, "back", int(hit.min()), values[2 * k + 1]))
        return found


def _refuse_poison(self, monkeypatch):
    raise RuntimeError("dirty.poison under an installed guard: the poison's fill covers the whole storage and would erase the bands")


def guard(monkeypatch, is_device=None, band: int = BAND) -> Guard:
    """Fixture style: active until ``monkeypatch`` is undone."""
    return Guard(is_device, band).install(monkeypatch)


@contextlib.contextmanager
def guarded(is_device=None, band: int = BAND):
    mp = pytest.MonkeyPatch()
    try:
        yield guard(mp, is_device, band)
    finally:
        mp.undo()
