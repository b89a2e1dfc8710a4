"""Data derived from weights and kept between calls: one cache class, one ledger of what a captured graph reads.

The hot path keeps copies of weight tensors in other layouts (MFMA fragment order, concatenated projections, folded batch-norm
statistics, fp32 copies).  Two things can go wrong with such a copy, and this module is where both are handled:

  * eager calls must never use a copy whose source changed.  ``DerivedCache`` ties an entry to the source tensor OBJECTS (weak
    references) and to each source's ``(_version, data_ptr, shape, dtype, device)``: a version bump, a new address on any
    source, a new object -- also one that reproduces the old address and version -- a new dtype or device all miss;
  * a captured HIP graph has the copy's ADDRESS baked in.  While a ``Ledger`` is recording (graph.GraphedCall records during
    its warm-up and capture; ``recording()`` does for anyone else), every cache hit or build adds a ``Pin``: the derived
    tensors (a strong reference -- eviction or a rebuild for eager use can no longer free them), weak references to the
    sources with the stamps the copy was built from, and a ``fill`` that rebuilds the copy INTO the same buffers.  Before a
    replay ``refresh`` walks the ledger: an unchanged source costs two comparisons, a source that changed in place gets its
    copy rebuilt on the current stream, a source that moved, changed dtype / shape / device or died raises before anything
    is launched.  Tables without a source (RelationTransformer.level_geometry) are pinned only.

What torch does not signal: a write through ``.data`` (``p.data.mul_()``, ``p.data.copy_()``) leaves ``p._version`` where it
was.  No cache can see it; ``drop_all()`` empties every cache for eager use and ``Ledger.refresh(force=True)`` (GraphedCall.
refresh_weights) rebuilds everything a graph pinned."""
from __future__ import annotations

import contextlib
import threading
import weakref
from typing import Callable, Iterable, List, Optional, Sequence

import torch

from . import _lib

KEEP, REFRESH = "current", "refresh in place"


def stamp(t: torch.Tensor) -> tuple:
    """What torch lets a cache observe of a source tensor."""
    return (t._version, t.data_ptr(), t.shape, t.dtype, t.device)


def _flat(derived) -> tuple:
    return (derived,) if torch.is_tensor(derived) else tuple(derived)


class Pin:
    """One derived copy a graph reads.  ``fill(derived, *sources)`` must not hold a source itself (the pin would keep a replaced
    parameter alive and never learn that it was replaced)."""
    __slots__ = ("kind", "derived", "sources", "stamps", "fill")

    def __init__(self, kind: str, derived, sources: Sequence[torch.Tensor], stamps: Sequence[tuple], fill: Optional[Callable]):
        self.kind, self.derived, self.fill = kind, derived, fill
        self.sources = tuple(weakref.ref(t) for t in sources)
        self.stamps = list(stamps)

    def tensors(self) -> tuple:
        return _flat(self.derived)


class Ledger:
    """The pins of one recording, in first-use order, one per derived copy."""

    def __init__(self):
        self.pins: List[Pin] = []
        self._seen: dict = {}
        self._names: dict = {}
        self._quick: Optional[list] = None
        self._quick_pins = 0

    def record(self, kind: str, derived, sources: Sequence[torch.Tensor] = (), stamps: Optional[Sequence[tuple]] = None,
               fill: Optional[Callable] = None) -> None:
        key = tuple(id(t) for t in _flat(derived))
        if key not in self._seen:
            pin = Pin(kind, derived, sources, [stamp(t) for t in sources] if stamps is None else stamps, fill)
            self._seen[key] = pin
            self.pins.append(pin)

    def kinds(self) -> set:
        return {p.kind for p in self.pins}

    def tensors(self) -> list:
        return [t for p in self.pins for t in p.tensors()]

    def sources(self) -> list:
        """The live source tensors, each once, in first-use order."""
        out, seen = [], set()
        for p in self.pins:
            for r in p.sources:
                t = r()
                if t is not None and id(t) not in seen:
                    seen.add(id(t))
                    out.append(t)
        return out

    def name_sources(self, modules: Iterable[torch.nn.Module]) -> None:
        """Qualified parameter / buffer names for the error messages, from the modules the captured callable closes over."""
        for m in modules:
            for name, t in list(m.named_parameters()) + list(m.named_buffers()):
                self._names.setdefault(id(t), name)

    def describe(self, pin: Pin, i: int) -> str:
        t = pin.sources[i]()
        name = self._names.get(id(t)) if t is not None else None
        _, _, shape, dtype, _ = pin.stamps[i]
        return f"`{name}`" if name else f"source {i} ({str(dtype).replace('torch.', '')}{list(shape)}) of {pin.kind}"

    def refresh(self, force: bool = False) -> int:
        """Decide (replay_decision: raises before anything is launched), then rebuild what changed into the pinned buffers on the
        current stream.  Returns the number of copies rebuilt."""
        if not force and self._unchanged():
            return 0
        todo = [pin for pin, action in replay_decision(self, force) if action == REFRESH]
        for pin in todo:
            sources = [r() for r in pin.sources]
            with torch.no_grad():
                pin.fill(pin.derived, *sources)
            pin.stamps = [stamp(t) for t in sources]
        self._quick = None
        return len(todo)

    def _unchanged(self) -> bool:
        """The per-replay walk when nothing happened: each distinct source once -- alive, same version, same address, same dtype
        (a new shape or device comes with a new address).  Anything else goes through replay_decision."""
        quick = self._quick
        if quick is None or self._quick_pins != len(self.pins):
            seen = {}
            for p in self.pins:
                for r, s in zip(p.sources, p.stamps):
                    t = r()
                    if t is None or seen.setdefault(id(t), s)[:2] != s[:2]:
                        return False
            quick = self._quick = [(r, s[0], s[1], s[3]) for p in self.pins for r, s in zip(p.sources, p.stamps)]
            quick[:] = list({id(q[0]()): q for q in quick}.values())
            self._quick_pins = len(self.pins)
        for ref, version, address, dtype in quick:
            t = ref()
            if t is None or t._version != version or t.data_ptr() != address or t.dtype is not dtype:
                return False
        return True


def replay_decision(ledger: Ledger, force: bool = False) -> list:
    """``[(pin, KEEP | REFRESH)]`` for a replay of the graph that recorded ``ledger``; pure host arithmetic, launches nothing.
    REFRESH: a source changed where it stands (version bump at the same address: an in-place op, ``load_state_dict``, an
    optimizer step), or ``force``.  Raises RdetrError, naming the tensor, for a source that died, moved or changed shape, dtype
    or device: the graph's other kernels read the source itself at the captured address, so no rebuild can help."""
    plan = []
    for pin in ledger.pins:
        stale = False
        for i, (ref, old) in enumerate(zip(pin.sources, pin.stamps)):
            t = ref()
            if t is None:
                raise _lib.RdetrError(f"captured graph: {ledger.describe(pin, i)} no longer exists (the parameter object was replaced "
                                      f"or freed); the graph still reads its old storage -- capture a new GraphedCall")
            if t._version == old[0] and t.data_ptr() == old[1] and t.dtype is old[3]:
                if t.shape == old[2] and t.device == old[4]:
                    continue
            new = stamp(t)
            if new[1:] != tuple(old[1:]):
                what = ("moved to another address" if new[1] != old[1] else "changed dtype" if new[3] != old[3] else
                        "changed shape" if new[2] != old[2] else "changed device")
                raise _lib.RdetrError(f"captured graph: {ledger.describe(pin, i)} {what} since capture ({_show(old)} -> {_show(new)}); "
                                      f"the graph reads the captured address -- capture a new GraphedCall")
            stale = True
        if pin.sources and (stale or force):
            if pin.fill is None:
                raise _lib.RdetrError(f"captured graph: a source of {pin.kind} changed and the copy cannot be rebuilt in place")
            plan.append((pin, REFRESH))
        else:
            plan.append((pin, KEEP))
    return plan


def _show(s: tuple) -> str:
    return f"{str(s[3]).replace('torch.', '')}{list(s[2])}@{s[1]:#x} v{s[0]} {s[4]}"


_state = threading.local()


def active() -> Optional[Ledger]:
    return getattr(_state, "ledger", None)


@contextlib.contextmanager
def recording(ledger: Optional[Ledger] = None):
    """``with recording() as ledger: forward(...)``: every derived copy the calls of this thread use is pinned in ``ledger``."""
    ledger = Ledger() if ledger is None else ledger
    before = active()
    _state.ledger = ledger
    try:
        yield ledger
    finally:
        _state.ledger = before


def pin(kind: str, tensors: Iterable[torch.Tensor]) -> None:
    """Pin tensors that have no source tensor (tables built from shapes) in the recording ledger, if there is one."""
    ledger = active()
    if ledger is not None:
        ledger.record(kind, tuple(tensors))


_caches: "weakref.WeakSet" = weakref.WeakSet()
_droppers: list = []


def on_drop(clear: Callable[[], None]) -> None:
    """Register the ``clear`` of a cache that is not a DerivedCache (host tables), for ``drop_all``."""
    _droppers.append(clear)


def drop_all() -> None:
    """Forget every cached derived copy and table: the next eager call rebuilds from the current tensors.  The one remedy after
    a write torch does not signal (through ``.data``).  What a live graph pinned stays alive in its ledger."""
    for cache in list(_caches):
        cache.clear()
    for clear in _droppers:
        clear()


class DerivedCache:
    """Derived copies of tensors, tied to the tensor OBJECTS: an entry holds weak references to its source tensors and is only a
    hit while every reference still resolves to the very tensor passed in and every stamp (``stamp``) matches.  A freed model
    whose storage address is recycled by the caching allocator for another model's weights (same ``data_ptr()``, same
    ``_version`` after an identical build sequence) can therefore never alias a stale copy.
    Lifetime: a copy lives as long as its source tensors are alive and unchanged -- entries are never evicted by size, only
    entries whose sources are gone are pruned (every ``prune_every`` misses; ADVICE round 3: a size cap with ``clear()`` freed
    copies that live graphs of a second network still read).  A copy that is replaced because a source changed is kept alive by
    the ledgers that recorded it (module docstring)."""

    def __init__(self, prune_every: int = 64, kind: str = "derived"):
        self._entries: dict = {}
        self._prune_every = prune_every
        self._misses = 0
        self.kind = kind
        _caches.add(self)

    def get(self, tensors, build, fill: Optional[Callable] = None, kind: Optional[str] = None, extra=None):
        """``build() -> derived`` (a tensor or a tuple of tensors); ``fill(derived, *tensors)`` rebuilds it in place (for a graph's
        refresh; it must not close over a source).  ``extra``: a hashable that is part of the state (an eps)."""
        key = tuple(id(t) for t in tensors)
        ver = [stamp(t) for t in tensors]
        hit = self._entries.get(key)
        derived = None
        if hit is not None:
            refs, hver, hextra, packed = hit
            if hver == ver and hextra == extra and all(r() is t for r, t in zip(refs, tensors)):
                derived = packed
        if derived is None:
            self._misses += 1
            if self._misses % self._prune_every == 0:   # drop the entries whose tensors are gone; live ones are never evicted
                self._entries = {k: v for k, v in self._entries.items() if all(r() is not None for r in v[0])}
            derived = build()
            self._entries[key] = (tuple(weakref.ref(t) for t in tensors), ver, extra, derived)
        ledger = active()
        if ledger is not None:
            ledger.record(kind or self.kind, derived, tensors, ver, fill)
        return derived

    def clear(self) -> None:
        self._entries = {}

    def __len__(self):
        return len(self._entries)
