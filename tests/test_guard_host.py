"""tests/guard.py on the CPU: every covered form comes back with the geometry the original allocator gives, inside intact bands; a
write one element past the end or one byte before the start is reported with its allocation, side and offset; torch is restored on
exit; the guard and dirty.poison refuse each other; and a scan of the package's source: every factory call there that sizes a
tensor is a covered form, reached through ``torch`` / a tensor at call time."""
import ast
import os

import pytest
import torch

import dirty
import guard
from test_dirty_host import _name, _package_sources
from test_dirty_host import scan as scan_uninitialised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = lambda t: True                                                          # "every tensor is a device tensor": the CPU path, forced
SMALL = 4096                                                                  # a band for the tests that do not need the real one


def _raw(t):
    return torch.tensor([], dtype=torch.uint8).set_(t.untyped_storage())


def _forms():
    like = torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    return {
        "empty": lambda: torch.empty(3, 5),
        "empty, shape as a tuple": lambda: torch.empty((7,), dtype=torch.bfloat16),
        "empty_like": lambda: torch.empty_like(like),
        "empty_like, dtype": lambda: torch.empty_like(like, dtype=torch.int32),
        "empty_like, contiguous": lambda: torch.empty_like(like, memory_format=torch.contiguous_format),
        "empty_strided": lambda: torch.empty_strided((3, 4), (8, 1), dtype=torch.int64),            # gaps between the rows
        "new_empty": lambda: like.new_empty(11, dtype=torch.bool),
        "zeros": lambda: torch.zeros(2, 9, dtype=torch.bfloat16),
        "ones": lambda: torch.ones(5, dtype=torch.int32),
        "full": lambda: torch.full((3, 3), -1, dtype=torch.int32),
        "zeros_like": lambda: torch.zeros_like(like, memory_format=torch.preserve_format),
        "ones_like": lambda: torch.ones_like(like),
        "full_like": lambda: torch.full_like(like, 2.5),
        "new_zeros": lambda: like.new_zeros(6),
        "new_ones": lambda: like.new_ones((2, 2)),
        "new_full": lambda: like.new_full((4,), 7, dtype=torch.int64),
        "zeros-or-empty": lambda: (torch.zeros if like.dim() == 0 else torch.empty)(6, dtype=torch.int32),
        "a leaf that requires grad": lambda: torch.empty(4, requires_grad=True),
        "zeros that require grad": lambda: torch.zeros(4, 2, requires_grad=True),
    }


def test_every_covered_form_keeps_the_geometry_of_the_original():
    forms = _forms()
    plain = {k: f() for k, f in forms.items()}
    with guard.guarded(ANY, band=SMALL) as g:
        made = {k: f() for k, f in forms.items()}
        assert g.fills == len(made) == len(g.allocations) and torch.empty(0).numel() == 0 and g.fills == len(made)   # an empty tensor: passed through
        assert not g.check()
        for (name, t), a in zip(made.items(), g.allocations):
            want = plain[name]
            assert (t.shape, t.stride(), t.dtype, t.device) == (want.shape, want.stride(), want.dtype, want.device), name
            assert t.is_contiguous() == want.is_contiguous(), name
            assert t.is_contiguous(memory_format=torch.channels_last) == want.is_contiguous(memory_format=torch.channels_last), name
            assert (t.requires_grad, t.is_leaf) == (want.requires_grad, want.is_leaf) and t._base is None, name
            assert t.data_ptr() % guard.ALIGN == 0 and g.of(t) is a and a.front >= SMALL and a.back == SMALL, name
            # the payload runs from the first to one past the last addressed element, and the back band begins right there
            assert a.span == guard.span_elements(t.shape, t.stride()) * t.element_size(), name
            assert t.data_ptr() == a.buffer.data_ptr() + a.front and a.buffer.numel() == a.front + a.span + a.back, name
            raw = a.buffer
            assert bool((raw[:a.front] == guard.BAND_BYTE).all()) and bool((raw[a.front + a.span:] == guard.BAND_BYTE).all()), name
            if name in ("zeros", "ones", "full", "zeros_like", "ones_like", "full_like", "new_zeros", "new_ones", "new_full", "zeros that require grad"):
                assert torch.equal(t.detach(), want.detach()), name
            else:                                                             # uninitialised forms: the payload pattern, gaps included
                assert bool((raw[a.front:a.front + a.span] == guard.PAYLOAD_BYTE).all()), name
    assert made["empty_like"].is_contiguous(memory_format=torch.channels_last) and made["empty_strided"].stride() == (8, 1)
    assert made["empty_strided"].shape == (3, 4) and g.allocations[5].span == (2 * 8 + 4) * 8          # the gaps are payload, the tail is not


def test_the_real_band_and_its_derivation():
    assert guard.BAND == 256 * 4096 * 2 == 2 ** 21 and guard.BAND % 4096 == 0
    assert guard.BAND_BYTE not in dirty.PATTERNS and guard.PAYLOAD_BYTE in dirty.PATTERNS
    with guard.guarded(ANY) as g:
        t = torch.empty(3, dtype=torch.bfloat16)
        a = g.of(t)
        assert a.back == guard.BAND and guard.BAND <= a.front < guard.BAND + guard.ALIGN and a.span == 6 and t.data_ptr() % 256 == 0
        assert not g.check()
    with pytest.raises(ValueError):
        guard.Guard(band=100)


def test_bands_stay_intact_under_ordinary_use():
    with guard.guarded(ANY, band=SMALL) as g:
        x = torch.empty(5, 7)
        x.fill_(3.0)
        x[1:4, 2:5] = -1.0
        x.t()[6].zero_()
        y = x[:, 3:].contiguous()                                             # not a covered form: torch's own output
        assert g.of(y) is None and g.of(x[2:, 1]) is g.allocations[0]         # a view lives in its base's allocation
        w = torch.zeros(4, 3, requires_grad=True)
        (w * torch.ones(4, 3)).sum().backward()
        assert w.grad is not None and bool((w.grad == 1).all())
        cl = torch.empty_like(torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))
        cl.copy_(torch.arange(120.0).view(2, 3, 4, 5))
        b = torch.empty(3, dtype=torch.bool).fill_(True)
        assert bool(b.all())
        assert not g.check() and g.fills >= 6 and all(g.of(t) is not None for t in (x, w, cl, b))


def test_a_write_just_past_the_end_is_reported():
    with guard.guarded(ANY, band=SMALL) as g:
        first, t, last = torch.empty(9), torch.empty(3, 5, dtype=torch.bfloat16), torch.zeros(2)
        a = g.of(t)
        assert a.index == 1 and not g.check()
        g.active.append("some.entry")
        inside = torch.empty(4)
        g.active.pop()
        assert g.of(inside).entry == "some.entry" and a.entry is None
        # one bf16 element behind the last one, through a byte view of the same storage: inside this test's own buffer
        end = a.front + a.span
        _raw(t)[end:end + 2] = torch.tensor([0x80, 0x3F], dtype=torch.uint8)
        damage = g.check()
        assert [(d.index, d.entry, d.side, d.offset, d.changed) for d in damage] == [(1, None, "back", 0, 2)]
        assert "back band of allocation 1" in str(damage[0])
        assert g.check([g.of(first), g.of(last)]) == [] and len(g.check([a])) == 1
        # ... and two rows of a "tile" stored past the tail, some way out: the nearest byte is what is reported
        _raw(inside)[g.of(inside).front + 16 + 40:g.of(inside).front + 16 + 48] = 0
        d = g.check([g.of(inside)])
        assert [(x.index, x.entry, x.side, x.offset, x.changed) for x in d] == [(3, "some.entry", "back", 40, 8)]


def test_a_write_just_before_the_start_is_reported():
    with guard.guarded(ANY, band=SMALL) as g:
        t = torch.empty(6, dtype=torch.int32)
        a = g.of(t)
        _raw(t)[a.front - 1] = 0
        assert [(d.index, d.side, d.offset, d.changed) for d in g.check()] == [(0, "front", -1, 1)]
        _raw(t)[a.front - 9] = 1
        assert [(d.index, d.side, d.offset, d.changed) for d in g.check()] == [(0, "front", -1, 2)]
        # a band byte rewritten with the band's own value is not damage, and neither is anything inside the payload
        u = torch.empty(4)
        _raw(u)[g.of(u).front - 1] = guard.BAND_BYTE
        u.fill_(float("nan"))
        assert g.check([g.of(u)]) == []


def test_host_tensors_empty_tensors_and_out_calls_pass_through():
    with guard.guarded(band=SMALL) as g:                                      # the default predicate: tensor.is_cuda
        a, b, c, d = torch.empty(64), torch.zeros(3), torch.zeros(2).new_full((5,), 1.0), torch.empty_strided((2, 2), (2, 1))
        assert g.fills == 0 and not g.allocations and all(g.of(t) is None for t in (a, b, c, d))
    with guard.guarded(lambda t: t.dtype == torch.float32, band=SMALL) as g:
        dev, host = torch.empty(16), torch.zeros(16, dtype=torch.int32)
        into = torch.zeros(4, out=torch.empty(4))                             # an out= call returns ITS tensor
        assert g.of(dev) is not None and g.of(host) is None and g.of(torch.empty(0)) is None and g.of(into) is not None
        assert g.fills == 2 and g.bytes == 64 + 16
        with g.pause():
            assert g.of(torch.empty(16)) is None
        assert g.of(torch.empty(16)) is not None


def test_everything_is_restored_and_the_buffers_are_held_until_then():
    before = {(o.__name__, n): getattr(o, n) for o, n, _ in guard.COVERED}
    assert "new_zeros" not in vars(torch.Tensor) and {n for _, n in dirty.COVERED} <= guard.COVERED_NAMES
    with guard.guarded(ANY, band=SMALL) as g:
        assert all(getattr(o, n).__wrapped__ is before[o.__name__, n] for o, n, _ in guard.COVERED)
        ptr = torch.empty(1000).data_ptr()                                    # dropped by the test, kept by the registry
        assert g.allocations[0].buffer.data_ptr() + g.allocations[0].front == ptr and not g.check()
    assert all(getattr(o, n) is before[o.__name__, n] for o, n, _ in guard.COVERED) and "new_zeros" not in vars(torch.Tensor)
    with pytest.raises(RuntimeError, match="inside"):
        with guard.guarded(ANY, band=SMALL):
            raise RuntimeError("inside")
    assert all(getattr(o, n) is before[o.__name__, n] for o, n, _ in guard.COVERED)
    mp = pytest.MonkeyPatch()
    g = guard.guard(mp, ANY, band=SMALL)                                      # the fixture style
    assert g.of(torch.zeros(3)) is not None
    mp.undo()
    assert all(getattr(o, n) is before[o.__name__, n] for o, n, _ in guard.COVERED)
    assert dirty.Poison.install is not guard._refuse_poison


def test_the_guard_and_the_poison_refuse_each_other():
    with dirty.poisoned(0x42, ANY):
        with pytest.raises(RuntimeError, match="must not be installed together"):
            with guard.guarded(ANY, band=SMALL):
                pass
    with guard.guarded(ANY, band=SMALL):
        with pytest.raises(RuntimeError, match="erase the bands"):
            with dirty.poisoned(0x42, ANY):
                pass
        with pytest.raises(RuntimeError, match="already wrapped"):
            with guard.guarded(ANY, band=SMALL):
                pass
    with dirty.poisoned(0x42, ANY) as p:                                      # and both work again afterwards
        assert torch.empty(3).tolist() == pytest.approx([48.564706] * 3, rel=1e-6) and p.fills == 1


# --------------------------------------------------------------------------------------------------------- the source scan
# every factory of torch that SIZES a tensor and fills it with a value (or with nothing): what the guard has to cover.  Factories
# that compute their content (arange, linspace, rand*, eye, tensor, from_numpy) are torch's own launches and not handed to a kernel
# of the package to write.
VALUE_FACTORIES = {"zeros", "ones", "full", "zeros_like", "ones_like", "full_like", "new_zeros", "new_ones", "new_full"}
FACTORIES = VALUE_FACTORIES | dirty.COVERED_NAMES
NEW_FORMS = {"new_empty", "new_zeros", "new_ones", "new_full"}


def scan(source, filename="<source>"):
    """-> 'file:line: what' for every factory call the guard would miss: the uninitialised ones by tests/test_dirty_host.py's scan,
    the value-filled ones by the same rules."""
    found = scan_uninitialised(source, filename)
    tree = ast.parse(source, filename)
    parent = {child: node for node in ast.walk(tree) for child in ast.iter_child_nodes(node)}

    def flag(node, what):
        found.append(f"{filename}:{node.lineno}: {what}")

    def is_callee(node):
        up = parent.get(node)
        if isinstance(up, ast.IfExp) and node in (up.body, up.orelse):         # (torch.zeros if x else torch.empty)(...)
            node, up = up, parent.get(up)
        return isinstance(up, ast.Call) and up.func is node

    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[0] == "torch":
            for alias in node.names:
                if alias.name in VALUE_FACTORIES:
                    flag(node, f"`from {node.module} import {alias.name}` binds the factory before the guard can replace it")
        elif isinstance(node, ast.Attribute) and node.attr in VALUE_FACTORIES:
            if _name(node).split(".")[0] in ("np", "numpy"):                   # a numpy array lives on the host: never a device tensor
                continue
            if not is_callee(node):
                flag(node, f"`{_name(node) or node.attr}` is taken as a value, not called: an alias outlives the guard's patch")
            elif node.attr not in NEW_FORMS and _name(node) != f"torch.{node.attr}":
                flag(node, f"`{_name(node) or node.attr}(...)`: the covered form is `torch.{node.attr}(...)`")
        if isinstance(node, ast.Call) and _name(node.func).split(".")[-1] in VALUE_FACTORIES and any(k.arg == "out" for k in node.keywords):
            flag(node, f"`{_name(node.func)}(..., out=)` fills a tensor the guard never sees")
    return found


def test_every_factory_call_of_the_package_is_a_covered_form():
    assert FACTORIES == guard.COVERED_NAMES                                   # the scan and the guard speak of the same forms
    found, calls, files = [], 0, 0
    for path in _package_sources():
        with open(path) as f:
            source = f.read()
        found += scan(source, os.path.relpath(path, ROOT))
        calls += sum(isinstance(n, ast.Attribute) and n.attr in FACTORIES for n in ast.walk(ast.parse(source)))
        files += 1
    assert files >= 20 and calls >= 130, (files, calls)                       # the scan did read the package
    assert not found, "\n".join(found)


def test_the_factories_that_feed_a_launch_are_covered():
    """The tensors the issue names: what denoising.py, criterion.py and optim.py hand to a kernel to write comes from these calls."""
    want = {"relation_detr_amd/denoising.py": ("torch.zeros", "torch.full"), "relation_detr_amd/criterion.py": ("torch.zeros",),
            "relation_detr_amd/optim.py": ("torch.zeros_like",)}
    for rel, names in want.items():
        with open(os.path.join(ROOT, rel)) as f:
            called = {_name(n.func) for n in ast.walk(ast.parse(f.read())) if isinstance(n, ast.Call)}
        assert set(names) <= called, (rel, sorted(set(names) - called))
        assert all(n.split(".")[-1] in guard.COVERED_NAMES for n in names)


SLIPS = {
    "an imported factory": "from torch import zeros\ndef f(n):\n    return zeros(n)\n",
    "an aliased factory": "import torch\n_alloc = torch.zeros\ndef f(n):\n    return _alloc(n)\n",
    "a factory as a default argument": "import torch\ndef f(x, alloc=torch.zeros_like):\n    return alloc(x)\n",
    "a factory through another name of torch": "import torch as th\ndef f(n):\n    return th.full((n,), 1)\n",
    "zeros with out=": "import torch\ndef f(x, n):\n    return torch.zeros(n, out=x)\n",
    "an uninitialised slip": "import torch\ndef f(x, n):\n    return x.resize_(n)\n",
    "an aliased empty": "import torch\n_alloc = torch.empty\ndef f(n):\n    return _alloc(n)\n",
}
FINE = {
    "the covered forms": "import torch\ndef f(x, n, z):\n    a = torch.zeros(n, device=x.device)\n    b = torch.full_like(x, 2)\n"
                         "    c = x.new_zeros(n)\n    d = x.new_full((n,), -1)\n    e = (torch.zeros if z else torch.empty)(n)\n"
                         "    g = torch.ones_like(x)\n    return a, b, c, d, e, g, torch.empty(n)\n",
    "factories that compute their content": "import torch\ndef f(n):\n    return torch.arange(n), torch.rand(n), torch.tensor([n]), torch.eye(n)\n",
    "numpy's host arrays": "import numpy as np\ndef f(n, a):\n    return np.zeros(n), np.zeros_like(a), np.full(n, 1)\n",
    "a variable called zeros": "def f(xs):\n    zeros = [x for x in xs if not x]\n    return zeros\n",
}


@pytest.mark.parametrize("label", list(SLIPS))
def test_the_scan_reports(label):
    assert scan(SLIPS[label]), f"the scan let {label} pass"


@pytest.mark.parametrize("label", list(FINE))
def test_the_scan_accepts(label):
    assert scan(FINE[label]) == []
