"""``Shadow(writes=True)`` (tests/shadow.py) on the CPU, with stub entries: an operand that is not in the entry's write set must come
back bit-identical, a declared ``out`` view may change nothing of its storage but its own elements, and the bands of tests/guard.py
are checked after every entry and once more at the end.  Needs neither a GPU nor the built library."""
import math

import pytest
import torch

import guard
import shadow
from relation_detr_amd import _lib

ANY = lambda t: True                                                          # noqa: E731
BAND = 4096


@pytest.fixture
def harness(monkeypatch):
    """-> make(name, fn, writes, fault=None, guarded=False): the harness's wrapper of the stub entry `fn` under the op name `name`."""
    import types
    stub = types.SimpleNamespace(**{name: (lambda *args: 0) for name in _lib.SIGNATURES})
    monkeypatch.setattr(_lib, "load", lambda: stub)

    def make(name, fn, writes, fault=None, guarded=False):
        g = guard.guard(monkeypatch, ANY, band=BAND) if guarded else None
        sh = shadow.Shadow(monkeypatch, fault=fault, writes=True, guard=g)
        monkeypatch.setitem(shadow.WRITES, name, writes)
        checker = lambda a, res: [shadow.Cmp("out", res, a["x"].double() * 2)]                          # noqa: E731
        return sh, sh._checked(name, fn, checker)
    return make


def double(x, w, out=None, extras=None):
    """The stub entry: out = 2 x.  `w` and whatever `extras` holds are read-only operands."""
    if out is None:
        out = torch.empty_like(x)
    out.copy_(x * 2)
    return out


def _writes(sh):
    return [r for r in sh.records if r.kind == "writes"]


def test_a_clean_call_records_one_more_record_under_the_same_op(harness):
    sh, fn = harness("stub.double", double, ("out",))
    x, w = torch.randn(5, 8), torch.randn(3)
    w[1] = float("nan")                                                        # a NaN operand equals itself
    fn(x, w, extras={"table": torch.arange(4), "pair": (torch.zeros(2), [torch.ones(1, dtype=torch.bool)])})
    assert [(r.op, r.kind, r.failing) for r in sh.records] == [("stub.double", "writes", 0), ("stub.double", "values", 0)]
    assert sh.called() == {"stub.double"} and sh.checked["stub.double"] == 40
    # x, w and the four tensors inside the dict / tuple / list were compared; no out= was handed in, so no storage was watched
    assert sh.write_checks["operand_bits"] == 40 + 3 + 4 + 2 + 1 and sh.write_checks["outside_view"] == 0
    sh.assert_ok({"stub.double"})
    text = sh.report("stub")
    assert "writes: checked / bad" in text and "write checks: declared 0, operand_bits 50" in text


def _bump(t, how):
    flat = t.view(-1)
    if how == "one element":
        flat[3] += 1.0
    elif how == "the sign bit of a zero":
        flat[3] = -0.0
    elif how == "a NaN's payload":
        flat.view(torch.int32)[3] = 0x7FC00001                                # a quiet NaN with another payload


@pytest.mark.parametrize("how", ["one element", "the sign bit of a zero", "a NaN's payload"])
@pytest.mark.parametrize("where", ["w", "extras.pair[1][0]"])
def test_an_undeclared_operand_changed_in_one_element_fails(harness, how, where):
    def scribbling(x, w, out=None, extras=None):
        _bump(w if where == "w" else extras["pair"][1][0], how)
        return double(x, w, out, extras)
    sh, fn = harness("stub.double", scribbling, ("out",))
    w, inner = torch.zeros(6), torch.zeros(6)
    if how == "a NaN's payload":
        w[3] = inner[3] = float("nan")
        assert w.view(torch.int32)[3].item() == 0x7FC00000
    fn(torch.randn(4, 8), w, extras={"pair": (torch.zeros(2), [inner])})
    (r,) = _writes(sh)
    assert r.failing == 1 and math.isinf(r.ratio) and f"`{where}`" in r.where and "flat index 3" in r.where, r
    assert [x.op for x in sh.failures()] == ["stub.double"]
    with pytest.raises(AssertionError, match="not in the write set"):
        sh.assert_ok()


def test_a_declared_operand_may_change_and_an_operand_aliasing_it_too(harness):
    sh, fn = harness("stub.double", double, ("out",))
    x, out = torch.randn(4, 8), torch.zeros(4, 8)
    fn(x, torch.randn(3), out=out)
    assert torch.equal(out, x * 2) and sh.write_checks["outside_view"] == 0     # the view is its whole storage: nothing outside
    # in place, as frozen_bn_act_forward(x, ..., out=x): x overlaps a declared operand by its byte range and counts as written
    y = torch.randn(4, 8)
    fn(y, torch.randn(3), out=y)
    # ... a view of out's rows handed in as a read-only operand as well
    z = torch.zeros(6, 8)
    fn(z[1:5].clone(), z[2:3], out=z[1:5])
    sh.assert_ok({"stub.double"})
    assert all(r.failing == 0 for r in _writes(sh)) and sh.write_checks["outside_view"] == 2 * 8 * 4


def test_a_declared_in_place_operand_by_another_name(harness):
    def zero_rows_(x, w):
        x[::2] = 0
        return x
    sh = harness("stub.zero_rows_", zero_rows_, ("x",))[0]
    fn = sh._checked("stub.zero_rows_", zero_rows_, lambda a, res: [shadow.Cmp("out", res, a["x"].double() * torch.tensor([0.0, 1, 0, 1]).view(4, 1))])
    fn(torch.randn(4, 3), torch.randn(2))
    sh.assert_ok({"stub.zero_rows_"})
    # the same function with nothing declared: its write is a finding
    sh2 = harness("stub.zero_rows_", zero_rows_, ())[0]
    fn2 = sh2._checked("stub.zero_rows_", zero_rows_, lambda a, res: [shadow.Cmp("out", res, res)])
    fn2(torch.randn(4, 3) + 5, torch.randn(2))
    (r,) = _writes(sh2)
    assert r.failing == 6 and "`x`" in r.where


@pytest.mark.parametrize("slice_of", ["columns", "rows"])
def test_a_declared_out_slice_whose_neighbour_changed_fails(harness, slice_of):
    wide = torch.full((6, 24), 7.0)
    out = wide[:, 8:16] if slice_of == "columns" else wide[1:5, :8]
    x = torch.randn(*out.shape)

    def clean(x, w, out=None, extras=None):
        return double(x, w, out, extras)

    def spilling(x, w, out=None, extras=None):
        res = double(x, w, out, extras)
        if slice_of == "columns":
            wide[2, 16] = 1.1                                                   # the first element of the neighbour column
        else:
            wide[5, 0] = 1.1                                                    # the first element of the row behind the slice
        return res
    sh, fn = harness("stub.double", clean, ("out",))
    fn(x, torch.randn(3), out=out)
    sh.assert_ok({"stub.double"})
    assert sh.write_checks["outside_view"] == (6 * 24 - out.numel()) * 4
    sh, fn = harness("stub.double", spilling, ("out",))
    fn(x, torch.randn(3), out=out)
    (r,) = _writes(sh)
    first = (2 * 24 + 16) * 4 if slice_of == "columns" else 5 * 24 * 4
    assert r.failing == 4 and "changed outside the view" in r.where and f"storage byte {first}" in r.where, r
    with pytest.raises(AssertionError):
        sh.assert_ok()


def test_a_dict_key_is_declared_by_its_dotted_name(harness):
    def fills(x, w, out=None, extras=None):
        extras["out_plus_one"].copy_(x + 1)
        return double(x, w, out, extras)
    x = torch.randn(2, 4)
    sh, fn = harness("stub.double", fills, ("out", "extras.out_plus_one"))
    fn(x, torch.randn(3), extras={"out_plus_one": torch.zeros(2, 4), "pos": torch.randn(2, 4)})
    sh.assert_ok({"stub.double"})
    sh, fn = harness("stub.double", fills, ("out",))
    fn(x, torch.randn(3), extras={"out_plus_one": torch.zeros(2, 4), "pos": torch.randn(2, 4)})
    assert _writes(sh)[0].failing == 8 and "`extras.out_plus_one`" in _writes(sh)[0].where


def test_a_callable_rule_names_the_tensors_of_an_object(harness):
    class Holder:
        def __init__(self):
            self.p, self.g = torch.nn.Parameter(torch.ones(4)), torch.full((4,), 0.5)

    def step(self):
        with torch.no_grad():
            self.p -= self.g
    checker = lambda a, res: [shadow.Cmp("p", a["self"].p, torch.full((4,), 0.5, dtype=torch.float64))]        # noqa: E731
    checker.snapshot = lambda a: dict(a)
    sh = harness("stub.step", step, lambda a: [a["self"].p])[0]
    h = Holder()
    sh._checked("stub.step", step, checker)(h)
    sh.assert_ok({"stub.step"})
    # the optimizer walk: parameters, gradients and state are operands; the rules of the two FusedAdamW entries
    p, q = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    opt = torch.optim.SGD([p, q], lr=0.1, momentum=0.9)
    p.grad = torch.ones(3)
    opt.state[p]["momentum_buffer"] = torch.zeros(3)
    paths = [path for path, _ in shadow.operand_tensors(opt, "self")]
    assert paths == ["self.param[0]", "self.param[0].grad", "self.state[0].momentum_buffer", "self.param[1]"]
    allowed = shadow.WRITES["optim.FusedAdamW._step_fused"]({"self": opt})
    assert [id(t) for t in allowed] == [id(p), id(opt.state[p]["momentum_buffer"])] and shadow.WRITES["optim.FusedAdamW._clip_fused"]({"self": opt}) == []


def test_band_damage_is_reported_against_the_entry_and_later_damage_at_the_end(harness):
    stray = {}

    def past_the_end(name, call, args, result, fn):
        if call == 1:                                                           # one element behind the returned tensor, in its own buffer
            raw = shadow.storage_bytes(result)
            end = (result.storage_offset() + result.numel()) * result.element_size()
            raw[end:end + 4] = 0
        if call == 2:                                                           # a later call damages the FIRST call's result
            raw = shadow.storage_bytes(stray["first"])
            raw[stray["first"].storage_offset() * 4 - 1] = 0
        return result
    sh, fn = harness("stub.double", double, ("out",), fault=past_the_end, guarded=True)
    g = sh.guard
    x, w = torch.randn(4, 8), torch.randn(3)
    assert g.of(x) is None and g.of(w) is None                                  # torch.randn is no covered form
    stray["first"] = fn(x, w)
    assert g.of(stray["first"]).entry == "stub.double" and not sh.failures() and sh.write_checks["bands"] == 2 * BAND + g.of(stray["first"]).front - BAND
    fn(x, w)
    (r,) = sh.failures()
    assert (r.op, r.call, r.kind, r.failing) == ("stub.double", 1, "writes", 4) and "back band of allocation 1 (allocated in stub.double)" in r.where
    assert "the nearest at +0" in r.where
    fn(x, w)                                                                    # its own buffers are clean: nothing new is recorded ...
    assert len(sh.failures()) == 1 and not sh.errors
    with pytest.raises(AssertionError, match="a later launch wrote into the front band of allocation 0"):
        sh.assert_ok()                                                          # ... the end-of-case pass finds it
    assert len(sh.errors) == 1 and "allocated in stub.double" in sh.errors[0] and "the nearest at -1" in sh.errors[0]
    assert sh.finish_bands() == []                                              # once
    # the harness's own copies and the checker's references were not guarded: three results and nothing else
    assert g.fills == 3


def test_operand_storage_bands_are_checked_with_the_entry(harness):
    def before_the_operand(name, call, args, result, fn):
        w = args["w"]
        shadow.storage_bytes(w)[w.storage_offset() * w.element_size() - 2] = 1
        return result
    sh, fn = harness("stub.double", double, ("out",), fault=before_the_operand, guarded=True)
    w = torch.zeros(3)                                                          # guarded: allocated outside any entry
    fn(torch.randn(2, 2), w)
    (r,) = sh.failures()
    assert r.kind == "writes" and "front band of allocation 0 (allocated in no checked entry)" in r.where and "-2" in r.where


def test_the_defaults_are_off_and_a_guard_needs_writes(harness, monkeypatch):
    sh = shadow.Shadow(monkeypatch)
    assert not sh.writes and sh.guard is None
    fn = sh._checked("stub.double", double, lambda a, res: [shadow.Cmp("out", res, a["x"].double() * 2)])
    w = torch.zeros(3)
    fn(torch.randn(2, 2), w)
    assert [r.kind for r in sh.records] == ["values"] and "writes" not in sh.report()
    with pytest.raises(ValueError):
        shadow.Shadow(monkeypatch, guard=object())
    # an entry without a rule is an error of the harness, not a pass
    sh = shadow.Shadow(monkeypatch, writes=True)
    sh._checked("stub.unknown", double, lambda a, res: [shadow.Cmp("out", res, res)])(torch.randn(2, 2), w)
    assert sh.errors == ["`stub.unknown` has no WRITES entry"]
